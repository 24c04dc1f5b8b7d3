"""Pins from the REFERENCE ITSELF: tests/golden/ref_*.npz hold what the reference's own routines -- compiled unmodified from
/root/reference by oracle/ref/Makefile, driven by oracle/ref/ref_harness.F90 -- return on the inputs of tests/golden/refvec.py
(generator: tests/golden/make_ref_golden.py).  Here the host mirror (cice5_amd/blocks.py) and the C restatement (oracle/) are
held against them, bit for bit; tests/test_ref_pins_gpu.py does the same for the HIP kernels.

Covered (the ghost-cell part of f-3):
  create_blocks (ice_blocks.F90:111), create_distribution cartesian (ice_distribution.F90:535) incl. land-block elimination
  (ice_domain.F90:387-441), ice_HaloUpdate 2DR8 / 3DR8 / 2DI4 for every field location x field type on cyclic / open /
  closed / tripole grids in 1 and 16 (padded) blocks, ice_HaloUpdate_stress, bound_state (ice_state.F90:173),
  ice_strength (ice_mechred.F90:2111), global_minval;
  the dynamics slice (evp_prep1 .. principal_stress, alone and as evp()'s chain) and the remap slice (make_masks .. update_fields
  of ice_transport_remap.F90, alone and as horizontal_remap's chain, with the count of the triangle branches entered).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from cice5_amd import blocks, constants as C
from oracle import orc
from tests.golden import refvec as rv

HERE = os.path.dirname(os.path.abspath(__file__))


def load(cfg):
    return np.load(os.path.join(HERE, "golden", f"ref_{cfg}.npz"))


def cases(cfg, z):
    nbt = ((rv.CONFIGS[cfg][0] - 1) // rv.CONFIGS[cfg][2] + 1) * ((rv.CONFIGS[cfg][1] - 1) // rv.CONFIGS[cfg][3] + 1)
    for ew, ns, land in rv.BOUNDARIES:
        if land == "landblock" and nbt == 1:
            continue
        case = rv.case_name(ew, ns, land)
        assert f"{case}/aborted" not in z.files, f"the reference aborted on {cfg} {case}: regenerate with a valid case"
        yield ew, ns, land, case


def decomp(cfg, z, ew, ns, case, nprocs=1, rank=0, shape="slenderX1"):
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    loc = z[f"{case}/blocks/blockLocation"]
    return blocks.create_distrb_cart(nx, ny, bx, by, nprocs=nprocs, rank=rank, ew_boundary_type=ew, ns_boundary_type=ns,
                                     processor_shape=shape, work_per_block=(loc != 0).astype(int))


@pytest.mark.parametrize("cfg", list(rv.CONFIGS))
def test_create_blocks_equals_reference(cfg):
    """every member of the reference's `block` type (ice_blocks.F90:22-35) for every block, all boundary types"""
    z = load(cfg)
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    n = 0
    for ew, ns, land, case in cases(cfg, z):
        bl = blocks.create_blocks(nx, ny, bx, by, ew, ns)
        desc, ig, jg = z[f"{case}/blocks/desc"], z[f"{case}/blocks/i_glob"], z[f"{case}/blocks/j_glob"]
        assert len(bl) == len(desc)
        for b, d, i_glob, j_glob in zip(bl, desc, ig, jg):
            assert (b.block_id, b.iblock, b.jblock, b.ilo, b.ihi, b.jlo, b.jhi, int(b.tripole)) == tuple(d), (case, d)
            assert np.array_equal(b.i_glob, i_glob), (case, d, b.i_glob, i_glob)
            assert np.array_equal(b.j_glob, j_glob), (case, d, b.j_glob, j_glob)
            n += 1
    assert n >= 7


@pytest.mark.parametrize("cfg", [c for c in rv.CONFIGS if rv.CONFIGS[c][4] > 1])
def test_cartesian_distribution_equals_reference(cfg):
    """blockLocation / blockLocalID of create_distrb_cart for 1, 2, 3, 4, 8 ranks, slenderX1 / slenderX2, with and without
    eliminated land blocks; and the local block list (create_local_block_ids)"""
    z = load(cfg)
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    for ew, ns, land, case in cases(cfg, z):
        d = decomp(cfg, z, ew, ns, case)
        assert np.array_equal(d.block_location, z[f"{case}/blocks/blockLocation"])
        assert [b.block_id for b in d.local_blocks] == list(z[f"{case}/blocks/blocks_ice"])
        lid = np.zeros(len(d.all_blocks), dtype=np.int32)
        for b in d.local_blocks:
            lid[b.block_id - 1] = b.local_id
        assert np.array_equal(lid, z[f"{case}/blocks/blockLocalID"])
        for nprocs, shape in rv.DISTRIBUTIONS:
            want_loc, want_lid = z[f"{case}/distrb/{nprocs}_{shape}/blockLocation"], z[f"{case}/distrb/{nprocs}_{shape}/blockLocalID"]
            got_lid = np.zeros_like(want_lid)
            for r in range(nprocs):
                dr = decomp(cfg, z, ew, ns, case, nprocs=nprocs, rank=r, shape=shape)
                assert np.array_equal(dr.block_location, want_loc), (case, nprocs, shape)
                for b in dr.local_blocks:
                    got_lid[b.block_id - 1] = b.local_id
            assert np.array_equal(got_lid, want_lid), (case, nprocs, shape)


def mpi_semantics(serial_out, inp, fill):
    """The fixtures come from the reference's SERIAL backend (serial/ice_boundary.F90), the only one that builds here; the
    production backend (mpi/ice_boundary.F90), which oracle and kernels follow, differs in ONE documented way: before the
    copies it overwrites the outermost nghost rows / columns of every block array with the fill value (mpi/ice_boundary.F90:
    1409-1416 "fill out halo region ... for halo grid cells that are not updated"), where the serial code leaves a ghost
    cell that no message writes (open / closed boundary) as it was.  Every input cell carries its own random value, so a
    cell the serial update left alone is one whose output equals its input."""
    e = serial_out.copy()
    ring = np.zeros(serial_out.shape, dtype=bool)
    ring[..., 0, :] = ring[..., -1, :] = ring[..., :, 0] = ring[..., :, -1] = True
    e[ring & (serial_out == inp)] = fill
    return e


def _ghost_report(d, got, want, inp):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return [(tuple(int(x) for x in k), float(got[tuple(k)]), float(want[tuple(k)]), float(inp[tuple(k)])) for k in bad[:6]], len(bad)


@pytest.mark.parametrize("cfg", list(rv.CONFIGS))
def test_halo_update_r8_equals_reference(cfg):
    """orc_halo_r8 == ice_HaloUpdate2DR8 / 3DR8 (serial/ice_boundary.F90:630, :1440) on every cell of every block"""
    z = load(cfg)
    checked = 0
    for ew, ns, land, case in cases(cfg, z):
        d = decomp(cfg, z, ew, ns, case)
        for key, nz, loc, typ, fill in rv.HALO_R8:
            inp = rv.halo_r8_input(cfg, case, key, d.nblocks, d.ny_block, d.nx_block, nz)
            want = mpi_semantics(z[f"{case}/halo_r8/{key}"], inp, 0.0 if fill is None else fill)
            got = inp.copy()
            kind = C.KIND_VECTOR if typ in (rv.TYPE["vector"], rv.TYPE["angle"]) else C.KIND_SCALAR
            if nz:
                for k in range(nz):
                    w = np.ascontiguousarray(got[:, k]); orc.halo_r8(d, w, loc, kind, 0.0 if fill is None else fill); got[:, k] = w
            else:
                orc.halo_r8(d, got, loc, kind, 0.0 if fill is None else fill)
            rep, nbad = _ghost_report(d, got, want, inp)
            assert nbad == 0, (cfg, case, key, nbad, rep)
            checked += 1
    assert checked >= 7 * len(rv.HALO_R8)


@pytest.mark.parametrize("cfg", list(rv.CONFIGS))
def test_halo_update_i4_and_stress_equal_reference(cfg):
    """orc_halo_i4 == ice_HaloUpdate2DI4 (:1170), orc_halo_stress == ice_HaloUpdate_stress (:3269)"""
    z = load(cfg)
    for ew, ns, land, case in cases(cfg, z):
        d = decomp(cfg, z, ew, ns, case)
        for key, loc, typ, fill in rv.HALO_I4:
            inp = rv.halo_i4_input(cfg, case, key, d.nblocks, d.ny_block, d.nx_block)
            got = inp.copy()
            orc.halo_i4(d, got, 0 if fill is None else fill)
            want = mpi_semantics(z[f"{case}/halo_i4/{key}"], inp, 0 if fill is None else fill)
            assert np.array_equal(got, want), (cfg, case, key, np.argwhere(got != want)[:5])
        a1 = rv.halo_r8_input(cfg, case, "stress1", d.nblocks, d.ny_block, d.nx_block, 0)
        a2 = rv.halo_r8_input(cfg, case, "stress2", d.nblocks, d.ny_block, d.nx_block, 0)
        got = a1.copy()
        orc.halo_stress(d, got, a2)
        want = z[f"{case}/halo_stress/center_scalar"]
        rep, nbad = _ghost_report(d, got, want, a1)
        assert nbad == 0, (cfg, case, nbad, rep)
        if ns != "tripole" and land not in ("landblock",) and not (cfg == "g26x18_b8x5" and ew == "closed"):
            assert np.array_equal(want, a1)          # without eliminated land blocks the stress update touches tripole grids only


@pytest.mark.parametrize("cfg", list(rv.CONFIGS))
def test_bound_state_equals_reference(cfg):
    """bound_state (ice_state.F90:173-238) == a centre / scalar halo update of every category and tracer plane"""
    z = load(cfg)
    n = 0
    for ew, ns, land, case in cases(cfg, z):
        if f"{case}/bound/aicen" not in z.files:
            continue
        d = decomp(cfg, z, ew, ns, case)
        mxb = rv.CONFIGS[cfg][4]
        aicen, vicen, vsnon, trcrn = rv.state_input(cfg, case, mxb, d.ny_block, d.nx_block, 3)
        assert bool(z[f"{case}/bound/trcrn_beyond_ntrcr_untouched"])
        for name, arr in (("aicen", aicen), ("vicen", vicen), ("vsnon", vsnon), ("trcrn", trcrn[:, :, :3].reshape(mxb, -1, d.ny_block, d.nx_block))):
            got = np.ascontiguousarray(arr[:d.nblocks]).copy()
            want = mpi_semantics(z[f"{case}/bound/{name}"].reshape(d.nblocks, -1, d.ny_block, d.nx_block), got, 0.0)
            for k in range(got.shape[1]):
                w = np.ascontiguousarray(got[:, k]); orc.halo_r8(d, w, C.LOC_CENTER, C.KIND_SCALAR, 0.0); got[:, k] = w
            assert np.array_equal(got, want), (cfg, case, name, np.argwhere(got != want)[:5])
            n += 1
    assert n >= 8


def test_ice_strength_equals_reference():
    """orc_ice_strength == ice_strength (ice_mechred.F90:2111-2269; asum_ridging, ridge_itd) for Rothrock with both
    participation / redistribution functions and for Hibler's formula.  The Fortran evaluates exp() with the compiler's
    intrinsic, the restatement (and the kernel) with the fixed algorithm of orc_exp (< 1 ulp): wherever exp enters
    (krdg_partic = 1, krdg_redist = 1, kstrength = 0) the result may differ in the last bits; everything else is bit-exact."""
    cfg = "g24x16_b24x16"
    z = load(cfg)
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    nxb, nyb = bx + 2, by + 2
    case = "cyclic_open"
    report = {}
    for ks, kp, kr in rv.STRENGTH_CASES:
        for rep in (0, 1):
            tag = f"k{ks}{kp}{kr}_{rep}"
            s = rv.strength_input(cfg, tag, nyb, nxb)
            want = z[f"{case}/strength/{tag}"]
            p = orc.make_params(3600.0, 120, 1.0e4, strength_mode=1, kstrength=ks, krdg_partic=kp, krdg_redist=kr, ncat=rv.NCAT,
                                mu_rdg=rv.MU_RDG, Cf=rv.CF)
            got = orc.ice_strength_block(nxb, nyb, 2, nxb - 1, 2, nyb - 1, s["indxi"], s["indxj"], s["aice"], s["vice"], s["aice0"],
                                         s["aicen"], s["vicen"], p)
            assert len(s["indxi"]) > 200
            if ks == 1:
                on = np.zeros((nyb, nxb), dtype=bool); on[s["indxj"] - 1, s["indxi"] - 1] = True
                assert np.all(want[~on] == 0.0) and np.all(got[~on] == 0.0)
            else:
                on = np.zeros((nyb, nxb), dtype=bool); on[1:-1, 1:-1] = True
            assert np.all(np.isfinite(want))
            nz = want[on] != 0
            assert nz.sum() > 50, (tag, nz.sum())
            rel = np.abs(got[on] - want[on]) / np.maximum(np.abs(want[on]), 1e-300)
            report[tag] = (int((got[on] != want[on]).sum()), int(on.sum()), float(rel.max()))
            uses_exp = (ks == 0) or kp == 1 or kr == 1
            if not uses_exp:
                assert np.array_equal(got, want), (tag, report[tag])
            else:
                assert rel.max() <= 4.5e-16, (tag, report[tag])      # 2 ulp
    print("ice_strength vs reference (cells differing, cells, max rel diff):", report)


@pytest.mark.parametrize("cfg", list(rv.CONFIGS))
def test_global_minval_equals_reference(cfg):
    """set_evp_parameters' xmin = global_minval(dxt, distrb_info, tmask) (ice_dyn_shared.F90:221): physical cells only"""
    z = load(cfg)
    for ew, ns, land, case in cases(cfg, z):
        d = decomp(cfg, z, ew, ns, case)
        dx = 1000.0 * (1.0 + rv.halo_r8_input(cfg, case, "minval", d.nblocks, d.ny_block, d.nx_block, 0) ** 2)
        msk = rv.halo_i4_input(cfg, case, "minval_mask", d.nblocks, d.ny_block, d.nx_block) % 10 > 3
        phys = np.zeros_like(msk)
        for n, b in enumerate(d.local_blocks):
            phys[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
        assert dx[msk & phys].min() == float(z[f"{case}/global_minval"])


def test_compute_tracers_equals_reference():
    """orc_compute_tracers == compute_tracers (ice_itd.F90:1359-1501, the arithmetic of work_to_state in transport_upwind):
    tracers on the area, the ice and snow volumes, on the level-ice / pond / brine fractions; Tsfc takes Tocnfrz and fbri 1
    where there is no ice, bit for bit."""
    import ctypes as ct
    cfg = "g24x16_b24x16"
    z = load(cfg)
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    nxb, nyb = bx + 2, by + 2
    L = orc.lib()
    for tag, (dep, n_tsfc, n_alvl, n_apnd, n_fbri, pond) in rv.TRACER_CASES.items():
        nt = len(dep)
        a, v, sn, atr = rv.tracers_input(cfg, tag, nyb, nxb, nt)
        want = z[f"cyclic_open/tracers/{tag}"]
        got = np.full((nt, nyb, nxb), 7.0)
        dp = np.asarray(dep, dtype=np.int32)
        L.orc_compute_tracers.argtypes = [ct.c_int] * 3 + [orc.c_i32p] + [ct.c_int] * 7 + [ct.c_double] + [orc.c_f64p] * 5
        L.orc_compute_tracers(nxb, nyb, nt, orc._p32(dp), n_tsfc, n_alvl, n_apnd, n_fbri, *pond, rv.TOCNFRZ,
                              orc._p64(atr), orc._p64(a), orc._p64(v), orc._p64(sn), orc._p64(got))
        assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:5])
        assert (want[0] == rv.TOCNFRZ).any() and np.abs(want).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# The slice fixtures tests/golden/ref_dyn_*.npz (tests/golden/make_ref_kernels.py): the reference's own evp_prep1, evp_prep2,
# stress, stepu, evp_finish and principal_stress, cut out of ice_dyn_shared / ice_dyn_evp at build time (oracle/ref/Makefile,
# target `kernels`; driver oracle/ref/ref_kernels.F90).  Single-routine records pin each routine on one block; chain records
# pin the whole call order of evp() on the whole grid with the reference's own halo updates in between.
# NOT pinned: the T<->U averages to_ugrid / t2ugrid_vector / u2tgrid_vector (ice_grid cannot be built): aiu, umass, the U-grid
# wind stress handed to the chain and the last average of strocnxT / strocnyT come from the restatement itself.
import ctypes as ct

SN = rv.STRESS_NAMES
P_ = orc._p64


class _Merged(dict):
    files = property(lambda self: list(self))


def load_dyn(cfg, case=None):
    """the chain records of `case`, or (case None) the single-routine records of every variant"""
    g = os.path.join(HERE, "golden")
    if case is not None:
        return np.load(os.path.join(g, f"ref_dyn_{cfg}.{case}.npz"))
    out = _Merged()
    for var in rv.BLOCK_VARIANTS:
        with np.load(os.path.join(g, f"ref_dyn_{cfg}.{var}.npz")) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _between(a, lo, hi):
    return int(((a > lo) & (a < hi)).sum())


def assert_block_coverage(cfg, z):
    """the branches the single-routine records must reach, counted on the reference's outputs (and the inputs they belong to)"""
    big = cfg == "g72x20_b72x20"
    n10, n3 = (10, 3) if big else (2, 1)
    for var in rv.BLOCK_VARIANTS:
        q = rv.block_inputs(cfg, "full", var)
        ilo, ihi, jlo, jhi = rv.BLOCK_RECORDS[cfg]["full"]
        ph = np.zeros(q["aice"].shape, dtype=bool); ph[jlo - 1:jhi, ilo - 1:ihi] = True
        pre = f"full/{var}"
        tm, itm = z[f"{pre}/evp_prep1/tmass"], z[f"{pre}/evp_prep1/icetmask"]
        assert (q["tmask"][ph] == 0).sum() >= n10 and (tm[q["tmask"] == 0] == 0).all()
        assert (itm[ph] == 1).sum() >= n10 and (itm[ph] == 0).sum() >= n10
        assert _between(tm, rv.M_MIN * (1 - 1e-8), rv.M_MIN) >= n3 and _between(tm, rv.M_MIN, rv.M_MIN * (1 + 1e-8)) >= n3
        assert _between(q["aice"], rv.A_MIN * (1 - 1e-8), rv.A_MIN) >= n3 and _between(q["aice"], rv.A_MIN, rv.A_MIN * (1 + 1e-8)) >= n3
        new, old = z[f"{pre}/evp_prep2/iceumask"] != 0, q["iceumask"] != 0
        assert (new & ~old & ph).sum() >= n10 and (old & ~new & ph).sum() >= n10, (cfg, var)
        for a, t in ((q["aiu"], rv.A_MIN), (q["umass"], rv.M_MIN)):
            assert _between(a[ph], t * (1 - 1e-8), t) >= 1 and _between(a[ph], t, t * (1 + 1e-8)) >= 1
        assert (q["umask"][ph] == 0).sum() >= n3
        act = np.zeros(ph.shape, dtype=bool)
        act[q["indxt"][1, :q["icellt"]] - 1, q["indxt"][0, :q["icellt"]] - 1] = True
        prs = z[f"{pre}/stress/prs_sig"]
        assert (act & (q["strength"] == 0)).sum() >= n10
        assert (act & (q["strength"] > 0) & (prs == 0)).sum() >= n10 and (act & (prs > 0)).sum() >= n10, (cfg, var)
        s1 = z[f"{pre}/principal_stress/sig1"]
        assert (s1 == 1.0e30).sum() >= n10 and (s1 != 1.0e30).sum() >= n10
    v = rv.BLOCK_VARIANTS
    assert {(x["revised_evp"], x["tilt_from_slope"], x["ksub"] == x["ndte"]) for x in v.values()} == {(0, 0, False), (1, 1, True)}


def assert_chain_coverage(cfg, case, d, f, z):
    """the branches a chain record must reach, per case, on physical cells, from the reference's outputs"""
    nmin = 200 if cfg == "g72x20_b72x20" else 60
    ph = np.zeros(f["aice"].shape, dtype=bool)
    for n, b in enumerate(d.local_blocks):
        ph[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    ew, ns, land, var = rv.DYN_CASES[case]
    for ndte in rv.DYN_NDTE:
        pre = f"ndte{ndte}"
        itm, ium, tm = z[f"{pre}/icetmask"], z[f"{pre}/iceumask"] != 0, z[f"{pre}/tmass"]
        assert (itm[ph] == 1).sum() >= nmin and ium[ph].sum() >= nmin, (cfg, case, int((itm[ph] == 1).sum()), int(ium[ph].sum()))
        assert int(z[f"{pre}/icell"][:, 1].sum()) == ium[ph].sum()
        if land != "none":
            assert (f["tmask"][ph] == 0).sum() >= 6
        if land != "none" or ns != "tripole":
            assert (f["umask"][ph] == 0).sum() >= 6
        old = f["iceumask"] != 0
        assert (ium & ~old & ph).sum() >= 10 and (old & ~ium & ph).sum() >= 10
        assert _between(tm[ph], rv.M_MIN * (1 - 1e-8), rv.M_MIN) >= 1 and _between(tm[ph], rv.M_MIN, rv.M_MIN * (1 + 1e-8)) >= 1
        a = f["aice"][ph]
        assert _between(a, rv.A_MIN * (1 - 1e-8), rv.A_MIN) >= 1 and _between(a, rv.A_MIN, rv.A_MIN * (1 + 1e-8)) >= 1
        act = ph & (itm == 1)
        assert (act & (f["strength"] == 0)).sum() >= 10
        prs = z[f"{pre}/prs_sig"]
        assert (act & (prs > 0)).sum() >= 10
        if ndte == 1:            # the patch at rest: Delta == 0 exactly in the first subcycle
            assert (act & (f["strength"] > 0) & (prs == 0)).sum() >= 10, (cfg, case, int((act & (f["strength"] > 0) & (prs == 0)).sum()))
        assert np.abs(z[f"{pre}/uvel"][ph]).max() > 1e-3 and (z[f"{pre}/fm"][ph] > 0).any() and (z[f"{pre}/fm"][ph] < 0).any()
    flags = {k: {c[3][k] for c in rv.DYN_CASES.values()} for k in ("revised_evp", "tilt_from_slope", "wind_on_ugrid")}
    assert all(v == {0, 1} for v in flags.values()) and (rv.COSW, rv.SINW) != (1.0, 0.0)


def _sig(q):
    return [(orc.c_f64p * 4)(*[P_(q[f"{k}_{c}"]) for c in (1, 2, 3, 4)]) for k in ("stressp", "stressm", "stress12")]


def _same(got, want, where):
    assert got.dtype == want.dtype and np.array_equal(got, want), (where, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("cfg", list(rv.KERNEL_CONFIGS))
def test_dyn_single_routines_equal_reference(cfg):
    """orc_evp_prep1, orc_evp_prep2, orc_stress (ksub < ndte and ksub == ndte), orc_stepu, orc_evp_finish and
    orc_principal_stress == the reference's own routines, every output array, every cell, bit for bit; classic EVP with the
    geostrophic tilt and revised EVP with the tilt from the surface slope, a 25 degree turning angle; a full block and (on the
    padded configuration) a block whose physical domain is 2 x 3 cells."""
    z = load_dyn(cfg)
    assert_block_coverage(cfg, z)
    L = orc.lib()
    i32, f64, pp = orc.c_i32p, orc.c_f64p, ct.POINTER(orc.OrcParams)
    L.orc_evp_prep1.argtypes = [ct.c_int] * 6 + [f64] * 3 + [i32] + [f64] * 5 + [i32, pp]
    L.orc_evp_prep2.argtypes = ([ct.c_int] * 6 + [i32] * 6 + [f64] * 4 + [i32] + [f64] * 6 + [i32, i32, f64, ct.c_double] + [f64] * 10 +
                                [ct.POINTER(f64)] * 3 + [f64] * 4 + [pp])
    L.orc_stepu.argtypes = [ct.c_int] * 3 + [f64, i32, i32] + [f64] * 19 + [pp]
    L.orc_evp_finish.argtypes = [ct.c_int] * 3 + [f64, i32, i32] + [f64] * 10 + [pp]
    nxb, nyb = rv.KERNEL_CONFIGS[cfg][2] + 2, rv.KERNEL_CONFIGS[cfg][3] + 2
    n = 0
    for rec, (ilo, ihi, jlo, jhi) in rv.BLOCK_RECORDS[cfg].items():
        for var, v in rv.BLOCK_VARIANTS.items():
            p = rv.block_params(var)
            pre = f"{rec}/{var}"
            q = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in rv.block_inputs(cfg, rec, var).items()}
            o = {k: np.zeros((nyb, nxb)) for k in ("strairx", "strairy", "tmass")}
            itm = np.zeros((nyb, nxb), np.int32)
            L.orc_evp_prep1(nxb, nyb, ilo, ihi, jlo, jhi, P_(q["aice"]), P_(q["vice"]), P_(q["vsno"]), orc._p32(q["tmask"]), P_(q["strairxT"]),
                            P_(q["strairyT"]), P_(o["strairx"]), P_(o["strairy"]), P_(o["tmass"]), orc._p32(itm), ct.byref(p))
            for k in o:
                _same(o[k], z[f"{pre}/evp_prep1/{k}"], (pre, "evp_prep1", k))
            _same(itm, z[f"{pre}/evp_prep1/icetmask"], (pre, "evp_prep1", "icetmask"))

            q = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in rv.block_inputs(cfg, rec, var).items()}
            for k in ("umassdti", "waterx", "watery", "forcex", "forcey"):
                q[k] = np.full((nyb, nxb), 9.0)
            cnt = (ct.c_int32 * 2)()
            idx = np.zeros((4, nxb * nyb), np.int32)
            sp, sm, s12 = _sig(q)
            L.orc_evp_prep2(nxb, nyb, ilo, ihi, jlo, jhi, ct.cast(ct.byref(cnt, 0), i32), ct.cast(ct.byref(cnt, 4), i32),
                            orc._p32(idx[0]), orc._p32(idx[1]), orc._p32(idx[2]), orc._p32(idx[3]),
                            P_(q["aiu"]), P_(q["umass"]), P_(q["umassdti"]), P_(q["fcor"]), orc._p32(q["umask"]), P_(q["uocn"]), P_(q["vocn"]),
                            P_(q["strairx"]), P_(q["strairy"]), P_(q["ss_tltx"]), P_(q["ss_tlty"]), orc._p32(q["icetmask"]),
                            orc._p32(q["iceumask"]), P_(q["fm"]), rv.DYN_DT, P_(q["strtltx"]), P_(q["strtlty"]), P_(q["strocnx"]),
                            P_(q["strocny"]), P_(q["strintx"]), P_(q["strinty"]), P_(q["waterx"]), P_(q["watery"]), P_(q["forcex"]),
                            P_(q["forcey"]), sp, sm, s12, P_(q["uvel_init"]), P_(q["vvel_init"]), P_(q["uvel"]), P_(q["vvel"]), ct.byref(p))
            for k in [x for x in z.files if x.startswith(f"{pre}/evp_prep2/")]:
                name = k.rsplit("/", 1)[1]
                got = {"icell": np.array(list(cnt), np.int32), "indx": idx}.get(name, q.get(name))
                _same(got, z[k], (pre, "evp_prep2", name))
                n += 1

            q = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in rv.block_inputs(cfg, rec, var).items()}
            strv = orc.stress_block(nxb, nyb, v["ksub"], v["ndte"], np.ascontiguousarray(q["indxt"][0, :q["icellt"]]),
                                    np.ascontiguousarray(q["indxt"][1, :q["icellt"]]), q, p)
            for k in SN + ["shear", "divu", "prs_sig", "rdg_conv", "rdg_shear"]:
                _same(q[k], z[f"{pre}/stress/{k}"], (pre, "stress", k))
            _same(strv, z[f"{pre}/stress/str"], (pre, "stress", "str"))
            assert (z[f"{pre}/stress/divu"] != rv.block_inputs(cfg, rec, var)["divu"]).any() == (v["ksub"] == v["ndte"])

            q = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in rv.block_inputs(cfg, rec, var).items()}
            L.orc_stepu(nxb, nyb, q["icellu"], P_(q["Cw"]), orc._p32(q["indxu"][0]), orc._p32(q["indxu"][1]), P_(q["aiu"]), P_(q["str"]),
                        P_(q["uocn"]), P_(q["vocn"]), P_(q["waterx"]), P_(q["watery"]), P_(q["forcex"]), P_(q["forcey"]), P_(q["umassdti"]),
                        P_(q["fm"]), P_(q["uarear"]), P_(q["strocnx"]), P_(q["strocny"]), P_(q["strintx"]), P_(q["strinty"]),
                        P_(q["uvel_init"]), P_(q["vvel_init"]), P_(q["uvel"]), P_(q["vvel"]), ct.byref(p))
            for k in ("strocnx", "strocny", "strintx", "strinty", "uvel", "vvel"):
                _same(q[k], z[f"{pre}/stepu/{k}"], (pre, "stepu", k))

            q = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in rv.block_inputs(cfg, rec, var).items()}
            L.orc_evp_finish(nxb, nyb, q["icellu"], P_(q["Cw"]), orc._p32(q["indxu"][0]), orc._p32(q["indxu"][1]), P_(q["uvel"]), P_(q["vvel"]),
                             P_(q["uocn"]), P_(q["vocn"]), P_(q["aiu"]), P_(q["fm"]), P_(q["strocnx"]), P_(q["strocny"]), P_(q["strocnxT"]),
                             P_(q["strocnyT"]), ct.byref(p))
            for k in ("strocnx", "strocny", "strocnxT", "strocnyT"):
                _same(q[k], z[f"{pre}/evp_finish/{k}"], (pre, "evp_finish", k))

            s1, s2 = np.zeros((nyb, nxb)), np.zeros((nyb, nxb))
            L.orc_principal_stress(nxb, nyb, P_(q["stressp_1"]), P_(q["stressm_1"]), P_(q["stress12_1"]), P_(q["prs"]), P_(s1), P_(s2))
            _same(s1, z[f"{pre}/principal_stress/sig1"], (pre, "sig1")); _same(s2, z[f"{pre}/principal_stress/sig2"], (pre, "sig2"))
    assert n >= 30 * len(rv.BLOCK_RECORDS[cfg]) * 2


def chain_cells(d):
    from tests import util
    m = {k: util.cell_mask(d, k) for k in ("all", "ne", "phys")}
    kind = {n: "all" for n in util.ALL_CELLS}
    kind.update({n: "ne" for n in util.NE_CELLS})
    kind.update({n: "phys" for n in util.PHYS_CELLS})
    return m, kind


def chain_diff(d, got, z, pre):
    """fields of `got` that differ from the chain record `pre` of fixture z on the cells the reference defines (tests/util.py)"""
    m, kind = chain_cells(d)
    bad = []
    for k in z.files:
        if not k.startswith(pre + "/"):
            continue
        n = k.split("/", 1)[1]
        if n not in kind or n not in got:
            continue
        a, b = got[n][m[kind[n]]], z[k][m[kind[n]]]
        if not np.array_equal(a != 0 if n == "iceumask" else a, b != 0 if n == "iceumask" else b):
            bad.append((n, int((a != b).sum()), float(np.abs(a.astype(float) - b.astype(float)).max())))
    return bad


_chain_inputs = {}


def chain_inputs(cfg, case):
    """(decomp, fields) of a chain record, built once per session and never modified (callers clone)"""
    if (cfg, case) not in _chain_inputs:
        _chain_inputs[cfg, case] = rv.dyn_fields(cfg, case)
    return _chain_inputs[cfg, case]


@pytest.mark.parametrize("case", list(rv.DYN_CASES))
@pytest.mark.parametrize("cfg", list(rv.KERNEL_CONFIGS))
def test_evp_chain_equals_reference(cfg, case):
    """orc.evp == the reference's evp_prep1 -> icetmask halo -> evp_prep2 -> ndte x (stress -> stepu -> velocity halo) ->
    stress fold (tripole) -> evp_finish, run by the reference's own routines and halo updates on the whole grid, for
    ndte = 6, 5 and 1: every output on the cells the reference defines, bit for bit; then principal_stress and the cell counts.
    The T<->U averages inside (aiu, umass, wind stress, the last step of strocnxT / strocnyT) are the restatement's own on
    both sides: they remain unpinned."""
    from tests import util
    z = load_dyn(cfg, case)
    d, f = chain_inputs(cfg, case)
    assert_chain_coverage(cfg, case, d, f, z)
    ph = util.cell_mask(d, "phys")
    for ndte in rv.DYN_NDTE:
        pk, po = rv.dyn_params(cfg, case, ndte, f, d)
        fo = util.clone(f)
        nt, nu, _ = orc.evp(d, po, fo)
        pre = f"ndte{ndte}"
        assert len([k for k in z.files if k.startswith(pre + "/")]) >= 36
        bad = chain_diff(d, fo, z, pre)
        assert not bad, (cfg, case, ndte, bad)
        assert nu == int(z[f"{pre}/icell"][:, 1].sum()) and nt == int((z[f"{pre}/icetmask"][ph] == 1).sum())
        s1, s2 = np.zeros_like(fo["uvel"]), np.zeros_like(fo["uvel"])
        for n in range(d.nblocks):
            orc.lib().orc_principal_stress(d.nx_block, d.ny_block, P_(fo["stressp_1"][n]), P_(fo["stressm_1"][n]), P_(fo["stress12_1"][n]),
                                           P_(fo["prs_sig"][n]), P_(s1[n]), P_(s2[n]))
        assert np.array_equal(s1[ph], z[f"{pre}/sig1"][ph]) and np.array_equal(s2[ph], z[f"{pre}/sig2"][ph])


# ---------------------------------------------------------------------------------------------------------------------
# horizontal_remap: the reference's own make_masks / construct_fields / limited_gradient / departure_points /
# locate_triangles / triangle_coordinates / transport_integrals / update_fields (tests/golden/ref_remap_*.npz; slice and driver:
# oracle/ref/Makefile, oracle/ref/ref_remap.F90; inputs: refvec.remap_fields / remap_block_inputs)
def load_remap(cfg, case):
    return np.load(os.path.join(HERE, "golden", f"ref_remap_{cfg}.{case}.npz"))


def assert_remap_coverage(cfg, per_case=None, stops=None):
    """the branches of locate_triangles the chain fixtures of one config enter, counted by the generator over the REFERENCE'S
    compressed triangle lists: every signature of refvec.remap_signatures and every branch of refvec.REMAP_PATTERNS on both
    edge kinds, no signature outside the list, the six (order, rule) pairs, and the two stop cases"""
    if per_case is None:
        per_case = {case: load_remap(cfg, case) for case in rv.REMAP_CASES}
        stops = load_remap(cfg, "stops")
    sig, pat, combos = {}, {}, set()
    for case, z in per_case.items():
        for order, midpt in rv.REMAP_CASES[case][2]:
            pre = f"o{order}m{midpt}"
            assert z[f"{pre}/stop"][0] == 0, (cfg, case, pre, "the reference stopped: lower refvec.REMAP_COURANT")
            combos.add((order, midpt))
            for e, g, di, dj, s, n in z[f"{pre}/sig"]:
                sig[(e, g, di, dj, s)] = sig.get((e, g, di, dj, s), 0) + n
            for e, p, n in z[f"{pre}/pat"]:
                pat[(e, p)] = pat.get((e, p), 0) + n
    assert combos == {(o, m) for o in (1, 2, 3) for m in (0, 1)}
    names = list(rv.REMAP_PATTERNS)
    for e in (0, 1):
        want = rv.remap_signatures(e == 1)
        got = {k[1:] for k in sig if k[0] == e}
        assert want <= got, (cfg, "edge kind", e, "signatures never produced:", sorted(want - got))
        assert got <= want, (cfg, "edge kind", e, "signatures outside the derived list:", sorted(got - want))
        missing = [names[p] for p in range(len(names)) if pat.get((e, p), 0) == 0]
        assert not missing, (cfg, "edge kind", e, "branches never entered:", missing)
    for name, (rc, _, _) in rv.REMAP_STOPS.items():
        assert stops[name][0] == rc, (name, stops[name])
    return sig, pat


@pytest.mark.parametrize("cfg", list(rv.KERNEL_CONFIGS))
def test_remap_fixtures_cover_the_triangle_branches(cfg):
    sig, pat = assert_remap_coverage(cfg)
    assert min(sig.values()) >= 1 and min(pat.values()) >= 1


def remap_phys(d, a):
    """the physical cells of a (nblocks, ..., ny, nx) array, and the rest"""
    m = np.zeros((d.nblocks,) + (1,) * (a.ndim - 3) + (d.ny_block, d.nx_block), dtype=bool)
    for n, b in enumerate(d.local_blocks):
        m[n, ..., b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    return np.broadcast_to(m, a.shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def remap_diff(d, case, pre, got_m, got_t, mm, tm, z):
    """differences from a chain record: physical cells bit for bit (signed zeros included), ghost cells as they were"""
    bad = []
    for name, got, inp, want in (("mm", got_m, mm, z[f"{pre}/mm"]), ("tm", got_t, tm, z[f"{pre}/tm"])):
        ph = remap_phys(d, got)
        if not np.array_equal(_bits(got)[ph], _bits(want)[ph]):
            k = np.argwhere((_bits(got) != _bits(want)) & ph)
            bad.append((case, pre, name, len(k), [(tuple(int(v) for v in q), float(got[tuple(q)]), float(want[tuple(q)])) for q in k[:3]]))
        if not np.array_equal(_bits(got)[~ph], _bits(inp)[~ph]):
            bad.append((case, pre, name, "ghost cells written", int((_bits(got) != _bits(inp))[~ph].sum())))
    return bad


@pytest.mark.parametrize("case", list(rv.REMAP_CASES))
@pytest.mark.parametrize("cfg", list(rv.KERNEL_CONFIGS))
def test_horizontal_remap_equals_reference_chain(cfg, case):
    """orc_horizontal_remap == the reference's own routines run in horizontal_remap's order with its own halo updates, on every
    physical cell of mm and tm, bit for bit: rough velocities whose sign changes from corner to corner (every triangle branch,
    see assert_remap_coverage), corners at rest, masses around puny, tracers with dependents around puny, 1 and 16 padded
    blocks, cyclic / open / closed / tripole boundaries, land, six tracers of the three types and none"""
    z = load_remap(cfg, case)
    d, f, mm, tm, tables = rv.remap_fields(cfg, case)
    bad = []
    for order, midpt in rv.REMAP_CASES[case][2]:
        mo, to = mm.copy(), tm.copy()
        assert orc.horizontal_remap(d, rv.REMAP_DT, f, mo, to, *tables, integral_order=order, l_dp_midpt=bool(midpt)) == 0
        assert np.abs(mo - mm).max() > 1e-3
        bad += remap_diff(d, case, f"o{order}m{midpt}", mo, to, mm, tm, z)
    assert not bad, bad[:4]


@pytest.mark.parametrize("cfg", list(rv.KERNEL_CONFIGS))
def test_horizontal_remap_stop_cases_equal_reference(cfg):
    """the reference's two l_stop cases: 1 where departure_points stops, 2 where update_fields meets a negative mass"""
    z = load_remap(cfg, "stops")
    for name, (rc, order, midpt) in rv.REMAP_STOPS.items():
        assert z[name][0] == rc
        d, f, mm, tm, tables = rv.remap_fields(cfg, "cyclic_open", stop=name)
        assert orc.horizontal_remap(d, rv.REMAP_DT, f, mm.copy(), tm.copy(), *tables, integral_order=order, l_dp_midpt=bool(midpt)) == rc, name


def _same_bits(got, want, where):
    """equal bit for bit: -0.0 and +0.0 differ"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, want.dtype, got.shape, want.shape)
    ne = got.view(np.int64) != want.view(np.int64) if got.dtype == np.float64 else got != want
    assert not ne.any(), (where, int(ne.sum()), [(k, float(got[tuple(k)]), float(want[tuple(k)])) for k in np.argwhere(ne)[:4].tolist()])


def load_remap_blk(var):
    return np.load(os.path.join(HERE, "golden", f"ref_remap_blk.{var}.npz"))


def _listed(z, pre, e):
    """(group, j, i) index arrays of the reference's compressed triangle lists: the only entries of xp, yp, iflux, jflux its
    arrays define"""
    ic, ii, jj = z[f"{pre}/locate_triangles/{e}/icells"], z[f"{pre}/locate_triangles/{e}/indxi"], z[f"{pre}/locate_triangles/{e}/indxj"]
    g = np.concatenate([np.full(ic[k], k) for k in range(6)])
    i = np.concatenate([ii[k, :ic[k]] for k in range(6)]) - 1
    j = np.concatenate([jj[k, :ic[k]] for k in range(6)]) - 1
    return g, j, i


@pytest.mark.parametrize("var", list(rv.REMAP_BLOCK_VARIANTS))
def test_remap_single_routines_equal_reference(var):
    """each of the eight routines of ice_transport_remap ALONE: the C restatement's routine on the reference's recorded input of
    that routine (what the routine before it returned) == the reference's recorded output, bit for bit with signed zeros.
    Blocks: a full 8 x 5 block and a padded 2 x 3 one; variants: six tracers of types 1 1 1 2 2 3 with integral orders 3, 2, 1
    and both departure-point rules, a table with one tracer with dependents, no tracers, and the departure-point stop.
    Compared where the Fortran defines its arrays: triangle vertices, iflux / jflux through the compressed lists; the open-
    water mc on physical cells (the reference lists open water over the whole block, make_masks :930-943, so its
    construct_fields also sets mc = mm in ghost cells, which horizontal_remap's halo update overwrites: a difference of
    interface, asserted here)."""
    L, z = orc.lib(), load_remap_blk(var)
    cfg = rv.REMAP_BLOCK_CFG
    nx, ny = rv.KERNEL_CONFIGS[cfg][2] + 2, rv.KERNEL_CONFIGS[cfg][3] + 2
    ncat, P32 = rv.REMAP_NCAT, orc._p32
    c = np.ascontiguousarray
    checked = 0
    for rec, (ilo, ihi, jlo, jhi) in rv.BLOCK_RECORDS[cfg].items():
        pre = f"{rec}/{var}"
        mm, tm, q, (ttype, depend, has), order, midpt = rv.remap_block_inputs(rec, var)
        nt = len(ttype)
        ttype, depend, has = c(ttype, dtype=np.int32), c(depend, dtype=np.int32), c(has, dtype=np.int32)
        box = (nx, ny, ilo, ihi, jlo, jhi)
        phys = np.zeros((ny, nx), dtype=bool); phys[jlo - 1:jhi, ilo - 1:ihi] = True
        eq = lambda got, key: _same_bits(got, z[f"{pre}/{key}"], (pre, key))
        N = lambda a: (P32(a) if a.dtype == np.int32 else P_(a)) if a.size else None
        # make_masks
        mmask, tmask, icells = np.zeros_like(mm), np.zeros_like(tm), np.zeros(ncat + 1, dtype=np.int32)
        for n in range(ncat + 1):
            L.orc_remap_make_masks(*box, int(n == 0), nt, P32(has) if nt else None, P_(c(mm[n])), P_(mmask[n]), N(tm[n - 1]) if n else None,
                                   N(tmask[n - 1]) if n else None, P32(icells[n:n + 1]))
        eq(mmask, "make_masks/mmask"); eq(tmask, "make_masks/tmask")
        assert np.array_equal(icells, z[f"{pre}/make_masks/icells"]), (pre, icells, z[f"{pre}/make_masks/icells"])
        rm, rt = z[f"{pre}/make_masks/mmask"], z[f"{pre}/make_masks/tmask"]
        # limited_gradient
        gx, gy = np.zeros((ny, nx)), np.zeros((ny, nx))
        L.orc_remap_limited_gradient(*box, P_(q["phi"]), P_(c(rm[1])), P_(q["cnx"]), P_(q["cny"]), P_(gx), P_(gy))
        eq(gx, "limited_gradient/gx"); eq(gy, "limited_gradient/gy")
        live = int((rm[1][phys] > 0).sum())                         # phi is a ramp under noise: few of the unmasked cells are extrema
        assert rec == "pad" or (live >= 10 and min(np.count_nonzero(gx), np.count_nonzero(gy)) >= live // 2), (live, np.count_nonzero(gx))
        # construct_fields
        mc, mx, my = np.zeros_like(mm), np.zeros_like(mm), np.zeros_like(mm)
        tc, tx, ty = np.zeros_like(tm), np.zeros_like(tm), np.zeros_like(tm)
        for n in range(ncat + 1):
            wt = n > 0
            L.orc_remap_construct_fields(*box, nt, N(ttype), N(depend), N(has), P_(q["hm"]), P_(c(mm[n])), P_(mc[n]), P_(mx[n]), P_(my[n]),
                                         P_(c(rm[n])), P_(c(tm[n - 1])) if wt else None, P_(tc[n - 1]) if wt else None,
                                         P_(tx[n - 1]) if wt else None, P_(ty[n - 1]) if wt else None, P_(c(rt[n - 1])) if wt else None)
        want0 = z[f"{pre}/construct_fields/mc"][0]
        _same_bits(mc[1:], z[f"{pre}/construct_fields/mc"][1:], (pre, "mc")); _same_bits(mc[0][phys], want0[phys], (pre, "mc open water"))
        assert np.array_equal(want0[~phys], np.where(mm[0] > 1e-11, mm[0], 0.0)[~phys]) and not mc[0][~phys].any()
        for k, a in (("mx", mx), ("my", my), ("tc", tc), ("tx", tx), ("ty", ty)):
            eq(a, f"construct_fields/{k}")
        rmc, rmx, rmy = (z[f"{pre}/construct_fields/{k}"] for k in ("mc", "mx", "my"))
        rtc, rtx, rty = (z[f"{pre}/construct_fields/{k}"] for k in ("tc", "tx", "ty"))
        # departure_points
        dpx, dpy, ij = np.zeros((ny, nx)), np.zeros((ny, nx)), np.zeros(2, dtype=np.int32)
        stop = L.orc_remap_departure_points(*box, rv.REMAP_DT, *(P_(q[k]) for k in ("uvel", "vvel", "dxu", "dyu", "HTN", "HTE")), P_(dpx), P_(dpy),
                                            midpt, P32(ij))
        assert (stop, ij[0], ij[1]) == tuple(z[f"{pre}/departure_points/stop"]), (pre, stop, ij, z[f"{pre}/departure_points/stop"])
        eq(dpx, "departure_points/dpx"); eq(dpy, "departure_points/dpy")
        checked += 1
        if stop:
            assert var == "t6_stop"
            continue
        rdx, rdy = c(z[f"{pre}/departure_points/dpx"]), c(z[f"{pre}/departure_points/dpy"])
        flx = {}
        for e, north in (("east", 0), ("north", 1)):
            # locate_triangles
            xp, yp = np.zeros((6, 4, ny, nx)), np.zeros((6, 4, ny, nx))
            ifl, jfl, tri = np.zeros((6, ny, nx), dtype=np.int32), np.zeros((6, ny, nx), dtype=np.int32), np.zeros((6, ny, nx))
            L.orc_remap_locate_triangles(*box, north, P_(rdx), P_(rdy), P_(q["dxu"]), P_(q["dyu"]), P_(xp), P_(yp), P32(ifl), P32(jfl), P_(tri))
            g, j, i = _listed(z, pre, e)
            assert len(g) > (4 if rec == "pad" else 40)
            eq(tri, f"locate_triangles/{e}/triarea")                 # zero wherever no triangle is listed, on both sides
            assert np.array_equal(np.argwhere(tri != 0), np.array(sorted(zip(g, j, i))).reshape(-1, 3))
            for k, a in (("iflux", ifl), ("jflux", jfl)):
                assert np.array_equal(a[g, j, i], z[f"{pre}/locate_triangles/{e}/{k}"][g, j, i]), (pre, e, k)
            for k, a in (("xp", xp), ("yp", yp)):
                _same_bits(a[g, 1:, j, i], z[f"{pre}/locate_triangles/{e}/{k}"][g, 1:, j, i], (pre, e, k))
            # triangle_coordinates, on the reference's vertices
            rtri = c(z[f"{pre}/locate_triangles/{e}/triarea"])
            xq, yq = c(z[f"{pre}/locate_triangles/{e}/xp"]), c(z[f"{pre}/locate_triangles/{e}/yp"])
            L.orc_remap_triangle_coordinates(nx, ny, order, P_(rtri), P_(xq), P_(yq))
            for k, a in (("xp", xq), ("yp", yq)):
                _same_bits(a[g, :, j, i], z[f"{pre}/triangle_coordinates/{e}/{k}"][g, :, j, i], (pre, e, k, "coordinates"))
            # transport_integrals, on the reference's triangles and fields
            rxp, ryp = c(z[f"{pre}/triangle_coordinates/{e}/xp"]), c(z[f"{pre}/triangle_coordinates/{e}/yp"])
            rif, rjf = c(z[f"{pre}/locate_triangles/{e}/iflux"]), c(z[f"{pre}/locate_triangles/{e}/jflux"])
            mflx, mtflx = np.zeros_like(mm), np.zeros_like(tm)
            for n in range(ncat + 1):
                wt = n > 0
                L.orc_remap_transport_integrals(nx, ny, nt, N(ttype), N(depend), order, P_(rtri), P32(rif), P32(rjf), P_(rxp), P_(ryp),
                                                P_(c(rmc[n])), P_(c(rmx[n])), P_(c(rmy[n])), P_(mflx[n]),
                                                P_(c(rtc[n - 1])) if wt else None, P_(c(rtx[n - 1])) if wt else None,
                                                P_(c(rty[n - 1])) if wt else None, P_(mtflx[n - 1]) if wt else None)
            eq(mflx, f"transport_integrals/{e}/mflx"); eq(mtflx, f"transport_integrals/{e}/mtflx")
            assert rec == "pad" or np.count_nonzero(mflx) > 40
            flx[e] = (z[f"{pre}/transport_integrals/{e}/mflx"], z[f"{pre}/transport_integrals/{e}/mtflx"])
        # update_fields, on the reference's fluxes
        um, ut, stops = mm.copy(), tm.copy(), np.zeros((ncat + 1, 3), dtype=np.int32)
        for n in range(ncat + 1):
            wt = n > 0
            stops[n, 0] = L.orc_remap_update_fields(*box, nt, N(ttype), N(depend), P_(q["tarear"]), P_(c(flx["east"][0][n])), P_(c(flx["north"][0][n])),
                                                    P_(um[n]), P_(c(flx["east"][1][n - 1])) if wt else None,
                                                    P_(c(flx["north"][1][n - 1])) if wt else None, P_(ut[n - 1]) if wt else None, P32(stops[n, 1:]))
        assert np.array_equal(stops, z[f"{pre}/update_fields/stop"]), (pre, stops, z[f"{pre}/update_fields/stop"])
        eq(um, "update_fields/mm"); eq(ut, "update_fields/tm")
    assert checked == 2
