"""Deterministic test inputs shared by tests/golden/make_ref_golden.py (which feeds them to the reference build,
oracle/_ref) and by the tests (which feed the same bytes to the C restatement and to the HIP path).  Only the OUTPUTS of
the reference are stored in tests/golden/ref_*.npz; the inputs are regenerated from (seed, shape) by the integer hash
below, which does not depend on any library's random stream.
"""
from __future__ import annotations

import numpy as np

# the builds of oracle/ref/Makefile the fixtures come from: name -> (NX, NY, BX, BY, MXB)
CONFIGS = {
    "g24x16_b24x16": (24, 16, 24, 16, 1),       # one block
    "g24x16_b6x4": (24, 16, 6, 4, 16),          # 4 x 4 blocks
    "g26x18_b8x5": (26, 18, 8, 5, 16),          # 4 x 4 blocks, the last ones padded in x and in y
}
NCAT = 5
MAX_NTRCR = 20              # ice_domain_size.F90:38-52 with the defines of oracle/ref/Makefile

# (ew_boundary_type, ns_boundary_type, land pattern)
BOUNDARIES = [
    ("cyclic", "open", "none"), ("cyclic", "closed", "rim"), ("cyclic", "tripole", "none"),
    ("open", "open", "none"), ("open", "closed", "rim"),
    ("closed", "open", "rim"), ("closed", "closed", "rim"),
    # (tripole grids are cyclic E-W: with 'open' / 'closed' the reference's copy out of the tripole buffer follows mirrored
    #  ghost indices resp. reads column nx_global + 1 of the buffer, serial/ice_boundary.F90:3752-3776, :3420-3424)
    ("cyclic", "open", "landblock"), ("cyclic", "tripole", "landblock"),
]

LOC = {"center": 1, "necorner": 2, "nface": 3, "eface": 4}           # ice_constants.F90 field_loc_*
TYPE = {"scalar": 1, "vector": 2, "angle": 3}                        # field_type_*

# the halo updates every case runs: (key, nz, loc, type, fill or None)
HALO_R8 = [(f"{l}_{t}", 0, LOC[l], TYPE[t], None) for l in LOC for t in ("scalar", "vector")] + [
    ("center_angle", 0, LOC["center"], TYPE["angle"], None),
    ("center_scalar_fill", 0, LOC["center"], TYPE["scalar"], -9.5),
    ("necorner_vector_fill", 0, LOC["necorner"], TYPE["vector"], 3.25),
    ("center_scalar_3d", 3, LOC["center"], TYPE["scalar"], None),
    ("necorner_vector_3d", 2, LOC["necorner"], TYPE["vector"], None),
]
HALO_I4 = [("center_scalar", LOC["center"], TYPE["scalar"], None), ("center_scalar_fill", LOC["center"], TYPE["scalar"], 7)]


def case_name(ew, ns, land):
    return f"{ew}_{ns}" + ("" if land in ("none", "rim") else f"_{land}")


def _splitmix(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash01(shape, seed: int) -> np.ndarray:
    """float64 in [0, 1) with full 53-bit mantissas, a pure function of (seed, flat index)"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        k = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x100000001B3)
        h = _splitmix(_splitmix(k))
    return ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(shape)


def seed_of(*parts) -> int:
    s = 1469598103934665603
    for p in parts:
        for ch in str(p):
            s = ((s ^ ord(ch)) * 1099511628211) % (1 << 63)
    return s % (1 << 40)


def halo_r8_input(cfg, case, key, nblocks, ny_block, nx_block, nz):
    """every cell, ghost cells included, gets its own value in (-1, 1): a ghost cell the update leaves alone is then visible"""
    shape = (nblocks, nz, ny_block, nx_block) if nz else (nblocks, ny_block, nx_block)
    return np.ascontiguousarray(2.0 * hash01(shape, seed_of(cfg, case, "r8", key)) - 1.0)


def halo_i4_input(cfg, case, key, nblocks, ny_block, nx_block):
    n = nblocks * ny_block * nx_block          # every cell its own value (a cell the update leaves alone stays recognisable)
    return np.ascontiguousarray((hash01((nblocks, ny_block, nx_block), seed_of(cfg, case, "i4", key)) * 5).astype(np.int32) - 1
                                + 10 * np.arange(1, n + 1, dtype=np.int32).reshape(nblocks, ny_block, nx_block))


def kmt_ulat(nx, ny, bx, by, ew, ns, land):
    """KMTG (1 ocean / 0 land) and ULATG (radians) handed to init_domain_distribution (ice_domain.F90:248)"""
    kmt = np.ones((ny, nx))
    if land in ("rim",):
        if ns == "closed":
            kmt[:2, :] = 0; kmt[-2:, :] = 0
        if ew == "closed":
            kmt[:, :2] = 0; kmt[:, -2:] = 0
    if land == "landblock":          # block (iblock, jblock) = (2, 2) is all land: eliminated from the distribution
        kmt[by:2 * by, bx:2 * bx] = 0
    if land == "patch":              # a small interior island inside the ice (no block is all land)
        c0, w = (2, 3) if nx < 40 else (7, 4)
        kmt[ny // 2 - 1:ny // 2 + 2, c0:c0 + w] = 0
    ulat = np.deg2rad(np.linspace(-80.0, 88.0, ny))[:, None] + np.zeros((1, nx))
    return kmt, ulat


def state_input(cfg, case, nblocks, ny_block, nx_block, ntrcr):
    """aicen, vicen, vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, MAX_NTRCR, ny, nx) for bound_state: every cell its own value"""
    s = lambda k, shape: np.ascontiguousarray(hash01(shape, seed_of(cfg, case, "state", k)))
    a = s("aicen", (nblocks, NCAT, ny_block, nx_block)) * 0.2
    a[a < 0.05] = 0.0                                                  # categories without ice
    v = s("vicen", (nblocks, NCAT, ny_block, nx_block)) * 2.0
    sn = s("vsnon", (nblocks, NCAT, ny_block, nx_block)) * 0.3
    t = s("trcrn", (nblocks, NCAT, MAX_NTRCR, ny_block, nx_block)) * 4.0 - 2.0
    return a, v, sn, t


def strength_input(cfg, tag, ny_block, nx_block):
    """a thickness distribution per cell that exercises ice_strength's branches: open-water fractions on both sides of
    Gstar = 0.15, empty categories, thin and thick ice; plus the list of cells it is evaluated on"""
    h = lambda k, shape: hash01(shape, seed_of(cfg, "strength", tag, k))
    hin = np.array([0.0, 0.64, 1.39, 2.47, 4.57, 9.0])
    aicen = h("a", (NCAT, ny_block, nx_block))
    aicen[h("hole", (NCAT, ny_block, nx_block)) < 0.25] = 0.0
    tot = aicen.sum(axis=0)
    target = h("tot", (ny_block, nx_block)) ** 0.3                      # mostly compact ice, some open cells
    target[h("full", (ny_block, nx_block)) < 0.15] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        aicen = np.where(tot > 0, aicen * (target / tot), 0.0)
    frac = h("hh", (NCAT, ny_block, nx_block))
    hi = hin[:-1, None, None] + frac * (hin[1:, None, None] - hin[:-1, None, None])
    vicen = aicen * hi
    aicen[aicen < 1e-11] = 0.0                                          # at or below puny: both branches of `aicen > puny`
    tiny = h("tiny", (NCAT, ny_block, nx_block)) < 0.03
    aicen[tiny] = 0.5e-11
    aice = aicen.sum(axis=0)
    vice = vicen.sum(axis=0)
    aice0 = np.maximum(1.0 - aice, 0.0)
    sel = (h("sel", (ny_block, nx_block)) < 0.9) & (aice > 1e-3)
    sel[0, :] = sel[-1, :] = False; sel[:, 0] = sel[:, -1] = False       # icetmask lives on physical cells
    jj, ii = np.nonzero(sel)                                            # j outer, i inner: the order of the reference's list
    c = np.ascontiguousarray
    return dict(aice=c(aice), vice=c(vice), aice0=c(aice0), aicen=c(aicen), vicen=c(vicen),
                indxi=(ii + 1).astype(np.int32), indxj=(jj + 1).astype(np.int32))


STRENGTH_CASES = [(1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)]       # (kstrength, krdg_partic, krdg_redist)
MU_RDG, CF = 3.0, 17.0                                                          # ice_init.F90:273-277 defaults
DISTRIBUTIONS = [(2, "slenderX1"), (4, "slenderX1"), (3, "slenderX1"), (4, "slenderX2"), (8, "slenderX2")]


# compute_tracers (ice_itd.F90:1359): tracer tables (trcr_depend, nt_Tsfc, nt_alvl, nt_apnd, nt_fbri, (cesm, lvl, topo))
# Tsfc, qice, qsno, alvl, vlvl, apnd (on alvl), hpnd (on apnd), fbri, a brine tracer (on fbri)
TRACER_CASES = {
    "lvl_ponds": ([0, 1, 2, 0, 1, 2 + 4, 2 + 6, 1, 2 + 8], 1, 4, 6, 8, (0, 1, 0)),
    "cesm_ponds": ([0, 1, 2, 0, 1, 0, 2 + 6, 1, 2 + 8], 1, 4, 6, 8, (1, 0, 0)),
    "plain": ([0, 1, 1, 2, 0], 1, 0, 0, 0, (0, 0, 0)),
}
TOCNFRZ = -1.8


def tracers_input(cfg, tag, ny_block, nx_block, ntrcr):
    h = lambda k, shape: hash01(shape, seed_of(cfg, "tracers", tag, k))
    a = h("a", (ny_block, nx_block)); a[a < 0.3] = 0.0; a[(a > 0.3) & (a < 0.35)] = 0.5e-11
    v = h("v", (ny_block, nx_block)) * 2.0; v[h("v0", (ny_block, nx_block)) < 0.25] = 0.0
    sn = h("s", (ny_block, nx_block)) * 0.4; sn[h("s0", (ny_block, nx_block)) < 0.3] = 0.0
    atr = h("atr", (ntrcr, ny_block, nx_block)) * 2.0 - 0.7
    atr[3] = np.abs(atr[3]) if ntrcr > 3 else 0        # (alvl, apnd, fbri products: positive where there is ice)
    if ntrcr > 7:
        atr[5] = np.abs(atr[5]); atr[7] = np.abs(atr[7])
        atr[5][h("p0", (ny_block, nx_block)) < 0.2] = 0.0
    c = np.ascontiguousarray
    return c(a), c(v), c(sn), c(atr)


# ---------------------------------------------------------------------------------------------------------------------
# the SLICE fixtures (oracle/ref/ref_kernels.F90, tests/golden/make_ref_kernels.py -> ref_dyn_*.npz): the reference's own
# evp_prep1 / evp_prep2 / stress / stepu / evp_finish / principal_stress.  A table of its own: the tests over CONFIGS expect a
# ref_<cfg>.npz per entry.
KERNEL_CONFIGS = {
    "g72x20_b72x20": (72, 20, 72, 20, 1),       # one block, wider than the 64-column tile / wave, five 4-row tiles tall
    "g26x18_b8x5": (26, 18, 8, 5, 16),          # 4 x 4 blocks, padded in x and y
}
# case -> (ew, ns, land, parameter variant); every flag takes both values over the cases
DYN_CASES = {
    "cyclic_open": ("cyclic", "open", "none", dict(revised_evp=0, tilt_from_slope=0, wind_on_ugrid=0)),
    "cyclic_tripole": ("cyclic", "tripole", "none", dict(revised_evp=1, tilt_from_slope=1, wind_on_ugrid=1)),
    "open_closed_rim": ("open", "closed", "rim", dict(revised_evp=0, tilt_from_slope=1, wind_on_ugrid=0)),
    "cyclic_open_patch": ("cyclic", "open", "patch", dict(revised_evp=1, tilt_from_slope=0, wind_on_ugrid=1)),
}
DYN_NDTE = (6, 5, 1)            # three pair launches / pairs + a single launch / one subcycle
DYN_DT = 3600.0
COSW, SINW = 0.9063077870366499, 0.42261826174069944      # a 25 degree turning angle, as literals (no libm in the inputs)
A_MIN, M_MIN, RHOI, RHOS, PSTAR = 0.001, 0.01, 917.0, 330.0, 2.75e4
STRESS_NAMES = [f"{k}_{c}" for k in ("stressp", "stressm", "stress12") for c in (1, 2, 3, 4)]


def dyn_decomp(cfg, case):
    from cice5_amd import blocks
    nx, ny, bx, by, _ = KERNEL_CONFIGS[cfg]
    ew, ns, _, _ = DYN_CASES[case]
    return blocks.create_distrb_cart(nx, ny, bx, by, ew_boundary_type=ew, ns_boundary_type=ns)


def zero_patch(nx):
    """(first column, first row), 1-based, of the 5 x 5 U cells at rest over still water: Delta == 0 exactly on the 4 x 4 T
    cells between them in the first subcycle"""
    return (1 if nx < 40 else 60), 3


def dyn_fields(cfg, case):
    """(decomp, fields): every array evp(dt) reads, in block layout, for a chain record.  Grid metrics: the analytic grid
    of cice5_amd.synth; masks from kmt_ulat; state and forcing from the hash.  Ice in a band of columns across the E-W seam
    (44 % of the grid) with open-water holes, cells at the a_min / m_min thresholds, cells without strength, a warm start
    (random old iceumask, velocities and stresses), a patch at rest.  Ghost cells: halo updates of the (pinned) restatement."""
    from cice5_amd import constants as C, synth
    from oracle import orc
    nx, ny, bx, by, _ = KERNEL_CONFIGS[cfg]
    ew, ns, land, _ = DYN_CASES[case]
    d = dyn_decomp(cfg, case)
    sc = synth.SynthCase(nx=nx, ny=ny, ew_boundary=C.BND_NAMES[ew], ns_boundary=C.BND_NAMES[ns], land="none")
    f = synth.make_block_fields(sc, d)
    kmt, _ = kmt_ulat(nx, ny, bx, by, ew, ns, land)
    h = lambda k: hash01((ny, nx), seed_of(cfg, case, "dyn", k))

    def scatter(G, loc, kind):
        a = np.zeros((d.nblocks, d.ny_block, d.nx_block))
        for n, b in enumerate(d.local_blocks):
            ni, nj = b.ihi - b.ilo + 1, b.jhi - b.jlo + 1
            a[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = G[b.jglob_lo - 1:b.jglob_lo - 1 + nj, b.iglob_lo - 1:b.iglob_lo - 1 + ni]
        orc.halo_r8(d, a, loc, kind, 0.0)
        return a
    T = lambda G: scatter(G, C.LOC_CENTER, C.KIND_SCALAR)
    hm = T(kmt)
    f["tmask"] = (hm > 0.5).astype(np.int32)
    um = np.zeros_like(hm)
    um[:, :-1, :-1] = np.minimum(np.minimum(hm[:, :-1, :-1], hm[:, :-1, 1:]), np.minimum(hm[:, 1:, :-1], hm[:, 1:, 1:]))
    phys = np.zeros(hm.shape, dtype=bool)
    for n, b in enumerate(d.local_blocks):
        phys[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    um[~phys] = 0.0
    orc.halo_r8(d, um, C.LOC_NECORNER, C.KIND_SCALAR, 0.0)
    f["umask"] = (um > 0.5).astype(np.int32)

    jj, ii = np.meshgrid(np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    pc, pr = zero_patch(nx)
    patchU = (ii >= pc) & (ii < pc + 5) & (jj >= pr) & (jj < pr + 5)
    patchT = (ii >= pc) & (ii <= pc + 5) & (jj >= pr) & (jj <= pr + 5)
    band = ((ii - 1 + int(0.22 * nx)) % nx) < int(0.44 * nx)
    hole = ((ii // 5 + jj // 3) % 4 == 0) & ~patchT
    icy = band & ~hole & (kmt > 0)
    thr = h("thr")
    aice = np.where(icy, 0.3 + 0.7 * h("aice"), 0.0)
    aice[icy & (thr < 0.04)] = A_MIN * (1 - 1e-9)
    aice[icy & (thr >= 0.04) & (thr < 0.08)] = A_MIN * (1 + 1e-9)
    vice = aice * (0.5 + 2.5 * h("hi"))
    vsno = aice * 0.3 * h("hs")
    for lo, eps in ((0.08, -1e-9), (0.12, 1e-9)):
        m = icy & (thr >= lo) & (thr < lo + 0.04)
        vice[m] = M_MIN * (1 + eps) / RHOI
        vsno[m] = 0.0
    strength = PSTAR * vice * (0.5 + h("str"))
    strength[h("str0") < 0.08] = 0.0
    f["aice"], f["vice"], f["vsno"] = T(aice), T(vice), T(vsno)
    f["aice_init"] = T(aice * (0.95 + 0.05 * h("ainit")))
    f["strength"] = T(strength)
    f["strairxT"] = T(aice * 0.2 * (h("wx") - 0.5)); f["strairyT"] = T(aice * 0.2 * (h("wy") - 0.5))
    U = lambda G: scatter(G, C.LOC_NECORNER, C.KIND_VECTOR) * f["umask"]
    still = np.where(patchU, 0.0, 1.0)
    f["strax"] = U(0.2 * (h("sx") - 0.5)); f["stray"] = U(0.2 * (h("sy") - 0.5))
    f["uocn"] = U(0.1 * (h("uo") - 0.5) * still); f["vocn"] = U(0.1 * (h("vo") - 0.5) * still)
    f["ss_tltx"] = U(1e-6 * (h("tx") - 0.5)); f["ss_tlty"] = U(1e-6 * (h("ty") - 0.5))
    f["Cdn_ocn"] = scatter(C.dragio * (0.7 + 0.6 * h("cw")), C.LOC_NECORNER, C.KIND_SCALAR)
    f["uvel"] = U(0.2 * (h("u") - 0.5) * still); f["vvel"] = U(0.2 * (h("v") - 0.5) * still)
    f["iceumask"] = (scatter(np.where(patchU | (h("old") < 0.5), 1.0, 0.0), C.LOC_NECORNER, C.KIND_SCALAR) * f["umask"]).astype(np.int32)
    warm = np.where(band, 1.0, 0.0)
    for k in STRESS_NAMES:
        f[k] = T(1.0e3 * (h(k) - 0.5) * warm)
    for k in ("strintx", "strinty", "strocnx", "strocny"):       # in/out of evp_prep2: zeroed where the ice has gone
        f[k] = U((h(k) - 0.5) * warm)
    # fm, strtltx, strtlty are in/out of evp_prep2 too: it writes them on the active U cells only, so in the reference a cell
    # that lost its ice keeps the value of an earlier step.  The device API has them as outputs only (include/evpk.h) and
    # cannot be handed such a history: the chain starts them as init_evp leaves them (zero, already in f).  That evp_prep2
    # leaves them alone on inactive cells is pinned by its single-routine record, whose inputs are not zero.
    return d, {k: np.ascontiguousarray(v) for k, v in f.items()}


def dyn_params(cfg, case, ndte, f, d):
    """(evpk.Params, orc.OrcParams) of a chain record; their equality is asserted by the generator and by the tests"""
    from cice5_amd import dyn
    from oracle import orc
    v = DYN_CASES[case][3]
    xmin = dyn.local_min_dx(f, d)
    kw = dict(cosw=COSW, sinw=SINW, tilt_from_slope=bool(v["tilt_from_slope"]), wind_on_ugrid=bool(v["wind_on_ugrid"]))
    return dyn.set_evp_parameters(DYN_DT, ndte, bool(v["revised_evp"]), xmin, **kw), orc.make_params(DYN_DT, ndte, xmin, bool(v["revised_evp"]), **kw)


# single-routine records: one call of one routine on one block, inputs straight from the hash
BLOCK_RECORDS = {"g72x20_b72x20": {"full": (2, 73, 2, 21)}, "g26x18_b8x5": {"full": (2, 9, 2, 6), "pad": (2, 3, 2, 4)}}
BLOCK_VARIANTS = {"classic": dict(revised_evp=0, tilt_from_slope=0, ndte=4, ksub=2),          # ksub < ndte
                  "revised": dict(revised_evp=1, tilt_from_slope=1, ndte=4, ksub=4)}          # ksub == ndte: diagnostics
XMIN_BLOCK = 2.0e4


def block_params(var):
    from oracle import orc
    v = BLOCK_VARIANTS[var]
    return orc.make_params(DYN_DT, v["ndte"], XMIN_BLOCK, bool(v["revised_evp"]), cosw=COSW, sinw=SINW,
                           tilt_from_slope=bool(v["tilt_from_slope"]))


def block_inputs(cfg, rec, var):
    """the planes of every single-routine record on a (ny_block, nx_block) block: dict of float64 / int32 arrays"""
    nx, ny, bx, by, _ = KERNEL_CONFIGS[cfg]
    nxb, nyb = bx + 2, by + 2
    ilo, ihi, jlo, jhi = BLOCK_RECORDS[cfg][rec]
    h = lambda k: hash01((nyb, nxb), seed_of(cfg, rec, var, "blk", k))
    r = lambda k, s=1.0: np.ascontiguousarray(s * (h(k) - 0.5))
    q = {}
    q["tmask"] = (h("tmask") > 0.15).astype(np.int32)
    q["umask"] = (h("umask") > 0.15).astype(np.int32)
    thr = h("thr")
    a = np.where(h("icy") < 0.6, 0.3 + 0.7 * h("aice"), 0.0)
    w = 0.05 if nxb * nyb > 500 else 0.1                  # share of the cells at each threshold
    a[thr < w] = A_MIN * (1 - 1e-9); a[(thr >= w) & (thr < 2 * w)] = A_MIN * (1 + 1e-9)
    q["aice"] = a
    q["vice"] = a * (0.5 + 2.5 * h("hi")); q["vsno"] = a * 0.3 * h("hs")
    for lo, eps in ((2 * w, -1e-9), (3 * w, 1e-9)):
        m = (thr >= lo) & (thr < lo + w)
        q["vice"][m] = M_MIN * (1 + eps) / RHOI; q["vsno"][m] = 0.0; q["aice"][m] = np.maximum(q["aice"][m], 0.5)
    q["strairxT"], q["strairyT"] = r("wx", 0.2), r("wy", 0.2)
    # evp_prep2
    aiu = np.where(h("icyu") < 0.6, 0.3 + 0.7 * h("aiu"), 0.0)
    t2 = h("thr2")
    aiu[t2 < w] = A_MIN * (1 - 1e-9); aiu[(t2 >= w) & (t2 < 2 * w)] = A_MIN * (1 + 1e-9)
    um = aiu * 900.0 * (0.5 + h("um"))
    um[(t2 >= 2 * w) & (t2 < 3 * w)] = M_MIN * (1 - 1e-9); um[(t2 >= 3 * w) & (t2 < 4 * w)] = M_MIN * (1 + 1e-9)
    aiu[(t2 >= 2 * w) & (t2 < 4 * w)] = 0.5
    q["aiu"], q["umass"] = aiu, um
    q["fcor"] = r("fcor", 2.8e-4)
    q["uocn"], q["vocn"] = r("uo", 0.1), r("vo", 0.1)
    q["strairx"], q["strairy"] = r("sx", 0.2), r("sy", 0.2)
    q["ss_tltx"], q["ss_tlty"] = r("tx", 1e-6), r("ty", 1e-6)
    q["icetmask"] = (h("itm") < 0.55).astype(np.int32)
    q["iceumask"] = (h("ium") < 0.5).astype(np.int32)
    for k in ("fm", "strtltx", "strtlty", "strocnx", "strocny", "strintx", "strinty", "uvel_init", "vvel_init", "strocnxT", "strocnyT"):
        q[k] = r(k)
    for k in STRESS_NAMES:
        q[k] = r(k, 1.0e3)
    u, v = r("u", 0.2), r("v", 0.2)
    u[3:9, 3:9] = 0.0; v[3:9, 3:9] = 0.0                   # at rest: Delta == 0 exactly on the T cells inside
    q["uvel"], q["vvel"] = u, v
    # stress: an analytic grid (cxp = 1.5 HTN(j) - 0.5 HTN(j-1), ...: ice_grid.F90:338-369) + strength with zeros
    htn = 2.0e4 * (1.0 + 0.3 * h("htn")); hte = 3.0e4 * (1.0 + 0.3 * h("hte"))
    htn_s = np.roll(htn, 1, axis=0); hte_w = np.roll(hte, 1, axis=1)
    q["dxt"], q["dyt"] = 0.5 * (htn + htn_s), 0.5 * (hte + hte_w)
    q["dxhy"], q["dyhx"] = 0.5 * (hte - hte_w), 0.5 * (htn - htn_s)
    q["cxp"], q["cyp"] = 1.5 * htn - 0.5 * htn_s, 1.5 * hte - 0.5 * hte_w
    q["cxm"], q["cym"] = -(1.5 * htn_s - 0.5 * htn), -(1.5 * hte_w - 0.5 * hte)
    tarea = q["dxt"] * q["dyt"]
    q["tarear"], q["tinyarea"], q["uarear"] = 1.0 / tarea, 1.0e-11 * tarea, 1.0 / (tarea * (0.9 + 0.2 * h("ua")))
    s = PSTAR * (0.2 + h("str")); s[h("str0") < 0.1] = 0.0
    q["strength"] = s
    for k in ("shear", "divu", "prs_sig", "rdg_conv", "rdg_shear"):
        q[k] = r("d" + k, 1e-6)
    q["prs"] = np.where(h("prs0") < 0.2, 0.5e-11, PSTAR * h("prs"))          # principal_stress: both sides of puny
    q["str"] = np.ascontiguousarray(1.0e3 * (hash01((8, nyb, nxb), seed_of(cfg, rec, var, "blk", "strtmp")) - 0.5))
    q["Cw"] = 0.00536 * (0.7 + 0.6 * h("cw"))
    q["umassdti"] = um / DYN_DT; q["waterx"], q["watery"], q["forcex"], q["forcey"] = r("wax", 0.1), r("way", 0.1), r("fx"), r("fy")
    # the lists, as evp_prep2 builds them: T cells jlo..jhi+1 x ilo..ihi+1 with icetmask = 1, U cells with aiu > 0.01
    def lst(mask, j1, i1):
        m = np.zeros_like(mask, dtype=bool); m[jlo - 1:j1, ilo - 1:i1] = mask[jlo - 1:j1, ilo - 1:i1] != 0
        j, i = np.nonzero(m)
        out = np.zeros((2, nxb * nyb), dtype=np.int32); out[0, :len(i)] = i + 1; out[1, :len(i)] = j + 1
        return out, len(i)
    q["indxt"], q["icellt"] = lst(q["icetmask"], jhi + 1, ihi + 1)
    q["indxu"], q["icellu"] = lst((aiu > 0.01) & (q["umask"] != 0), jhi, ihi)
    return {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in q.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the REMAP fixtures (oracle/ref/ref_remap.F90, tests/golden/make_ref_remap.py -> ref_remap_*.npz): the reference's own
# make_masks / construct_fields / limited_gradient / departure_points / locate_triangles / triangle_coordinates /
# transport_integrals / update_fields, alone on one block and chained on the whole grid in horizontal_remap's order.
REMAP_NCAT = 3                                   # NICECAT of the ref_remap build (RNCAT in oracle/ref/Makefile)
REMAP_DEPEND = (0, 1, 2 + 1, 2 + 2)              # with hice, hsno in front: tracer types 1, 1, 1, 2, 2, 3
REMAP_DT = 3600.0
# the largest local Courant number |u| dt / dxu of the rough velocities.  Found on the CPU with the reference binary
# (make_ref_remap.py --courant): departure_points accepts every value below 1, but the divergent corners of a field whose
# sign changes from corner to corner empty a cell faster than a uniform flow does, and update_fields stops on a negative
# mass in some case of some config for 0.45 and above (in steps of 0.05: 9, 8, 8, 7, 3, 2, 1 of the 20 chains stop at 0.9, 0.8,
# 0.7, 0.6, 0.55, 0.5, 0.45); 0.4 is the largest step for which no chain stops.
REMAP_COURANT = 0.4
# case -> (boundary / land case of DYN_CASES, trcr_depend or None for ntrace = 0, [(integral_order, l_dp_midpt), ...]);
# the six (order, rule) pairs all occur
REMAP_CASES = {
    "cyclic_open": ("cyclic_open", REMAP_DEPEND, [(3, 1), (2, 0)]),
    "cyclic_tripole": ("cyclic_tripole", REMAP_DEPEND, [(3, 1), (1, 0)]),
    "open_closed_rim": ("open_closed_rim", REMAP_DEPEND, [(3, 0), (2, 1)]),
    "cyclic_open_patch": ("cyclic_open_patch", REMAP_DEPEND, [(1, 1), (3, 1)]),
    "areas_only": ("cyclic_tripole", None, [(3, 1), (2, 0)]),
}
# the two stop cases -> (return code, integral_order, l_dp_midpt): the fields of `cyclic_open` with one corner moving 1.25
# cells, resp. the four corners of one cell flying apart at Courant 0.95 under the Euler rule (the midpoint rule reads the
# velocity half way, where such a field has almost none) (remap_fields)
REMAP_STOPS = {"bad_departure": (1, 3, 1), "negative_mass": (2, 3, 0)}
REMAP_GRID = ["hm", "uvel", "vvel", "dxu", "dyu", "HTN", "HTE", "tarear"]        # the planes ref_remap.F90 reads, in its order


def remap_tables(trcr_depend):
    from oracle import orc
    if trcr_depend is None:
        e = np.zeros(0, dtype=np.int32)
        return e, e.copy(), e.copy()
    return orc.remap_tables(list(trcr_depend))


def _remap_state(h, icy, ocean, ncat, ntrace):
    """mm (ncat + 1, ...), tm (ncat, ntrace, ...) on arrays of any shape: categories with holes, masses at, just below and
    just above puny, tracers with dependents at |tm| <= puny and exactly zero, values without meaning in cells without ice"""
    shape = icy.shape
    mm = np.zeros((ncat + 1,) + shape)
    tm = np.zeros((ncat, ntrace) + shape)
    for n in range(1, ncat + 1):
        a = 0.05 + 0.25 * h(f"a{n}")
        a[h(f"hole{n}") < 0.25] = 0.0
        thr = h(f"thr{n}")
        a[thr < 0.04] = 0.5e-11
        a[(thr >= 0.04) & (thr < 0.07)] = 1.0e-11
        a[(thr >= 0.07) & (thr < 0.10)] = 1.0e-11 * (1 + 1e-6)
        a[~icy] = 0.0
        mm[n] = a
        for k in range(ntrace):
            t = h(f"t{n}_{k}")
            if k == 0:
                v = 0.2 + 3.0 * t                                # hice
            elif k == 1:
                v = np.where(t < 0.2, 0.0, 0.3 * t)              # hsno
            else:
                v = 4.0 * t - 2.0
            if k in (0, 2, 3):                                   # the tracers other tracers depend on (REMAP_DEPEND)
                s = h(f"s{n}_{k}")
                v = np.where(s < 0.05, 0.5e-11 * np.sign(v), v)
                v = np.where((s >= 0.05) & (s < 0.08), 0.0, v)
            junk = h(f"j{n}_{k}") < 0.3
            tm[n - 1, k] = np.where((a > 0) | junk, v, 0.0)
    mm[0] = np.where(ocean, 1.0 - mm[1:].sum(axis=0), 0.0)
    return mm, tm


def _remap_courant(h, shape, courant):
    """Courant numbers per corner in (-courant, courant) with sign changes from corner to corner; 6 % of the corners at rest,
    5 % each with exactly one component zero (ydl == 0, ydr == 0, xdl == xcl of locate_triangles under the Euler rule)"""
    cx, cy = courant * (2.0 * h("cx") - 1.0), courant * (2.0 * h("cy") - 1.0)
    z = h("zero")
    cx[z < 0.11] = 0.0
    cy[(z < 0.06) | ((z >= 0.11) & (z < 0.16))] = 0.0
    return cx, cy


def remap_fields(cfg, case, courant=None, stop=None):
    """(decomp, fields, mm, tm, tables) of a chain record: the grid, masks and boundaries of dyn_fields(cfg, base case) with
    the remap grid arrays, a rough velocity field and an ice state from the hash; ghost cells current (halo updates of the
    pinned restatement).  stop: one of REMAP_STOPS."""
    from cice5_amd import constants as C, synth
    from oracle import orc
    base, trcr_depend, _ = REMAP_CASES[case]
    nx, ny, bx, by, _ = KERNEL_CONFIGS[cfg]
    ew, ns, land, _ = DYN_CASES[base]
    d, f = dyn_fields(cfg, base)
    sc = synth.SynthCase(nx=nx, ny=ny, ew_boundary=C.BND_NAMES[ew], ns_boundary=C.BND_NAMES[ns], land="none")
    synth.add_remap_grid(sc, d, f)
    f["hm"] = f["tmask"].astype(np.float64)
    kmt, _ = kmt_ulat(nx, ny, bx, by, ew, ns, land)
    ocean = kmt > 0
    h = lambda k: hash01((ny, nx), seed_of(cfg, case, "remap", k))
    tables = remap_tables(trcr_depend)
    ntrace = len(tables[0])

    def scatter(G, loc, kind):
        a = np.zeros((d.nblocks, d.ny_block, d.nx_block))
        for n, b in enumerate(d.local_blocks):
            ni, nj = b.ihi - b.ilo + 1, b.jhi - b.jlo + 1
            a[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = G[b.jglob_lo - 1:b.jglob_lo - 1 + nj, b.iglob_lo - 1:b.iglob_lo - 1 + ni]
        orc.halo_r8(d, a, loc, kind, 0.0)
        return a
    jj, ii = np.meshgrid(np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    icy = ocean & (h("icy") < 0.85)
    gm, gt = _remap_state(h, icy, ocean, REMAP_NCAT, ntrace)
    cx, cy = _remap_courant(h, (ny, nx), REMAP_COURANT if courant is None else courant)
    pc, pr = zero_patch(nx)
    rest = (ii >= pc) & (ii < pc + 5) & (jj >= pr) & (jj < pr + 5)
    cx[rest] = 0.0; cy[rest] = 0.0
    I, J = np.arange(1, nx + 1)[None, :], np.arange(1, ny + 1)[:, None]
    gu = cx * sc.field("dxu", I, J) / REMAP_DT
    gv = cy * sc.field("dyu", I, J) / REMAP_DT
    # two pairs of departure points that mirror each other through the midpoint of a north resp. an east edge in exact arithmetic
    # (dx, dy = -/+ 1/4, +/- 1/8 on the north edge, the same rotated on the east edge): xic == 0 and ydm == 0 under the Euler
    # rule, the equalities of `xic >= c0` and `ydm >= c0` (:2564-2565).  The corners' dxu, dyu become 4 dt S and 8 dt S' with
    # S, S' the powers of two that change them least (below), their velocities S, S', so every quotient is exact.  The corners
    # lie inside a block of either config, away from the land of every case and from the patch at rest.
    jm = ny - 6
    gdx, gdy = sc.field("dxu", I, J) + 0 * J, sc.field("dyu", I, J) + 0 * I
    pow2 = lambda x: 2.0 ** np.round(np.log2(x))
    mirror = []
    for pair, kx, ky in ((((jm, 11, 1.0, -1.0), (jm, 12, -1.0, 1.0)), 4, 8), (((jm, 14, -1.0, -1.0), (jm - 1, 14, 1.0, 1.0)), 8, 4)):
        sx = pow2(max(gdx[j, i] for j, i, _, _ in pair) / (kx * REMAP_DT))
        sy = pow2(max(gdy[j, i] for j, i, _, _ in pair) / (ky * REMAP_DT))
        for j, i, su, sv in pair:
            assert ocean[j - 1:j + 2, i - 1:i + 2].all() and not rest[j, i]
            gu[j, i], gv[j, i] = su * sx, sv * sy
            mirror.append((j, i, kx * REMAP_DT * sx, ky * REMAP_DT * sy))
    jc, ic = ny // 2, (2 * nx) // 3                      # 0-based cell well inside the ocean of every case
    if stop == "bad_departure":
        gu[jc, ic] = -1.25 * sc.field("dxu", I, J)[jc, ic] / REMAP_DT
    elif stop == "negative_mass":                        # the four corners of one cell fly apart at Courant 0.95
        for dj, di, su, sv in ((0, 0, 1, 1), (0, -1, -1, 1), (-1, 0, 1, -1), (-1, -1, -1, -1)):
            gu[jc + dj, ic + di] = su * 0.95 * sc.field("dxu", I, J)[jc + dj, ic + di] / REMAP_DT
            gv[jc + dj, ic + di] = sv * 0.95 * sc.field("dyu", I, J)[jc + dj, ic + di] / REMAP_DT
        gm[1, jc, ic] = 0.3
        gm[0, jc, ic] = 1.0 - gm[1:, jc, ic].sum()
    else:
        assert stop is None
    for j, i, new_dxu, new_dyu in mirror:
        for n, b in enumerate(d.local_blocks):
            lj, li = j + 1 - b.jglob_lo + b.jlo - 1, i + 1 - b.iglob_lo + b.ilo - 1          # 0-based block-local indices
            if b.jlo - 1 <= lj < b.jhi and b.ilo - 1 <= li < b.ihi:
                assert b.jlo - 1 < lj < b.jhi - 1 and b.ilo - 1 < li < b.ihi - 1, "a mirror corner lies in a neighbour's halo"
                f["dxu"][n, lj, li], f["dyu"][n, lj, li] = new_dxu, new_dyu
    f["uvel"] = scatter(gu, C.LOC_NECORNER, C.KIND_VECTOR) * f["umask"]
    f["vvel"] = scatter(gv, C.LOC_NECORNER, C.KIND_VECTOR) * f["umask"]
    mm = np.stack([scatter(gm[n], C.LOC_CENTER, C.KIND_SCALAR) for n in range(REMAP_NCAT + 1)], axis=1)
    tm = np.zeros((d.nblocks, REMAP_NCAT, ntrace, d.ny_block, d.nx_block))
    for n in range(REMAP_NCAT):
        for k in range(ntrace):
            tm[:, n, k] = scatter(gt[n, k], C.LOC_CENTER, C.KIND_SCALAR)
    f = {k: np.ascontiguousarray(v) for k, v in f.items()}
    return d, f, np.ascontiguousarray(mm), np.ascontiguousarray(tm), tables


# single-routine records: one call of each routine on one block of g26x18_b8x5 (a 10 x 7 block keeps the triangle arrays
# small), every cell of every input plane -- ghost cells included -- its own value from the hash
REMAP_BLOCK_CFG = "g26x18_b8x5"
REMAP_BLOCK_VARIANTS = {"t6_o3_mid": (REMAP_DEPEND, 3, 1), "t6_o2_euler": (REMAP_DEPEND, 2, 0), "t6_o1_mid": (REMAP_DEPEND, 1, 1),
                        "t3_o3_euler": ((0, 1), 3, 0),           # types 1, 1, 1, 2 with hice the only tracer with dependents
                        "t0_o3_mid": (None, 3, 1),
                        "t6_stop": (REMAP_DEPEND, 3, 1)}         # departure_points stops
REMAP_BLOCK_GRID = REMAP_GRID + ["phi", "cnx", "cny"]


def remap_block_inputs(rec, var):
    """mm (ncat + 1, ny, nx), tm (ncat, ntrace, ny, nx), the planes of REMAP_BLOCK_GRID, the tables"""
    cfg = REMAP_BLOCK_CFG
    nx, ny, bx, by, _ = KERNEL_CONFIGS[cfg]
    nxb, nyb = bx + 2, by + 2
    trcr_depend, order, midpt = REMAP_BLOCK_VARIANTS[var]
    tables = remap_tables(trcr_depend)
    h = lambda k: hash01((nyb, nxb), seed_of(cfg, rec, var, "rblk", k))
    ocean = h("ocean") > 0.1
    mm, tm = _remap_state(h, ocean & (h("icy") < 0.85), ocean, REMAP_NCAT, len(tables[0]))
    q = {"hm": ocean.astype(np.float64)}
    q["dxu"], q["dyu"] = 2.0e4 * (1.0 + 0.3 * h("dxu")), 3.0e4 * (1.0 + 0.3 * h("dyu"))
    q["HTN"], q["HTE"] = 2.0e4 * (1.0 + 0.3 * h("htn")), 3.0e4 * (1.0 + 0.3 * h("hte"))
    q["tarear"] = 1.0 / (q["HTN"] * q["HTE"])
    cx, cy = _remap_courant(h, (nyb, nxb), 0.6)
    q["uvel"], q["vvel"] = cx * q["dxu"] / REMAP_DT, cy * q["dyu"] / REMAP_DT
    if var == "t6_o2_euler" and rec == "full":
        # (a) departure points BETWEEN the two bounds of the stop test (ice_transport_remap.F90:1564-1565 compares dpx with
        # HTN(i+1,j), dpy with HTE(i,j+1), not with the corner's own): no stop
        j, i = next((j, i) for j in range(1, 3) for i in range(1, nxb - 2) if q["HTN"][j, i + 1] > 1.05 * q["HTN"][j, i])
        q["uvel"][j, i] = -0.5 * (q["HTN"][j, i] + q["HTN"][j, i + 1]) / REMAP_DT
        j, i = next((j, i) for j in range(4, nyb - 2) for i in range(1, 4) if q["HTE"][j + 1, i] > 1.05 * q["HTE"][j, i])
        q["vvel"][j, i] = -0.5 * (q["HTE"][j, i] + q["HTE"][j + 1, i]) / REMAP_DT
        # (b) two departure points that mirror each other through the midpoint of a north edge, in exact arithmetic (dx = -/+ 1/4,
        # dy = +/- 1/8): xic == 0 and ydm == 0, the equalities of `xic >= c0` and `ydm >= c0` (:2564-2565)
        for i, sgn in ((5, 1.0), (6, -1.0)):
            q["dxu"][3, i], q["dyu"][3, i] = 4 * REMAP_DT, 8 * REMAP_DT
            q["uvel"][3, i], q["vvel"][3, i] = sgn, -sgn
    if var == "t6_stop":
        q["vvel"][3, 4] = 1.5 * q["HTE"][3, 4] / REMAP_DT; q["uvel"][2, 2] = -1.5 * q["HTN"][2, 2] / REMAP_DT
    jj, ii = np.meshgrid(np.arange(nyb), np.arange(nxb), indexing="ij")          # a ramp under the noise: few cells are extrema
    q["phi"], q["cnx"], q["cny"] = 0.35 * ii - 0.25 * jj + 0.8 * h("phi"), 0.2 * (h("cnx") - 0.5), 0.2 * (h("cny") - 0.5)
    return mm, tm, {k: np.ascontiguousarray(q[k]) for k in REMAP_BLOCK_GRID}, tables, order, midpt


# The (group, iflux - i, jflux - j, sign of triarea) signatures locate_triangles can produce with l_fixed_area = .false.,
# per edge kind.  Source cells (ice_transport_remap.F90:1879-1890 north, :1913-1924 east): TL, BL, TR, BR, TC, BC.  The sign
# of triarea per group and source cell: REMAP_SIGNS below.
#   group 1  TL (:2057)  BL (:2072)  TL1 (:2087, with BL1 in group 3)  BL2 (:2115, with TL2 in group 3)
#   group 2  TR (:2150)  BR (:2165)  TR1 (:2180, with BR1 in group 3)  BR2 (:2208, with TR2 in group 3)
#   group 3  BL1 (:2087)  TL2 (:2115)  BR1 (:2180)  TR2 (:2208)
#   groups 4, 5, 6  the TC / BC triangles: all three in TC (:2397), all three in BC (:2478), and the eight crossing cases
#            ydl >= 0 > ydr (:2564, :2606, :2648, :2690) and ydl < 0 <= ydr (:2732, :2774, :2816, :2858) by the sign of xic and
#            of ydm, which put group 4 and 5 on opposite sides of the edge and group 6 on the side of ydm.
# Every signature below must occur on both edge kinds in the chain fixtures; beyond the signatures, REMAP_PATTERNS names the
# branches by the source cells of several groups of ONE edge, which tells apart what a signature alone cannot.
# EXCLUDED as unreachable: GROUP 6 altogether.  With l_fixed_area = .false. its triangle is (DL, DR, DM), (DL, IC, DM) or
# (ICR, ICL, DM) (:2397-2898): DM is the midpoint of DL DR, IC lies on that line, and ICL = ICR = IC (:2047-2050; :2257-2388 move them and DM
# only when the area is prescribed), so its three vertices are collinear or two of them coincide, its area is zero up to rounding
# and falls under the eps16 threshold (:2940): the reference lists no group-6 triangle on any fixture (the generator and
# assert_remap_coverage fail if one appears).  For the same reason the SIGN OF ydm cannot be told from any output: the
# two branches of each crossing case that differ in it give groups 4 and 5 the same vertices, source cells and area factors
# and differ in group 6 only; the patterns below therefore tell the crossing cases apart by the sign of xic alone.
# ALSO EXCLUDED: "ydl >= 0, ydr >= 0, ydm < 0" (:2437) and "ydl < 0, ydr < 0, ydm >= 0" (:2519), both marked rare.  With
# l_fixed_area = .false. DM is the midpoint of DL DR (:2027-2028) and is never moved; DL / DR are moved to IL / IR (:2242-2250),
# which lie on the same straight line, so as long as xcl <= xdm <= xcr -- that is |dx_left + dx_right| <= 1, true for every
# Courant number up to 0.5 -- ydm lies between the two ordinates and cannot have the sign neither has.  (Beyond 0.5 the
# midpoint can leave the edge's span; REMAP_COURANT stays below.)
def _shifts(north):
    return dict(TL=(-1, 1), BL=(-1, 0), TR=(1, 1), BR=(1, 0), TC=(0, 1), BC=(0, 0)) if north else \
           dict(TL=(1, 1), BL=(0, 1), TR=(1, -1), BR=(0, -1), TC=(1, 0), BC=(0, 0))


# group -> (source cell, sign of triarea) it can hold; the sign is that of areafact times the orientation of the three vertices
# in the order the branch stores them (A > 0 iff counterclockwise, :2934-2938), worked out from CL = (-1/2, 0), CR = (1/2, 0) and
# the branch's own conditions:  TL (CL, IL, DL) ccw x -  |  BL (CL, DL, IL) ccw x +  |  TL1 (CL, DL, IC) ccw x +  with
# BL1 (CL, IC, IL) ccw x +  |  TL2 (CL, IL, IC) ccw x -  with BL2 (CL, IC, DL) ccw x -; the right-hand side mirrored;
# group 4 (CL, CR / IC, DL) is ccw in every branch: - in TC, + in BC; group 5 (CR, DR, DL / IC) is ccw in the crossing cases
# and "nearly always" otherwise (:2911-2918: when it is not, the quadrilateral is the difference of two triangles): both signs.
REMAP_SIGNS = {1: (("TL", -1), ("TL", 1), ("BL", 1), ("BL", -1)), 2: (("TR", -1), ("TR", 1), ("BR", 1), ("BR", -1)),
               3: (("TL", -1), ("BL", 1), ("TR", -1), ("BR", 1)), 4: (("TC", -1), ("BC", 1)),
               5: (("TC", -1), ("BC", 1), ("TC", 1), ("BC", -1))}


def remap_signatures(north):
    s = _shifts(north)
    return {(g,) + s[c] + (sign,) for g, cells in REMAP_SIGNS.items() for c, sign in cells}


# branch name -> {group: its source cell on one edge, or (cell, False): the group does not hold a triangle of that cell;
# "xic": sign of xic, 1 standing for `xic >= c0`, 0 for xic == 0 exactly}
REMAP_PATTERNS = {
    "TL": {1: "TL", 3: ("BL", False)}, "BL": {1: "BL", 3: ("TL", False)}, "TL1+BL1": {1: "TL", 3: "BL"}, "TL2+BL2": {1: "BL", 3: "TL"},
    "TR": {2: "TR", 3: ("BR", False)}, "BR": {2: "BR", 3: ("TR", False)}, "TR1+BR1": {2: "TR", 3: "BR"}, "TR2+BR2": {2: "BR", 3: "TR"},
    "TC*a": {4: "TC", 5: "TC"}, "BC*a": {4: "BC", 5: "BC"},
    # the crossing cases (:2564-2898) by the sign of xic, read back from the vertex of the BC triangle that lies on the edge
    "ydl>=0>ydr xic>=0": {4: "TC", 5: "BC", "xic": 1}, "ydl>=0>ydr xic<0": {4: "TC", 5: "BC", "xic": -1},
    "ydl<0<=ydr xic<0": {4: "BC", 5: "TC", "xic": -1}, "ydl<0<=ydr xic>=0": {4: "BC", 5: "TC", "xic": 1},
    "ydl>=0>ydr xic==0": {4: "TC", 5: "BC", "xic": 0},          # the mirrored pairs of remap_fields (Euler rule)
}
