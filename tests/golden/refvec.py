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
