"""Deterministic inputs of the ridge_ice fixtures (tests/golden/make_ref_ridge.py -> ref_ridge_<cfg>.<case>.npz) and of the tests that
feed the same bytes to the numpy restatement (tests/npridge.py) and to the HIP path.  Everything comes from refvec.hash01.

A state "after transport": thickness distributions as refvec.strength_input makes them (open-water fractions on both sides of Gstar,
empty categories, aicen at 0.5 puny), with the areas scaled so that aice0 + sum(aicen) differs from 1 in both directions on most cells,
strongly on the blocks whose index is odd and hardly at all on the others (so that some blocks repeat ridging and some do not), and
deformation rates that include zeros.
"""
from __future__ import annotations

import numpy as np

from . import refvec
from .refvec import hash01, seed_of

CONFIGS = {"g24x16_b24x16": refvec.CONFIGS["g24x16_b24x16"], "g26x18_b8x5": refvec.CONFIGS["g26x18_b8x5"]}
LAND = {"g24x16_b24x16": "none", "g26x18_b8x5": "patch"}
NCAT = refvec.NCAT
HIN_MAX = np.array([0.0, 0.64, 1.39, 2.47, 4.57, 9.0])              # (the same boundaries as refvec.strength_input)
DT, NDTD = 3600.0, 2
MU_RDG, RHOS = refvec.MU_RDG, refvec.RHOS
SWITCHES = {"p1r1": (1, 1), "p0r1": (0, 1)}                          # (krdg_partic, krdg_redist)

# refvec.TRACER_CASES extended with nt_qsno / nt_vlvl / nt_hpnd (nslyr = 1: NSNWLYR of the reference build), plus a tr_pond_topo table
# Tsfc, qice, qsno, alvl, vlvl, apnd, hpnd, fbri, a brine tracer
_FULL = dict(nt_qsno=3, nslyr=1, nt_alvl=4, nt_vlvl=5, nt_apnd=6, nt_hpnd=7, nt_fbri=8)
TRACER_CASES = {
    "lvl_ponds": (refvec.TRACER_CASES["lvl_ponds"][0], dict(_FULL, tr_pond_lvl=1)),
    "cesm_ponds": (refvec.TRACER_CASES["cesm_ponds"][0], dict(_FULL, tr_pond_cesm=1)),
    "plain": (refvec.TRACER_CASES["plain"][0], dict(nt_qsno=4, nslyr=1)),
    "topo_ponds": (refvec.TRACER_CASES["cesm_ponds"][0], dict(_FULL, tr_pond_topo=1)),
}
# the records of each configuration: (tracer case, switches)
RECORDS = {
    "g26x18_b8x5": [(t, s) for t in TRACER_CASES for s in SWITCHES],
    "g24x16_b24x16": [("lvl_ponds", "p1r1"), ("cesm_ponds", "p0r1"), ("plain", "p1r1"), ("topo_ponds", "p0r1")],
}
DIAG_2D = ["dardg1dt", "dardg2dt", "dvirdgdt", "opening", "fpond", "fresh", "fhocn"]
DIAG_3D = ["dardg1ndt", "dardg2ndt", "dvirdgndt", "aparticn", "krdgn", "araftn", "vraftn", "aredistn", "vredistn"]
STATE = ["aice0", "aicen", "vicen", "vsnon", "trcrn"]


def record_name(tcase, sw):
    return f"{tcase}_{sw}"


def decomp(cfg):
    from cice5_amd import blocks
    nx, ny, bx, by, _ = CONFIGS[cfg]
    return blocks.create_distrb_cart(nx, ny, bx, by, ew_boundary_type="cyclic", ns_boundary_type="open")


def tmask(cfg, d):
    """int32 (nb, ny, nx): ocean on the cells of the grid, land on the patch, 0 beyond the north / south boundary and on padding"""
    from cice5_amd import blocks
    nx, ny, bx, by, _ = CONFIGS[cfg]
    kmt, _ = refvec.kmt_ulat(nx, ny, bx, by, "cyclic", "open", LAND[cfg])

    def fn(I, J):
        Ig = (I - 1) % nx
        ok = (J >= 1) & (J <= ny) & (I >= 1) & (I <= nx)
        return np.where(ok, kmt[np.clip(J - 1, 0, ny - 1), Ig], 0)
    return np.ascontiguousarray(blocks.to_blocks(d, fn).astype(np.int32))


def listed(d, tm):
    """bool (nb, ny, nx): step_ridge's list -- physical cells with tmask"""
    m = np.zeros(tm.shape, dtype=bool)
    for n, b in enumerate(d.local_blocks):
        m[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = tm[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] != 0
    return m


def ridge_input(cfg, tcase, ncat=NCAT, tag="fix", strong=None):
    """dict of the arrays of one ridge_ice call on every block; `strong`: per-block amplitude of the area imbalance (default: odd
    blocks strong, even blocks balanced)"""
    d = decomp(cfg)
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    dep, tr = TRACER_CASES[tcase]
    ntrcr = len(dep)
    h = lambda k, shape: hash01(shape, seed_of(cfg, "ridge", tag, tcase if k.startswith("t") else "", k))
    hin = HIN_MAX if ncat == NCAT else np.concatenate([HIN_MAX[:ncat], [9.0]])
    aicen = h("a", (nb, ncat, ny, nx))
    aicen[h("hole", (nb, ncat, ny, nx)) < 0.25] = 0.0
    tot = aicen.sum(axis=1)
    target = h("tot", (nb, ny, nx)) ** 0.3
    target[h("full", (nb, ny, nx)) < 0.15] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        aicen = np.where(tot[:, None] > 0, aicen * (target / tot)[:, None], 0.0)
    frac = h("hh", (nb, ncat, ny, nx))
    hi = hin[:-1, None, None] + frac * (hin[1:, None, None] - hin[:-1, None, None])
    vicen = aicen * hi
    aicen[aicen < 1e-11] = 0.0
    aicen[h("tiny", (nb, ncat, ny, nx)) < 0.03] = 0.5e-11
    aice0 = np.maximum(1.0 - aicen.sum(axis=1), 0.0)
    vsnon = aicen * 0.4 * h("hs", (nb, ncat, ny, nx))
    vsnon[h("s0", (nb, ncat, ny, nx)) < 0.2] = 0.0
    # "transport": the areas no longer sum to 1 -- both directions; and the deformation rates, zeros included
    if strong is None:
        strong = np.array([1.0 if b % 2 else 0.0 for b in range(nb)]) if nb > 1 else np.ones(1)
    amp = np.asarray(strong, dtype=float)[:, None, None]
    e = (h("e", (nb, ny, nx)) * 0.2 - 0.08) * amp
    e[h("e0", (nb, ny, nx)) < 0.3] = 0.0
    aicen = aicen * (1.0 + e)[:, None]
    vicen = vicen * (1.0 + e)[:, None]
    aice0 = aice0 * (1.0 + e)
    conv = h("conv", (nb, ny, nx)) * 2.0e-5 * (0.02 + amp)
    conv[h("c0", (nb, ny, nx)) < 0.3] = 0.0
    shear = h("shear", (nb, ny, nx)) * 4.0e-5 * (0.02 + amp)
    shear[h("sh0", (nb, ny, nx)) < 0.3] = 0.0
    trcrn = h("trcrn", (nb, ncat, ntrcr, ny, nx)) * 2.0 - 0.7
    for k in ("nt_alvl", "nt_apnd", "nt_fbri", "nt_vlvl", "nt_hpnd"):          # fractions / depths: in [0, 1), some exactly 0
        nt = tr.get(k, 0)
        if nt:
            f = h("t" + k, (nb, ncat, ny, nx))
            f[h("t0" + k, (nb, ncat, ny, nx)) < 0.1] = 0.0
            trcrn[:, :, nt - 1] = f
    c = np.ascontiguousarray
    tm = tmask(cfg, d)
    out = dict(d=d, tmask=tm, listed=listed(d, tm), ncat=ncat, ntrcr=ntrcr, trcr_depend=np.array(dep, dtype=np.int32), tracers=dict(tr),
               hin_max=hin.copy(), dt=DT, ndtd=NDTD, mu_rdg=MU_RDG, rhos=RHOS,
               rdg_conv=c(conv), rdg_shear=c(shear), aice0=c(aice0), aicen=c(aicen), vicen=c(vicen), vsnon=c(vsnon), trcrn=c(trcrn))
    for k in DIAG_2D:                           # every cell its own value: a cell the call leaves alone stays recognisable
        out[k] = c(h("d" + k, (nb, ny, nx)) - 0.5)
    for k in DIAG_3D:
        out[k] = c(h("d" + k, (nb, ncat, ny, nx)) - 0.5)
    return out


def blocks_of(d):
    return [(b.ilo, b.ihi, b.jlo, b.jhi) for b in d.local_blocks]


# tiny stop records (one block, g24x16_b24x16's build): one input per l_stop reason that inputs can provoke.  One cell (i, j) (1-based
# block indices) of the "plain" state is overwritten with open water aice0 and a single category n (1-based) of area a, thickness h:
#   aice0_negative  aice0 = -0.2 and asum = 1: nothing closes, nothing opens, aice0 stays below -puny                      (:1583)
#   ardg_exceeds    an area of 1e9: ardg1n = apartic * closing_gross * dt, reduced to "100 %" by tmpfac, exceeds aicen by more
#                   than puny through round-off at that magnitude                                                           (:1656)
#   niter           an area of 1e4 of 8 m ice: each pass removes the whole category and returns 1 / krdg ~ 1 / 2.2 of it      (:453)
# |asum - 1| > puny at the end (:729) cannot be provoked: ridge_check lets only |asum - 1| < puny leave the loop, so it would take
# |asum - 1| == puny exactly.
STOPS = {"aice0_negative": dict(cell=(7, 5), aice0=-0.2, n=3, a=1.2, h=2.0 / 1.2, reason=1),
         "ardg_exceeds": dict(cell=(9, 6), aice0=0.0, n=5, a=1.0e9, h=8.0, reason=2),
         "niter": dict(cell=(9, 6), aice0=0.0, n=5, a=1.0e4, h=8.0, reason=3)}


def stop_input(name):
    x = ridge_input("g24x16_b24x16", "plain", tag="stop")
    sp = STOPS[name]
    i, j = sp["cell"]
    x["aice0"][0, j - 1, i - 1] = sp["aice0"]
    for k in ("aicen", "vicen", "vsnon"):
        x[k][0, :, j - 1, i - 1] = 0.0
    x["aicen"][0, sp["n"] - 1, j - 1, i - 1] = sp["a"]
    x["vicen"][0, sp["n"] - 1, j - 1, i - 1] = sp["a"] * sp["h"]
    x["rdg_conv"][0, j - 1, i - 1] = 0.0
    x["rdg_shear"][0, j - 1, i - 1] = 0.0
    return x
