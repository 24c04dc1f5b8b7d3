"""Deterministic inputs of the step_therm2 tests (tests/nptherm2.py, evpk_new_ice_lateral_melt, evpk_step_therm2): the two grids of
tests/golden/litdvec.py with their land masks and itdvec's quiet state -- thickness distributions inside their category bounds on 60 % of
the ocean cells -- under tracer tables of their own (itdvec's carry tr_brine and no nt_sice):
  Tsfc, qice x 4, qsno, sice x 4, iage, FY, alvl, vlvl           "plain"
  ... and apnd, hpnd on top                                      "lvl_ponds", "cesm_ponds", "topo_ponds"
  Tsfc, qice x 4, qsno, sice x 4                                 "bare" (tr_iage, tr_FY, tr_lvl off)
salinz is horizontally uniform (include/evpk.h, departure (b)).  Block 1 (0-based) of a grid of several blocks is ice-free.  No shape is
larger than 26 x 18 cells.

Each ocean cell draws a kind, so that a block mixes them (vi0new below: frzmlt dt / (rhoi Lfresh), which ktherm = 2 makes up to 4 x larger):
  neg, zero      frzmlt = -30, frzmlt = 0
  thin           new ice thinner than hfrazilmin:                         hi0new = hfrazilmin
  mid            vi0new = 0.1 aice0:                                      hfrazilmin < hi0new < hi0max
  surplus        an ice cell, vi0new = 2 aice0:                           aice0 > puny, hi0new > hi0max, aice0 + puny < 1 -- both lists
  surplus_empty  the same with category 3 emptied;  surplus_tinyv: with aicen(4) = 2e-11, vicen(4) = 5e-12 (0 < vicen <= puny)
  thick_free     an ice-free cell, vi0new = 2:                            a single category thicker than hi0max (rebin moves it)
  full, full5    areas that sum to exactly 1 resp. 1 - 5e-12:             no open water, aice0 = 0 and aice0 = 5e-12
  empty1         category 1 emptied, thin new ice;  empty1_tiny: frzmlt = 1e-8, vicen(1) <= puny after the merge;
  empty1_warm    the same with Tf = +0.5:                                 the Tsfc clamp
  fy1            FY = 1 in category 1
  alvl0          alvl = 0 in category 1 of area 0.1, frzmlt = 2e-10:      ai0new below puny aicen(1): the level-pond rule is skipped
Independently: rside <= 0 (0 and -0.1), in (0, 1), exactly 1; sss in {0, 1.2, 5, 34, 100} (both Si0new formulas, the -0.1 clamp of Ti,
both sides of Sb_liq); frz_onset 0 or 200.
"""
from __future__ import annotations

import numpy as np

from . import itdvec, litdvec
from .refvec import hash01, seed_of

CONFIGS = litdvec.CONFIGS
PUNY = itdvec.PUNY
NILYR, NSLYR = itdvec.NILYR, itdvec.NSLYR
_BASE = dict(nt_Tsfc=1, nt_qice=2, nilyr=NILYR, nt_qsno=6, nslyr=NSLYR, nt_sice=7)
_FULL = dict(_BASE, nt_iage=11, nt_FY=12, nt_alvl=13, nt_vlvl=14)
_DEP = [0, 1, 1, 1, 1, 2, 1, 1, 1, 1]
_DEPF = _DEP + [1, 0, 0, 1]
TRACER_CASES = {
    "plain": (_DEPF, dict(_FULL)),
    "lvl_ponds": (_DEPF + [2 + 13, 2 + 15], dict(_FULL, nt_apnd=15, nt_hpnd=16, tr_pond_lvl=1)),
    "cesm_ponds": (_DEPF + [0, 2 + 15], dict(_FULL, nt_apnd=15, nt_hpnd=16, tr_pond_cesm=1)),
    "topo_ponds": (_DEPF + [0, 2 + 15], dict(_FULL, nt_apnd=15, nt_hpnd=16, tr_pond_topo=1)),
    "bare": (_DEP, dict(_BASE)),
}
POND_CASES = ["plain", "lvl_ponds", "cesm_ponds", "topo_ponds"]
HIN0 = {"plain": 0.1, "lvl_ponds": 0.0, "cesm_ponds": 0.1, "topo_ponds": 0.0, "bare": 0.0}
HI_MIN = 0.05
SSS = [0.0, 1.2, 5.0, 34.0, 100.0]
SCALARS = dict(yday=123.0, hfrazilmin=0.05, phi_init=0.75, dSin0_frazil=3.0, cp_ocn=4218.0, rhow=1026.0)
ICE_KINDS = [("neg", 0.12), ("zero", 0.08), ("thin", 0.14), ("mid", 0.14), ("surplus", 0.1), ("surplus_empty", 0.05), ("surplus_tinyv", 0.05),
             ("full", 0.05), ("full5", 0.05), ("empty1", 0.05), ("empty1_tiny", 0.04), ("empty1_warm", 0.04), ("fy1", 0.04), ("alvl0", 0.05)]
FREE_KINDS = [("neg", 0.2), ("zero", 0.15), ("thin", 0.25), ("mid", 0.2), ("thick_free", 0.15), ("empty1_tiny", 0.05)]
STATE = ["aicen_init", "vicen_init", "aicen", "vicen", "vsnon", "trcrn", "aice", "aice0"]
FORCING = ["frain", "frzmlt", "Tf", "sss", "rside", "salinz"]
FLUXES = ["frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn"]
OUT = ["aicen", "vicen", "vsnon", "trcrn", "aice", "aice0"] + FLUXES + ["first_ice"]


def _base(cfg, tcase, ncat):
    """itdvec's quiet state under one of TRACER_CASES (the builder is told where the grid and the table are, as litdvec does for the grid)"""
    saved = dict(itdvec.CONFIGS), dict(itdvec.TRACER_CASES), dict(itdvec.HIN0)
    itdvec.CONFIGS[cfg] = CONFIGS[cfg]
    itdvec.TRACER_CASES[tcase] = TRACER_CASES[tcase]
    itdvec.HIN0[tcase] = HIN0[tcase]
    try:
        return itdvec.itd_input(cfg, tcase, ncat=ncat, tag="therm2", quiet=True)
    finally:
        for dst, src in zip((itdvec.CONFIGS, itdvec.TRACER_CASES, itdvec.HIN0), saved):
            dst.clear()
            dst.update(src)


def _draw(u, kinds):
    edges = np.cumsum([w for _, w in kinds])
    return kinds[min(int(np.searchsorted(edges, u * edges[-1], side="right")), len(kinds) - 1)][0]


def therm2_input(cfg, tcase, ncat=itdvec.NCAT, quiet=False):
    """dict of the arrays and scalars of one step_therm2 call on every block.  quiet: frzmlt <= 0 and rside <= 0 everywhere."""
    x = _base(cfg, tcase, ncat)
    d, tr, k = x["d"], x["tracers"], x["k"]
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    h = lambda q, shape: hash01(shape, seed_of(cfg, "therm2", tcase, str(ncat), q))
    hin = x["hin_max"]
    a, v, s, t = x["aicen"], x["vicen"], x["vsnon"], x["trcrn"]
    for l in range(NILYR):                                                               # bulk salinities, ages, first-year fractions
        t[:, :, tr["nt_sice"] - 1 + l] = 1.0 + 7.0 * h(f"sice{l}", (nb, ncat, ny, nx))
    if tr.get("nt_iage"):
        t[:, :, tr["nt_iage"] - 1] = 3.0e6 * h("iage", (nb, ncat, ny, nx))
    if tr.get("nt_FY"):
        t[:, :, tr["nt_FY"] - 1] = h("FY", (nb, ncat, ny, nx))
    if nb > 1:                                                                          # an ice-free block; its tracers stay as they are
        for q in ("aicen", "vicen", "vsnon"):
            x[q][1] = 0.0
    x.update(SCALARS)
    x["hi_min"] = HI_MIN
    ocean = x["ocean"]
    rhoL = k["rhoi"] * k["Lfresh"] / x["dt"]                                           # frzmlt of vi0new = 1 m (ktherm = 1)
    frzmlt = np.zeros((nb, ny, nx)); rside = np.zeros((nb, ny, nx))
    Tf = -1.9 + 0.2 * h("Tf", (nb, ny, nx))
    sss = np.array(SSS)[np.minimum((h("sss", (nb, ny, nx)) * len(SSS)).astype(np.int64), len(SSS) - 1)]
    frz_onset = np.where(h("onset", (nb, ny, nx)) < 0.5, 0.0, 200.0)
    kinds = np.full((nb, ny, nx), "", dtype=object)
    u, ur = h("kind", (nb, ny, nx)), h("rside", (nb, ny, nx))
    exact = [2.0 ** -(n + 1) for n in range(ncat - 1)] + [2.0 ** -(ncat - 1)]           # areas that sum to exactly 1
    if not quiet:
        for b, j, i in zip(*np.nonzero(ocean)):
            ice = a[b, :, j, i].sum() > 0.0
            kd = _draw(u[b, j, i], ICE_KINDS if ice else FREE_KINDS)
            kinds[b, j, i] = kd
            A, V, S, T = a[b, :, j, i], v[b, :, j, i], s[b, :, j, i], t[b, :, :, j, i]
            if kd in ("full", "full5"):
                for n in range(ncat):
                    A[n] = exact[n]
                    V[n] = A[n] * 0.5 * (hin[n] + min(hin[n + 1], hin[n] + 1.0))
                    S[n] = A[n] * 0.1
                if kd == "full5":
                    A[ncat - 1] -= 5.0e-12
            if kd == "alvl0":
                A[1:] *= 0.5; V[1:] *= 0.5; S[1:] *= 0.5
                A[0] = 0.1; V[0] = 0.1 * 0.3; S[0] = 0.01
                if tr.get("nt_alvl"):
                    T[0, tr["nt_alvl"] - 1] = 0.0
            if kd.startswith("empty1") and ice:
                A[0] = 0.0; V[0] = 0.0; S[0] = 0.0
            if kd == "surplus_empty" and ncat >= 3:
                A[2] = 0.0; V[2] = 0.0; S[2] = 0.0
            if kd == "surplus_tinyv" and ncat >= 4:
                A[3] = 2.0e-11; V[3] = 5.0e-12; S[3] = 0.0
            if kd == "fy1" and tr.get("nt_FY"):
                A[0] = max(A[0], 0.02); V[0] = A[0] * 0.3
                T[0, tr["nt_FY"] - 1] = 1.0
            a0 = max(1.0 - A.sum(), 0.0)
            if kd == "neg":
                frzmlt[b, j, i] = -30.0
            elif kd in ("thin", "empty1", "empty1_warm", "fy1"):
                frzmlt[b, j, i] = 0.008 * a0 * rhoL
            elif kd == "mid":
                frzmlt[b, j, i] = 0.1 * a0 * rhoL
            elif kd in ("surplus", "surplus_empty", "surplus_tinyv", "thick_free"):
                frzmlt[b, j, i] = 2.0 * a0 * rhoL
            elif kd in ("full", "full5"):
                frzmlt[b, j, i] = 0.05 * rhoL
            elif kd == "empty1_tiny":
                frzmlt[b, j, i] = 1.0e-8
            elif kd == "alvl0":
                frzmlt[b, j, i] = 2.0e-10
            if kd == "empty1_warm":
                Tf[b, j, i] = 0.5
            r = ur[b, j, i]
            rside[b, j, i] = 0.0 if r < 0.35 else -0.1 if r < 0.45 else 1.0 if r > 0.92 else (r - 0.45) / 0.47 * 0.6 + 0.01
    x["kinds"] = kinds
    x["aicen_init"] = a.copy()
    grow = 1.0 + 0.2 * (h("grow", (nb, ncat, ny, nx)) - 0.5)
    plainkind = np.isin(kinds, ["neg", "zero", "thin", "mid", "surplus", ""])
    x["vicen_init"] = np.where(plainkind[:, None], v * grow, v)
    aice = np.zeros((nb, ny, nx))
    for n in range(ncat):
        aice = aice + a[:, n]
    x["aice"] = aice                                                                    # aggregate_area's, as linear_itd leaves them
    x["aice0"] = np.maximum(1.0 - aice, 0.0)
    x["frain"] = 1.0e-5 * h("frain", (nb, ny, nx))
    x["frzmlt"], x["Tf"], x["sss"], x["rside"] = frzmlt, Tf, sss, rside
    prof = 2.0 + 1.2 * np.arange(NILYR + 1)                                             # one profile for every cell
    x["salinz"] = np.ascontiguousarray(np.broadcast_to(prof[None, :, None, None], (nb, NILYR + 1, ny, nx)))
    x["frz_onset"] = frz_onset
    x["frazil"] = h("frazil", (nb, ny, nx)) - 0.5                                      # overwritten on ocean cells
    x["meltl"] = h("meltl", (nb, ny, nx)) * 0.01
    for q in STATE + FORCING + FLUXES:
        x[q] = np.ascontiguousarray(x[q], dtype=np.float64)
    return x


def stop_input():
    """g26x18_b8x5, "plain": the cells of itdvec's stop record neg_aicen (an area of -1e-9 in one category, zap_small_areas returns at the
    first one in (n, j, i) order) with no growth and no melt in them, so that the stop is cleanup_itd's"""
    x = therm2_input("g26x18_b8x5", "plain")
    sp = itdvec.STOPS["neg_aicen"]
    for b, i, j in sp["cells"]:
        assert x["ocean"][b - 1, j - 1, i - 1]
        for q in ("aicen", "vicen", "vsnon", "aicen_init", "vicen_init"):
            x[q][b - 1, :, j - 1, i - 1] = 0.0
        n = 1 if (i, j) == (2, 4) else 3
        for q, val in (("aicen", -1.0e-9), ("vicen", 1.0e-9)):
            x[q][b - 1, n, j - 1, i - 1] = val
            x[q + "_init"][b - 1, n, j - 1, i - 1] = val
        for q, val in (("aicen", 0.3), ("vicen", 0.09)):
            x[q][b - 1, 0, j - 1, i - 1] = val
            x[q + "_init"][b - 1, 0, j - 1, i - 1] = val
        x["frzmlt"][b - 1, j - 1, i - 1] = 0.0
        x["rside"][b - 1, j - 1, i - 1] = 0.0
    x["stop_expect"] = (sp["reason"],) + tuple(sp["expect"])
    return x
