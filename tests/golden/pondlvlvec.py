"""Deterministic inputs of the level-ice pond tests (tests/nppondlvl.py, evpk_step_therm1_lvl, evpk_step_radiation_dedd_lvl): the grids,
masks, state and forcing of tests/golden/deddvec.py -- which are those of tests/golden/therm1svec.py under a shortwave forcing, so one
input serves both calls and the chain of them (no shape larger than 26 x 18 cells; two blocks at least, the second ice-free) -- with the
tables "plain" (nilyr 4, nslyr 1, ncat 5: the fixed instantiations) and "deep" (7, 2, ncat 3: the generic ones), five tracer planes behind
the table's own
  apnd, hpnd   deddvec's planes: none; 0.1 .. 0.5 of the level ice with hpnd 1 .. 4 mm, 1 .. 19 cm or 25 .. 60 cm; and, drawn here, "film"
               (hpnd 1e-6 .. 2e-5 m: drained completely by a permeable column) and "speck" (apnd 1e-9 .. 1e-8: apondn aicen > puny, but any
               loss of volume takes the area below puny)
  alvl, vlvl   0.3 .. 1 of the category; one column in twelve has alvl aicen = 5e-11 (above puny**2, below 10 puny: melt water runs off)
  ipnd         no lid; 1 .. 10 mm (thinner than an hour's Stefan growth from open water at -10 C); 5 .. 30 cm
and draws of their own:
  aicen        one column with ice in sixteen is scaled, with vicen and vsnon, to aicen = 5e-12: listed by compute_ponds_lvl (aicen alvl >
               puny**2), not by the thermodynamics nor by the shortwave (aicen <= puny); aice and aice0 are summed again
  frain        zero on half of the cells: with no melt dvn == 0 exactly, the lid grows
  Tair         potT on three cells in five (cold under winter forcing); 273.15 .. 276 K on the rest (Ts >= 0)
  fsnow        therm1vec's, the one field both calls read: zero on half of the cells, else up to 4e-5 kg m-2 s-1 (fsnow dt > hs_min)
  dhsn         0; hs exactly (the pond ice is snow-free though the sea ice is not); 0.2 .. 0.8 hs; 0.05 m over bare ice (reset)
  ffracn       0, 1, or a draw strictly between
  hpnd         on up to EDGE_COLUMNS snow-covered ponded columns per input with ffracn = 0 and dhsn = 0: the depth at which rp = rhofresh hp /
               (rhofresh hp + rhos hs) comes out EXACTLY p15 in double precision, so that the strict comparison rp < p15 of run_dEdd's
               level-ice block (source/ice_shortwave.F90:1493) decides them ("p15_edge")
The shortwave's outputs are deddvec's non-zero pre-fills: a test that calls the thermodynamics alone takes fswsfcn, fswintn, fswthrun,
Sswabsn and Iswabsn (CARRIED) from a shortwave call on the same input, as a time step does.
"""
from __future__ import annotations

import numpy as np

from . import deddvec
from .refvec import hash01, seed_of

CONFIGS = deddvec.CONFIGS
PUNY = deddvec.PUNY
TABLES = {"plain": 5, "deep": 3}                                  # table -> ncat
FRZPND = ["cesm", "hlid"]
DPSCALES = [0.0, 1.0e-3, 1.0]                                     # off; the shipped ice_in's; the default of source/ice_init.F90:300
NAMELIST = dict(hs1=0.03)                                         # source/ice_init.F90:299
PLANES = ["apnd", "hpnd", "alvl", "vlvl", "ipnd"]                 # behind the table's own tracers, in this order
POND_ARRAYS = ["dhsn", "ffracn", "Tair", "fsnow"]
CARRIED = ["fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn"]
LID = [("none", 0.4), ("thin", 0.25), ("thick", 0.35)]
DHS = [("zero", 0.45), ("all", 0.2), ("part", 0.2), ("stale", 0.15)]
FFRAC = [("zero", 0.5), ("one", 0.2), ("mid", 0.3)]
EDGE_COLUMNS = 12
RHOFRESH, P15 = 1000.0, 0.15                                      # drivers/auscom/ice_constants.F90:56, :139 of drivers/cice's


def _hp_at_p15(hs, rhos):
    """the pond depth hp for which rhofresh hp / (rhofresh hp + rhos hs) rounds to exactly p15, or None if no double does"""
    hp = np.float64(P15 * rhos * hs / ((1.0 - P15) * RHOFRESH))
    for _ in range(64):
        rp = (RHOFRESH * hp) / (RHOFRESH * hp + rhos * hs)
        if rp == P15:
            return float(hp)
        hp = np.nextafter(hp, np.inf if rp < P15 else -np.inf)
    return None


def pondlvl_input(cfg, tcase):
    """dict of the arrays and scalars of one evpk_step_radiation_dedd_lvl call and one evpk_step_therm1_lvl call on every block"""
    ncat = TABLES[tcase]
    x = deddvec.dedd_input(cfg, tcase, "cesm", ncat=ncat)
    d, tr = x["d"], dict(x["tracers"])
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    s2, s3 = (nb, ny, nx), (nb, ncat, ny, nx)
    h = lambda q, shape: hash01(shape, seed_of(cfg, "pondlvl", tcase, q))
    kind = deddvec._kind
    # the tiny-area columns
    a, v, s = x["aicen"], x["vicen"], x["vsnon"]
    tiny = (a > 0.0) & (h("tiny", s3) < 1.0 / 16.0)
    f = np.where(tiny, 5.0e-12 / np.where(a > 0.0, a, 1.0), 1.0)
    x["aicen"] = np.ascontiguousarray(np.where(tiny, 5.0e-12, a))
    x["vicen"], x["vsnon"] = np.ascontiguousarray(v * f), np.ascontiguousarray(s * f)
    x["tiny_area"] = tiny
    a = x["aicen"]
    aice = np.zeros(s2)
    for n in range(ncat):
        aice = aice + a[:, n]
    x["aice"], x["aice0"] = aice, np.maximum(1.0 - aice, 0.0)
    ice = a > 0.0
    safe = np.where(ice, a, 1.0)
    hs = x["vsnon"] / safe
    # tracer planes: deddvec put apnd, hpnd behind the table's own; alvl, vlvl, ipnd follow
    t0 = x["trcrn"]
    n0 = t0.shape[2] - 2
    t = np.zeros((nb, ncat, n0 + 5, ny, nx))
    t[:, :, :n0 + 2] = t0
    pk = x["pond_kinds"].copy()
    u = h("pondkind2", s3)
    pk[(pk != "none") & (u < 0.12)] = "film"
    pk[(pk != "none") & (u >= 0.12) & (u < 0.24)] = "speck"
    x["pond_kinds"] = pk
    t[:, :, n0] = np.where(pk == "speck", 1.0e-9 + 9.0e-9 * h("speck", s3), t[:, :, n0])
    t[:, :, n0 + 1] = np.where(pk == "film", 1.0e-6 + 1.9e-5 * h("film", s3), t[:, :, n0 + 1])
    alvl = 0.3 + 0.7 * h("alvl", s3)
    deformed = h("deformed", s3) < 1.0 / 12.0
    alvl = np.where(deformed, 5.0e-11 / safe, alvl)
    lk = kind(h("lidkind", s3), LID)
    ul = h("ipnd", s3)
    ipnd = np.where(lk == "thin", 0.001 + 0.009 * ul, np.where(lk == "thick", 0.05 + 0.25 * ul, 0.0))
    for k, plane in ((n0, t[:, :, n0]), (n0 + 1, t[:, :, n0 + 1]), (n0 + 2, alvl), (n0 + 3, alvl * (0.8 + 0.4 * h("vlvl", s3))), (n0 + 4, ipnd)):
        t[:, :, k] = np.where(ice, plane, 0.0)
    x["trcrn"] = np.ascontiguousarray(t)
    x["lid_kinds"], x["deformed"] = lk, deformed
    tr.update(tr_pond_cesm=0, tr_pond_lvl=1, tr_pond_topo=0, nt_apnd=n0 + 1, nt_hpnd=n0 + 2, nt_alvl=n0 + 3, nt_vlvl=n0 + 4, nt_ipnd=n0 + 5)
    x["tracers"] = tr
    x["ntrcr"] = n0 + 5
    # forcing and the two arrays the calls hand each other
    x["frain"] = np.ascontiguousarray(np.where(h("norain", s2) < 0.5, 0.0, x["frain"]))
    x["Tair"] = np.ascontiguousarray(np.where(h("Tairkind", s2) < 0.6, x["potT"], 273.15 + 2.85 * h("Tair", s2)))
    dk = kind(h("dhskind", s3), DHS)
    dhs = np.where(dk == "all", hs, np.where(dk == "part", (0.2 + 0.6 * h("dhs", s3)) * hs, np.where(dk == "stale", 0.05, 0.0)))
    x["dhsn"] = np.ascontiguousarray(np.where(ice, dhs, 0.0))
    fk = kind(h("ffrackind", s3), FFRAC)
    x["ffracn"] = np.ascontiguousarray(np.where(fk == "one", 1.0, np.where(fk == "mid", 0.02 + 0.96 * h("ffracn", s3), 0.0)))
    x["dhs_kinds"], x["ffrac_kinds"] = dk, fk
    # the columns on the edge of rp < p15: ponded (not a speck), under at least 1 mm of snow, nothing else hiding the pond
    edge = np.zeros(s3, dtype=bool)
    t = x["trcrn"]
    cand = x["ocean"][:, None] & (a > PUNY) & ~tiny & (hs >= 1.0e-3) & np.isin(pk, ("shallow", "trans", "deep")) & (fk == "zero") & (dk == "zero")
    for b, n, j, i in zip(*np.nonzero(cand)):
        if edge.sum() == EDGE_COLUMNS:
            break
        hp = _hp_at_p15(float(x["vsnon"][b, n, j, i]) / float(a[b, n, j, i]), x["k"]["rhos"])
        if hp is not None:
            t[b, n, n0 + 1, j, i] = hp
            edge[b, n, j, i] = True
    x["p15_edge"] = edge
    x.update(NAMELIST)
    return x
