"""Deterministic inputs of the step_therm1 tests (tests/nptherm1s.py, evpk_step_therm1): the grids, masks, tracer tables and vertical
states of tests/golden/therm1vec.py (no shape larger than 26 x 18 cells), so that the result can go straight on into step_therm2, with
the further forcing of step_therm1 drawn per ocean cell so that a block mixes:
  frzmlt    therm2vec's where it is positive; where it is zero or negative a melting potential of its own, -5 .. -400 W m-2
  melt      per cell with frzmlt < 0 one of
            small      sst - Tf of 0.02 .. 0.2 K under a large |frzmlt|: fbot is the cpchr product, the xtmp limit does not act
            large      sst - Tf of 1 .. 3 K: fbot is clamped by frzmlt, the xtmp limit acts
            zero       sst = Tf exactly: deltaT = 0, pow of zero
            boiling    sst = Tf + 1500: rside clamped at 1 (no ocean is like that; the clamp has to be reached)
  strocn    1e-6 .. 0.3 N m-2: ustar below and above ustar_min = 0.005
  wind      0.3 .. 15 m/s (below and above 1 m/s), uatm / vatm a direction of their own
  zlvl      10 (= zref), 2.5, 20 or 40 m
  lmask     north, south or neither, by cell
therm1vec's potT, Qa and Tsfc give stable and unstable air (|hol| below the clamp at high wind, at it at low wind) and delq of both signs.
fswthrun is non-zero where there is shortwave; Cdn_atm and merge_fluxes' 22 cumulative planes are pre-filled with non-zero values.
The tables that carry iage and FY ("plain", "cesm_ponds") get tr_iage = tr_FY = 1.
"""
from __future__ import annotations

import numpy as np

from . import therm1vec
from .refvec import hash01, seed_of

CONFIGS = therm1vec.CONFIGS
PUNY = therm1vec.PUNY
TABLES = ["plain", "cesm_ponds"]                     # the tracer tables that carry iage and FY (lvl and topo ponds are refused)
SCALARS = dict(chio=0.006, ustar_min=0.005, natmiter=5, calc_strair=1, pndaspect=0.8, rfracmin=0.15, rfracmax=1.0)
MELTS = [("small", 0.35), ("large", 0.35), ("zero", 0.15), ("boiling", 0.15)]
ZLVLS = [10.0, 2.5, 20.0, 40.0]
IN2D = ["aice", "frzmlt", "sst", "Tf", "strocnxT", "strocnyT", "uatm", "vatm", "wind", "zlvl", "frain"]
MERGED = ["strairxT", "strairyT", "Cdn_atm_ratio", "fsurf", "fcondtop", "fsens", "flat", "fswabs", "flwout", "evap", "Tref", "Qref", "Uref",
          "fresh", "fsalt", "fhocn", "fswthru", "meltt", "meltb", "melts", "congel", "snoice"]
PERCAT8 = ["shcoef", "lhcoef", "strairxn", "strairyn", "Cdn_atm_ratio_n", "Trefn", "Qrefn", "Urefn"]
OUT2D = ["rside", "fbot", "Tbot", "aice_init"]
OUT3D = ["aicen_init", "vicen_init"] + PERCAT8
INOUT2D = ["Cdn_atm"] + MERGED
WRITTEN = therm1vec.WRITTEN + OUT2D + OUT3D + INOUT2D


def therm1s_input(cfg, tcase, ncat=5):
    """dict of the arrays and scalars of one evpk_step_therm1 call on every block (therm1vec's, with shcoef, lhcoef, fbot, Tbot and rside
    turned into outputs)"""
    x = therm1vec.therm1_input(cfg, tcase, ncat=ncat)
    d, tr = x["d"], dict(x["tracers"])
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    s2, s3 = (nb, ny, nx), (nb, ncat, ny, nx)
    h = lambda q, shape: hash01(shape, seed_of(cfg, "therm1s", tcase, str(ncat), q))
    tr["tr_iage"], tr["tr_FY"] = int(bool(tr.get("nt_iage"))), int(bool(tr.get("nt_FY")))
    x["tracers"] = tr
    ocean = x["ocean"]
    u = {q: h(q, s2) for q in ("melt", "frz", "dT", "tau", "taudir", "wind", "winddir", "zlvl", "lmask", "Tf")}
    frzmlt = x["frzmlt"].copy()
    sst = x["Tf"] + 0.5 * u["dT"]
    melts = np.full(s2, "", dtype=object)
    for b, j, i in zip(*np.nonzero(ocean)):
        if frzmlt[b, j, i] > 0.0:
            continue
        kd = therm1vec._draw(u["melt"][b, j, i], MELTS)
        melts[b, j, i] = kd
        Tf = x["Tf"][b, j, i]
        if kd == "small":
            frzmlt[b, j, i] = -150.0 - 250.0 * u["frz"][b, j, i]
            sst[b, j, i] = Tf + 0.02 + 0.18 * u["dT"][b, j, i]
        elif kd == "large":
            frzmlt[b, j, i] = -5.0 - 45.0 * u["frz"][b, j, i]
            sst[b, j, i] = Tf + 1.0 + 2.0 * u["dT"][b, j, i]
        elif kd == "zero":
            frzmlt[b, j, i] = -20.0 - 100.0 * u["frz"][b, j, i]
            sst[b, j, i] = Tf
        else:
            frzmlt[b, j, i] = -50.0 - 300.0 * u["frz"][b, j, i]
            sst[b, j, i] = Tf + 1500.0
    tau = 10.0 ** (-6.0 + 5.5 * u["tau"])
    wind = np.where(u["wind"] < 0.25, 0.3 + 2.8 * u["wind"], 1.0 + 14.0 * (u["wind"] - 0.25) / 0.75)
    x.update(frzmlt=frzmlt, sst=sst, melt_kinds=melts,
             strocnxT=tau * np.cos(6.283 * u["taudir"]), strocnyT=tau * np.sin(6.283 * u["taudir"]),
             wind=wind, uatm=wind * np.cos(6.283 * u["winddir"]), vatm=0.9 * wind * np.sin(6.283 * u["winddir"]),
             zlvl=np.asarray(ZLVLS)[np.minimum((u["zlvl"] * 4).astype(int), 3)])
    x["lmask_n"] = np.ascontiguousarray(u["lmask"] < 0.4, dtype=np.int32)
    x["lmask_s"] = np.ascontiguousarray((u["lmask"] >= 0.4) & (u["lmask"] < 0.8), dtype=np.int32)
    sw = (x["fswsfcn"] > 0.0) | (x["fswintn"] > 0.0)
    x["fswthrun"] = np.where(sw, 0.5 + 6.0 * h("fswthrun", s3), 0.0)
    x["Cdn_atm"] = 1.0e-3 * (0.5 + h("Cdn_atm", s2))
    for q in MERGED:
        x[q] = h("m" + q, s2) - 0.37
    for q in OUT2D:
        x[q] = h("o" + q, s2) - 0.5
    for q in OUT3D:
        x[q] = h("o" + q, s3) - 0.5
    x.update(SCALARS)
    for q in IN2D + ["fswthrun"] + INOUT2D + OUT2D + OUT3D:
        x[q] = np.ascontiguousarray(x[q], dtype=np.float64)
    return x


def stop_input(reason=6, cfg="g26x18_b8x5", tcase="plain"):
    """therm1vec's crafted stop (one tracer value in four places) under the forcing of step_therm1"""
    x = therm1s_input(cfg, tcase)
    s = therm1vec.stop_input(reason, cfg, tcase)
    x["trcrn"] = s["trcrn"]
    x["stop_places"] = s["stop_places"]
    return x
