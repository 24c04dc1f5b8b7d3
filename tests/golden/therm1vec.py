"""Deterministic inputs of the thermo_vertical tests (tests/nptherm1.py, evpk_thermo_vertical): the grids, land masks, tracer tables and
thickness distributions of tests/golden/therm2vec.py (no shape larger than 26 x 18 cells), so that the result can go straight on into
step_therm2, with a vertical state and a forcing of their own.  A further table, "deep", has nilyr = 7 and nslyr = 2 (the generic kernel):
  Tsfc, qice x 7, qsno x 2, sice x 7

Every ocean cell draws a forcing (2-D: one per cell) and every category with ice in it draws a kind of vertical state, so that a block
mixes them:
  forcing   winter      cold air, little longwave, no shortwave                      a cold surface, bottom growth, one or two iterations
            summer      warm air, shortwave at the surface and inside the ice        a melting surface, top melt, several iterations
            spring      air around the freezing point, some shortwave                surfaces on both sides of 0 C (conditions 1, 2 and 4)
            dry         Qa = 0 over a large lhcoef                                   sublimation, through thin snow into the ice
            humid       moist warm air over a cold surface                           condensation onto snow and onto bare ice
            hotocean    fbot = -2000 W m-2; category 1 is 3 cm thick                 bottom melt; a category that melts away entirely
            steady      a column at Tbot throughout under a surface flux of zero     convergence in one iteration
  state     snow, bare, dusting (2 mm of snow), thinsnow (0.05 mm: below hs_min), deep (snow that pushes the ice below the water line),
            warm (ice within 0.5 K of its melting temperature), coldtop (a warm top layer over cold ice under a surface at 0 C),
            salty (bottom salinity 20 or 36: qbot > qbotmax; 36 puts Tmlts below Tbot, so that the matrix solution exceeds Tmlts), thin (3 cm of ice, category 1), tsn0 (a snow enthalpy a rounding error above
            -rhos Lfresh: the zTsn > 0 reset)
Independently per cell: fsnow = 0 or > 0; mlt_onset and frz_onset 0 or 200.  Block 1 (0-based) of a grid of several blocks is ice-free.
"""
from __future__ import annotations

import numpy as np

from . import itdvec, therm2vec
from .refvec import hash01, seed_of
from ..npridge import dev_exp

CONFIGS = therm2vec.CONFIGS
PUNY = itdvec.PUNY
_DEEP = dict(nt_Tsfc=1, nt_qice=2, nilyr=7, nt_qsno=9, nslyr=2, nt_sice=11)
TRACER_CASES = dict(therm2vec.TRACER_CASES, deep=([0] + [1] * 7 + [2] * 2 + [1] * 7, _DEEP))
HIN0 = dict(therm2vec.HIN0, deep=0.0)
CP_OCN, DEPRESST = 4218.0, 0.054
TFFRESH, TTTICE, QQQICE, STEFAN = 273.15, 5897.8, 11637800.0, 567.0e-10
SCALARS = dict(yday=123.0, min_salin=0.1, rhow=1026.0)
FORCINGS = [("winter", 0.26), ("summer", 0.22), ("spring", 0.2), ("dry", 0.08), ("humid", 0.1), ("hotocean", 0.08), ("steady", 0.06)]
KINDS = [("snow", 0.25), ("sunlit", 0.05), ("bare", 0.16), ("dusting", 0.1), ("thinsnow", 0.06), ("deep", 0.07), ("warm", 0.1), ("coldtop", 0.07), ("salty", 0.06),
         ("thin", 0.04), ("tsn0", 0.04)]
STATE = ["aicen", "vicen", "vsnon", "trcrn"]
IN2D = ["flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "sss"]
IN3D = ["shcoef", "lhcoef"]
INOUT3D = ["fswsfcn", "fswintn", "Sswabsn", "Iswabsn"]
INOUT2D = ["fpond", "mlt_onset", "frz_onset"]
OUT15 = ["flwoutn", "evapn", "freshn", "fsaltn", "fhocnn", "fsensn", "flatn", "fsurfn", "fcondtopn", "melttn", "meltsn", "meltbn", "congeln",
         "snoicen", "dsnown"]
WRITTEN = STATE + INOUT3D + INOUT2D + OUT15


def _base(cfg, tcase, ncat):
    """therm2vec's input under one of TRACER_CASES (the builder is told where the table is, as therm2vec tells itdvec)"""
    saved = dict(therm2vec.TRACER_CASES), dict(therm2vec.HIN0)
    therm2vec.TRACER_CASES[tcase] = TRACER_CASES[tcase]
    therm2vec.HIN0[tcase] = HIN0[tcase]
    try:
        return therm2vec.therm2_input(cfg, tcase, ncat=ncat)
    finally:
        for dst, src in zip((therm2vec.TRACER_CASES, therm2vec.HIN0), saved):
            dst.clear()
            dst.update(src)


def _draw(u, kinds):
    edges = np.cumsum([w for _, w in kinds])
    return kinds[min(int(np.searchsorted(edges, u * edges[-1], side="right")), len(kinds) - 1)][0]


def qice_of(T, S, k):
    """the BL99 enthalpy of ice at temperature T < Tmlt = -depressT S (ice_therm_bl99.F90:748-750)"""
    Tm = -S * DEPRESST
    return -k["rhoi"] * (k["cp_ice"] * (Tm - T) + k["Lfresh"] * (1.0 - Tm / T) - CP_OCN * Tm)


def therm1_input(cfg, tcase, ncat=itdvec.NCAT):
    """dict of the arrays and scalars of one evpk_thermo_vertical call on every block; it keeps therm2vec's forcing for the step_therm2
    that may follow (aicen_init / vicen_init are the state of entry, as step_therm1 saves them)"""
    x = _base(cfg, tcase, ncat)
    d, tr, k = x["d"], x["tracers"], x["k"]
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    nilyr, nslyr = tr["nilyr"], tr["nslyr"]
    h = lambda q, shape: hash01(shape, seed_of(cfg, "therm1", tcase, str(ncat), q))
    a, v, s, t = x["aicen"], x["vicen"], x["vsnon"], x["trcrn"]
    ocean = x["ocean"]
    s2, s3 = (nb, ny, nx), (nb, ncat, ny, nx)
    uf, uk = h("forcing", s2), h("kind", s3)
    r2 = {q: h(q, s2) for q in ("potT", "flw", "Qa", "fbot", "sw", "fsnow", "onm", "onf", "pond")}
    r3 = {q: h(q, s3) for q in ("hs", "Ttop", "S", "sh", "lh", "swf", "Tsfc")}
    rl = h("layers", (nb, ncat, nilyr, ny, nx))
    f = {q: np.zeros(s2) for q in IN2D}
    f["rhoa"][:] = 1.3
    f["Tbot"][:] = -1.8
    f["sss"][:] = x["sss"]
    f["fbot"][:] = -2.0
    for q in IN3D + ["fswsfcn", "fswintn"]:
        f[q] = np.zeros(s3)
    f["Sswabsn"] = np.zeros((nb, ncat, nslyr, ny, nx))
    f["Iswabsn"] = np.zeros((nb, ncat, nilyr, ny, nx))
    forcing = np.full(s2, "", dtype=object)
    kinds = np.full(s3, "", dtype=object)
    for b, j, i in zip(*np.nonzero(ocean)):
        fk = _draw(uf[b, j, i], FORCINGS)
        forcing[b, j, i] = fk
        u = {q: r2[q][b, j, i] for q in r2}
        sw = 0.0
        if fk == "winter":
            potT, flw, Qa = 243.0 + 20.0 * u["potT"], 150.0 + 70.0 * u["flw"], 3.0e-4 + 7.0e-4 * u["Qa"]
        elif fk == "summer":
            potT, flw, Qa, sw = 272.0 + 6.0 * u["potT"], 280.0 + 50.0 * u["flw"], 3.0e-3 + 1.0e-3 * u["Qa"], 40.0 + 110.0 * u["sw"]
            f["fbot"][b, j, i] = -5.0 - 35.0 * u["fbot"]
        elif fk == "spring":
            potT, flw, Qa, sw = 267.0 + 6.0 * u["potT"], 230.0 + 70.0 * u["flw"], 2.0e-3 + 1.0e-3 * u["Qa"], 60.0 * u["sw"]
        elif fk == "dry":
            potT, flw, Qa, sw = 262.0 + 8.0 * u["potT"], 220.0 + 40.0 * u["flw"], 0.0, 30.0 * u["sw"]
        elif fk == "humid":
            potT, flw, Qa = 273.5 + 2.0 * u["potT"], 300.0 + 20.0 * u["flw"], 5.0e-3 + 2.0e-3 * u["Qa"]
        elif fk == "steady":                   # fsurfn(Tsf = Tbot) = 0 up to rounding: potT = TsfK, Qa = Qsfc, flw = sigma TsfK**4
            TsfK = -1.8 + TFFRESH
            potT, flw, Qa = TsfK, STEFAN * ((TsfK * TsfK) * (TsfK * TsfK)), QQQICE * dev_exp(-TTTICE * (1.0 / TsfK)) / 1.3
        else:
            potT, flw, Qa = 255.0 + 15.0 * u["potT"], 200.0 + 60.0 * u["flw"], 1.0e-3
            f["fbot"][b, j, i] = -2000.0
        f["potT"][b, j, i], f["flw"][b, j, i], f["Qa"][b, j, i] = potT, flw, Qa
        f["fsnow"][b, j, i] = 0.0 if u["fsnow"] < 0.5 else 4.0e-5 * u["fsnow"]
        warm_air = fk in ("summer", "spring")
        for n in range(ncat):
            if not a[b, n, j, i] > 0.0:
                continue
            w = {q: r3[q][b, n, j, i] for q in r3}
            kd = _draw(uk[b, n, j, i], KINDS)
            hi = v[b, n, j, i] / a[b, n, j, i]
            if fk == "hotocean" and n == 0:
                kd = "thin"
            if kd == "thin" and n > 0:
                kd = "snow"
            if kd == "deep" and hi > 1.2:
                kd = "snow"
            kinds[b, n, j, i] = kd
            if kd == "thin":
                hi = 0.03
                v[b, n, j, i] = a[b, n, j, i] * hi
            hs = {"bare": 0.0, "warm": 0.0, "sunlit": 0.0, "coldtop": 0.0, "dusting": 0.002, "thinsnow": 0.5e-4, "deep": 0.45 * hi + 0.2, "thin": 0.0}.get(
                kd, 0.05 + 0.35 * w["hs"])
            s[b, n, j, i] = a[b, n, j, i] * hs
            S = 1.0 + 5.0 * w["S"] + 2.0 * (np.arange(nilyr) + 0.5) / nilyr
            if kd == "salty":
                S[nilyr - 1] = 20.0 if (w["S"] < 0.5 or fk == "steady") else 36.0     # (36: Tmlts below Tbot, the ocean warms the layer past it)
            Tm = -S * DEPRESST
            if warm_air or fk == "humid" and kd == "warm":
                Ttop = -0.4 - 2.5 * w["Ttop"]
            else:
                Ttop = -5.0 - 20.0 * w["Ttop"]
            if kd in ("warm", "sunlit"):
                T = Tm - 0.005 - 0.1 * rl[b, n, :, j, i]
            else:
                T = Ttop + (-1.9 - Ttop) * (np.arange(nilyr) + 0.5) / nilyr
                T = np.minimum(T, Tm - 0.05)
            if kd == "coldtop":
                T[:] = -12.0
                T[0] = min(-0.5, Tm[0] - 0.05)
            Tsfc = 0.0 if (kd == "coldtop" or (warm_air and w["Tsfc"] < 0.5)) else min(T[0] - 1.0 * w["Tsfc"], -0.05)
            if fk == "humid":
                Tsfc = min(Tsfc, -3.0)
            if fk == "steady":
                T[:] = -1.8
                Tsfc = -1.8
            t[b, n, tr["nt_Tsfc"] - 1, j, i] = Tsfc
            for l in range(nilyr):
                t[b, n, tr["nt_sice"] - 1 + l, j, i] = S[l]
                t[b, n, tr["nt_qice"] - 1 + l, j, i] = qice_of(T[l], S[l], k)
            Tsn = min(0.5 * (Tsfc + T[0]), 0.0)
            for l in range(nslyr):
                t[b, n, tr["nt_qsno"] - 1 + l, j, i] = -k["rhos"] * (k["Lfresh"] - k["cp_ice"] * Tsn)
                if kd == "tsn0":
                    t[b, n, tr["nt_qsno"] - 1 + l, j, i] = -k["rhos"] * k["Lfresh"] * (1.0 - 1.0e-13)
            f["shcoef"][b, n, j, i] = 8.5 * (0.5 + w["sh"])
            f["lhcoef"][b, n, j, i] = 2.4e4 * (0.5 + w["lh"]) * (3.0 if fk == "dry" else 1.0)
            if kd == "sunlit":                   # more shortwave inside the ice than takes a layer to its melting temperature
                per = 4000.0 * (hi / nilyr) * (0.5 + rl[b, n, :, j, i])
                f["Iswabsn"][b, n, :, j, i] = per
                f["fswintn"][b, n, j, i] = per.sum()
                f["fswsfcn"][b, n, j, i] = 20.0
            elif sw > 0.0:
                f["fswsfcn"][b, n, j, i] = sw * (0.4 + 0.3 * w["swf"])
                inside = sw * (0.1 + 0.3 * w["swf"])
                frac_snow = 0.3 if hs > 1.0e-3 else 0.0
                f["fswintn"][b, n, j, i] = inside
                wl = 0.5 ** np.arange(nilyr)
                f["Iswabsn"][b, n, :, j, i] = inside * (1.0 - frac_snow) * wl / wl.sum()
                f["Sswabsn"][b, n, :, j, i] = inside * frac_snow / nslyr
    x.update(f)
    x.update(SCALARS)
    x["forcing_kinds"], x["state_kinds"] = forcing, kinds
    x["mlt_onset"] = np.where(r2["onm"] < 0.5, 0.0, 200.0)
    x["frz_onset"] = np.where(r2["onf"] < 0.5, 0.0, 200.0)
    x["fpond"] = r2["pond"] - 0.5
    for q in OUT15:                                                                     # overwritten on every cell
        x[q] = h("out" + q, s3) - 0.5
    x["aicen_init"], x["vicen_init"] = a.copy(), v.copy()                               # for the step_therm2 that follows
    aice = np.zeros(s2)
    for n in range(ncat):
        aice = aice + a[:, n]
    x["aice"], x["aice0"] = aice, np.maximum(1.0 - aice, 0.0)
    for q in STATE + IN2D + IN3D + INOUT3D + INOUT2D + OUT15:
        x[q] = np.ascontiguousarray(x[q], dtype=np.float64)
    return x


# one crafted tracer value per stop reason that an input can reach: (tracer, layer (0-based), value).  Reason 4 (zTin > Tmlts) cannot be
# reached: zTin = min(root, Tmlts).  Reason 6: an enthalpy above that of the layer's melting temperature -- zTin = Tmlts passes every check
# of init_vertical_profile, but einit holds an energy no temperature reproduces, so condition 5 fails in all nitermax iterations.
STOPS = {1: ("nt_qsno", 0, lambda k: -k["rhos"] * k["Lfresh"] * 0.9),
         2: ("nt_qsno", 0, lambda k: -k["rhos"] * (k["Lfresh"] + k["cp_ice"] * 150.0)),
         3: ("nt_sice", 2, lambda k: 0.05),
         5: ("nt_qice", 1, lambda k: -k["rhoi"] * (k["cp_ice"] * 150.0 + k["Lfresh"])),
         6: ("nt_qice", 1, lambda k: -1.0e5)}


def _usable(x, snow):
    ok = (x["aicen"] > PUNY) & x["ocean"][:, None]
    if snow:
        ok = ok & (x["vsnon"] / np.where(x["aicen"] > 0.0, x["aicen"], 1.0) > 0.01)
    return ok


def _four_places(ok):
    """(b, n, j, i) 0-based, the first of which the reference meets first, chosen so that every level of the order decides once:
      0  block B, category n_lo, row j1, a large i                the winner
      1  block B, category n_lo, a later row, a smaller i          j outer / i inner
      2  block B, a higher category, a cell before the winner's    the category comes before the cell
      3  a higher block, a lower category                          the block comes before the category"""
    nb, ncat = ok.shape[:2]
    for b in range(nb - 1):
        for nlo in range(1, ncat - 1):
            cells = np.argwhere(ok[b, nlo])
            for j1, i1 in cells:
                later = [(j, i) for j, i in cells if j > j1 and i < i1]
                before = [(n, j, i) for n in range(nlo + 1, ncat) for j, i in np.argwhere(ok[b, n]) if (j, i) < (j1, i1)]
                above = [(bb, n, j, i) for bb in range(b + 1, nb) for n in range(nlo) for j, i in np.argwhere(ok[bb, n])[:1]]
                if later and before and above:
                    return [(b, nlo, j1, i1), (b, nlo) + tuple(later[0]), (b,) + tuple(before[0]), tuple(above[0])]
    raise AssertionError("no four places")


def stop_input(reason, cfg="g26x18_b8x5", tcase="plain"):
    """the crafted value in the four places of _four_places; stop_places[0] is the one the reference meets first"""
    x = therm1_input(cfg, tcase)
    name, layer, val = STOPS[reason]
    tr, k = x["tracers"], x["k"]
    picks = _four_places(_usable(x, name == "nt_qsno"))
    for b, n, j, i in picks:
        x["trcrn"][b, n, tr[name] - 1 + layer, j, i] = val(k)
    x["stop_places"] = [(int(b) + 1, int(n) + 1, int(i) + 1, int(j) + 1) for b, n, j, i in picks]
    return x


# two reasons in one block and category, the later check of the reference's sequence in the EARLIER cell: the sequence comes before the cell
#   snow   reason 2 (zTsn < Tmin) in the earlier cell, reason 1 (zTsn > Tmax) in the later one: the reference meets reason 1
#   ice    reason 3 in ice layer 3 in the earlier cell, reason 5 in ice layer 2 in the later one: the reference meets reason 5
#   late   reason 6 (no convergence) in the earlier cell, reason 5 in the later one: the reference meets reason 5
MIXED = {"snow": (2, 1), "ice": (3, 5), "late": (6, 5)}


def stop_mixed_input(kind, cfg="g26x18_b8x5", tcase="plain"):
    x = therm1_input(cfg, tcase)
    tr, k = x["tracers"], x["k"]
    early, late = MIXED[kind]
    ok = _usable(x, kind == "snow")
    for b, n in np.argwhere(ok.sum(axis=(2, 3)) >= 2):
        cells = np.argwhere(ok[b, n])
        (j0, i0), (j1, i1) = cells[0], cells[-1]
        break
    for reason, (j, i) in ((early, (j0, i0)), (late, (j1, i1))):
        name, layer, val = STOPS[reason]
        x["trcrn"][b, n, tr[name] - 1 + layer, j, i] = val(k)
    x["stop_expect"] = (late, int(b) + 1, int(n) + 1, int(i1) + 1, int(j1) + 1)
    return x
