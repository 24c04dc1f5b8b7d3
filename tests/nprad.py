"""numpy / Python restatement of the shortwave of ice_step, written from the Fortran in its loop order -- the checker of
evpk_step_radiation and evpk_prep_radiation (tests/test_rad_gpu.py), independent of the HIP code:
  step_radiation   source/ice_step_mod.F90:1364-1524 on its calc_Tsfc / not-dEdd branch: the initialisation of :1408-1423, then
                   shortwave_ccsm3 (source/ice_shortwave.F90:425-646) PER CATEGORY as the reference runs it -- the cell list, Sswabs = 0,
                   compute_albedos (:652-861) or constant_albedos (:867-1011) on block-wide work arrays, absorbed_solar (:1020-1238) --
                   and behind it the albedo lines of coupling_prep (drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586)
  prep_radiation   source/ice_step_mod.F90:33-145

Parity: shortwave_ccsm3 and below are held to reference-built records (tests/golden/ref_sw_c_*.npz, tests/test_shortwave_ref.py: bit for bit
on LIBM); prep_radiation, the call order and the coupling_prep lines are held to the Fortran by reading.

The math functions are parameters: PORTS (npridge.dev_exp and tests/npfmath2.py: the device's bits) or LIBM (math.exp / math.atan).
min / max are a comparison and a select.  Stated departure, shared with the device (include/evpk.h): the cell lists require tmask.
The ocean albedo is the AusCOM build's 2-D ocn_albedo2D or, where that is None, the scalar albocn of the stock build.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), Sswabsn (nb, ncat, nslyr, ny,
nx), Iswabsn (nb, ncat, nilyr, ny, nx), fswpenln (nb, ncat, nilyr + 1, ny, nx) or None.
"""
from __future__ import annotations

import math

import numpy as np

from . import npfmath2 as f2
from .npridge import dev_exp

PUNY = 1.0e-11
C0, C1, C2, C4, P5 = 0.0, 1.0, 2.0, 4.0, 0.5
KAPPAV, TIMELT = 1.4, 0.0                                          # drivers/auscom/ice_constants.F90:82, :65
DT_MELT, DALB_MLT, DALB_MLTV, DALB_MLTI = 1.0, -0.075, -0.1, -0.15  # source/ice_shortwave.F90:709-716
I0VIS = 0.70                                                       # :1079
WARMICE, COLDICE, WARMSNOW, COLDSNOW = 0.68, 0.70, 0.77, 0.81      # :923-927

PORTS = dict(exp=dev_exp, atan=f2.evpk_atan)
LIBM = dict(exp=math.exp, atan=math.atan)

SCALARS = ["albicev", "albicei", "albsnowv", "albsnowi", "ahmax", "snowpatch", "albocn", "awtvdr", "awtidr", "awtvdf", "awtidf"]
OUT3D = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun"]
OUT_LAYERS = ["Sswabsn", "Iswabsn", "fswpenln"]
OUT2D = ["coszen", "alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "scale_factor"]
INFO_KEYS = ["listed", "hs_pos", "hs_zero", "fh_capped", "fh_below", "fT_zero", "fT_neg", "ocn_max_taken", "ocn_max_not", "night", "lit",
             "warm_const", "cold_const"]
PREP_INFO_KEYS = ["aice_zero", "sf_tiny", "scaled", "listed"]


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if b > a else a


def _ocn(p, y, b):
    """the ocean albedo of block b as a plane (ocn_albedo2Da, or albocn on every cell)"""
    if y.get("ocn_albedo2D") is not None:
        return y["ocn_albedo2D"][b]
    return np.full(y["swvdr"][b].shape, p["albocn"])


def compute_albedos(cells, p, y, b, n, ocn, W, M, info, sig):
    atan = M["atan"]
    fhtan = atan(p["ahmax"] * C4)
    for q in ("alvdrni", "alidrni", "alvdfni", "alidfni", "alvdrns", "alidrns", "alvdfns", "alidfns"):
        W[q][:] = ocn
    for q in ("alvdrn", "alidrn", "alvdfn", "alidfn"):
        y[q][b, n] = ocn
    y["albicen"][b, n] = C0
    y["albsnon"][b, n] = C0
    nt_Tsfc = p["tr"]["nt_Tsfc"] - 1
    for (j, i) in cells:
        aicen = float(y["aicen"][b, n, j, i])
        hi = float(y["vicen"][b, n, j, i]) / aicen
        hs = float(y["vsnon"][b, n, j, i]) / aicen
        o = float(ocn[j, i])
        r = atan(hi * C4) / fhtan
        capped = C1 < r
        info["fh_capped" if capped else "fh_below"] += 1
        fh = _min(r, C1)
        albo = o * (C1 - fh)
        avi = p["albicev"] * fh + albo
        aii = p["albicei"] * fh + albo
        dTs = TIMELT - float(y["trcrn"][b, n, nt_Tsfc, j, i])
        r = dTs / DT_MELT - C1
        cold = not (r < C0)
        info["fT_zero" if cold else "fT_neg"] += 1
        fT = _min(r, C0)
        avi = avi - DALB_MLT * fT
        aii = aii - DALB_MLT * fT
        tv, ti = o > avi, o > aii
        info["ocn_max_taken" if (tv or ti) else "ocn_max_not"] += 1
        W["alvdfni"][j, i] = _max(avi, o)
        W["alidfni"][j, i] = _max(aii, o)
        snow = hs > PUNY
        info["hs_pos" if snow else "hs_zero"] += 1
        sig[b, n, j, i] = (capped, cold, tv, ti, snow)
        if snow:
            W["alvdfns"][j, i] = p["albsnowv"]
            W["alidfns"][j, i] = p["albsnowi"]
            W["alvdfns"][j, i] = float(W["alvdfns"][j, i]) - DALB_MLTV * fT
            W["alidfns"][j, i] = float(W["alidfns"][j, i]) - DALB_MLTI * fT
        W["alvdrni"][j, i] = W["alvdfni"][j, i]
        W["alidrni"][j, i] = W["alidfni"][j, i]
        W["alvdrns"][j, i] = W["alvdfns"][j, i]
        W["alidrns"][j, i] = W["alidfns"][j, i]
        asnow = hs / (hs + p["snowpatch"]) if snow else C0
        g = lambda q: float(W[q][j, i])
        y["alvdfn"][b, n, j, i] = g("alvdfni") * (C1 - asnow) + g("alvdfns") * asnow
        y["alidfn"][b, n, j, i] = g("alidfni") * (C1 - asnow) + g("alidfns") * asnow
        y["alvdrn"][b, n, j, i] = g("alvdrni") * (C1 - asnow) + g("alvdrns") * asnow
        y["alidrn"][b, n, j, i] = g("alidrni") * (C1 - asnow) + g("alidrns") * asnow
        y["albicen"][b, n, j, i] = p["awtvdr"] * g("alvdrni") + p["awtidr"] * g("alidrni") + p["awtvdf"] * g("alvdfni") + p["awtidf"] * g("alidfni")
        y["albsnon"][b, n, j, i] = p["awtvdr"] * g("alvdrns") + p["awtidr"] * g("alidrns") + p["awtvdf"] * g("alvdfns") + p["awtidf"] * g("alidfns")


def constant_albedos(cells, p, y, b, n, ocn, W, info, sig):
    for q in ("alvdrn", "alidrn", "alvdfn", "alidfn"):
        y[q][b, n] = ocn
    y["albicen"][b, n] = C0
    y["albsnon"][b, n] = C0
    nt_Tsfc = p["tr"]["nt_Tsfc"] - 1
    for (j, i) in cells:
        hs = float(y["vsnon"][b, n, j, i]) / float(y["aicen"][b, n, j, i])
        warm = float(y["trcrn"][b, n, nt_Tsfc, j, i]) >= -C2 * PUNY
        snow = hs > PUNY
        info["hs_pos" if snow else "hs_zero"] += 1
        info["warm_const" if warm else "cold_const"] += 1
        sig[b, n, j, i] = (warm, snow)
        if snow:
            a = WARMSNOW if warm else COLDSNOW
        else:
            a = WARMICE if warm else COLDICE
        for q in ("alvdfn", "alidfn", "alvdrn", "alidrn"):
            y[q][b, n, j, i] = a
        for q in ("alvdrni", "alidrni", "alvdrns", "alidrns", "alvdfni", "alidfni", "alvdfns", "alidfns"):
            W[q][j, i] = a
        g = lambda q: float(W[q][j, i])
        y["albicen"][b, n, j, i] = p["awtvdr"] * g("alvdrni") + p["awtidr"] * g("alidrni") + p["awtvdf"] * g("alvdfni") + p["awtidf"] * g("alidfni")
        y["albsnon"][b, n, j, i] = p["awtvdr"] * g("alvdrns") + p["awtidr"] * g("alidrns") + p["awtvdf"] * g("alvdfns") + p["awtidf"] * g("alidfns")


def absorbed_solar(cells, p, y, b, n, W, M, info):
    exp = M["exp"]
    nilyr = p["tr"]["nilyr"]
    shape = y["swvdr"][b].shape
    fswpen, trantop, tranbot = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    y["fswsfcn"][b, n] = C0
    y["fswintn"][b, n] = C0
    y["fswthrun"][b, n] = C0
    y["Iswabsn"][b, n] = C0
    pen = y.get("fswpenln")
    for (j, i) in cells:
        aicen = float(y["aicen"][b, n, j, i])
        hs = float(y["vsnon"][b, n, j, i]) / aicen
        asnow = hs / (hs + p["snowpatch"]) if hs > PUNY else C0
        g = lambda q: float(W[q][j, i])
        swvdr, swvdf, swidr, swidf = (float(y[q][b, j, i]) for q in ("swvdr", "swvdf", "swidr", "swidf"))
        info["night" if (swvdr == C0 and swvdf == C0 and swidr == C0 and swidf == C0) else "lit"] += 1
        swabsv = (swvdr * ((C1 - g("alvdrni")) * (C1 - asnow) + (C1 - g("alvdrns")) * asnow)
                  + swvdf * ((C1 - g("alvdfni")) * (C1 - asnow) + (C1 - g("alvdfns")) * asnow))
        swabsi = (swidr * ((C1 - g("alidrni")) * (C1 - asnow) + (C1 - g("alidrns")) * asnow)
                  + swidf * ((C1 - g("alidfni")) * (C1 - asnow) + (C1 - g("alidfns")) * asnow))
        swabs = swabsv + swabsi
        fswpenvdr = swvdr * (C1 - g("alvdrni")) * (C1 - asnow) * I0VIS
        fswpenvdf = swvdf * (C1 - g("alvdfni")) * (C1 - asnow) * I0VIS
        fswpen[j, i] = fswpenvdr + fswpenvdf
        y["fswsfcn"][b, n, j, i] = swabs - float(fswpen[j, i])
        trantop[j, i] = C1
    for k in range(1, nilyr + 1):
        for (j, i) in cells:
            hi = float(y["vicen"][b, n, j, i]) / float(y["aicen"][b, n, j, i])
            hilyr = hi / float(nilyr)
            tranbot[j, i] = exp(-KAPPAV * hilyr * float(k))
            y["Iswabsn"][b, n, k - 1, j, i] = float(fswpen[j, i]) * (float(trantop[j, i]) - float(tranbot[j, i]))
            trantop[j, i] = tranbot[j, i]
            if pen is not None:
                if k == 1:
                    pen[b, n, 0, j, i] = fswpen[j, i]
                pen[b, n, k, j, i] = float(fswpen[j, i]) * float(tranbot[j, i])
    for (j, i) in cells:
        y["fswthrun"][b, n, j, i] = float(fswpen[j, i]) * float(tranbot[j, i])
        y["fswintn"][b, n, j, i] = float(fswpen[j, i]) - float(y["fswthrun"][b, n, j, i])


def step_radiation(blocks, tmask, p, y, M=PORTS):
    """step_radiation and the albedo lines of coupling_prep on every block.  blocks: (ilo, ihi, jlo, jhi) 1-based; p: dict of SCALARS,
    albedo_type ('default' / 'constant') and tr (nt_Tsfc, nilyr, nslyr); y: dict of the arrays, the outputs rewritten in place (fswpenln
    may be None).  Returns (infos per block, sig): sig holds the branches taken per listed (block, category, j, i)"""
    ncat = y["aicen"].shape[1]
    infos, sig = [], {}
    pen = y.get("fswpenln")
    with np.errstate(all="ignore"):
        for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
            info = {k: 0 for k in INFO_KEYS}
            infos.append(info)
            for q in ("alvdrn", "alidrn", "alvdfn", "alidfn", "fswsfcn", "fswintn", "fswthrun", "Iswabsn", "Sswabsn"):      # ice_step_mod.F90:1408-1423
                y[q][b] = C0
            if pen is not None:
                pen[b] = C0
            ocn = _ocn(p, y, b)
            shape = ocn.shape
            W = {q: np.zeros(shape) for q in ("alvdrni", "alidrni", "alvdfni", "alidfni", "alvdrns", "alidrns", "alvdfns", "alidfns")}
            y["coszen"][b] = P5                                                      # ice_shortwave.F90:523
            for n in range(ncat):
                cells = [(j, i) for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi) if tmask[b, j, i] and y["aicen"][b, n, j, i] > PUNY]
                info["listed"] += len(cells)
                y["Sswabsn"][b, n] = C0
                if p.get("albedo_type", "default") == "constant":
                    constant_albedos(cells, p, y, b, n, ocn, W, info, sig)
                else:
                    compute_albedos(cells, p, y, b, n, ocn, W, M, info, sig)
                absorbed_solar(cells, p, y, b, n, W, M, info)
            # coupling_prep (CICE_RunMod.F90:503-548): every cell of the block arrays
            for q in ("alvdf", "alidf", "alvdr", "alidr", "albice", "albsno"):
                y[q][b] = C0
            for n in range(ncat):
                a = y["aicen"][b, n]
                y["alvdf"][b] = y["alvdf"][b] + y["alvdfn"][b, n] * a
                y["alidf"][b] = y["alidf"][b] + y["alidfn"][b, n] * a
                y["alvdr"][b] = y["alvdr"][b] + y["alvdrn"][b, n] * a
                y["alidr"][b] = y["alidr"][b] + y["alidrn"][b, n] * a
                sun = y["coszen"][b] > PUNY
                y["albice"][b] = np.where(sun, y["albice"][b] + y["albicen"][b, n] * a, y["albice"][b])
                y["albsno"][b] = np.where(sun, y["albsno"][b] + y["albsnon"][b, n] * a, y["albsno"][b])
            # :564-567 (the _ai copies are the caller's aliases) and :582-586
            y["scale_factor"][b] = (((y["swvdr"][b] * (C1 - y["alvdr"][b]) + y["swvdf"][b] * (C1 - y["alvdf"][b]))
                                     + y["swidr"][b] * (C1 - y["alidr"][b])) + y["swidf"][b] * (C1 - y["alidf"][b]))
    return infos, sig


def prep_radiation(blocks, tmask, p, y):
    """prep_radiation on every block.  y: aice, aicen, the four sw*, alvdr_ai .. alidf_ai (read), scale_factor, fswfac and the radiation
    arrays (rewritten in place on the cells the reference touches).  Returns the info records per block"""
    ncat = y["aicen"].shape[1]
    tr = p["tr"]
    infos = []
    pen = y.get("fswpenln")
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        info = {k: 0 for k in PREP_INFO_KEYS}
        infos.append(info)
        for j in range(jlo - 1, jhi):
            for i in range(ilo - 1, ihi):
                sf = float(y["scale_factor"][b, j, i])
                g = lambda q: float(y[q][b, j, i])
                if g("aice") > C0 and sf > PUNY:
                    netsw = (g("swvdr") * (C1 - g("alvdr_ai")) + g("swvdf") * (C1 - g("alvdf_ai")) + g("swidr") * (C1 - g("alidr_ai"))
                             + g("swidf") * (C1 - g("alidf_ai")))
                    y["scale_factor"][b, j, i] = netsw / sf
                    info["scaled"] += 1
                else:
                    info["aice_zero"] += int(not g("aice") > C0)
                    info["sf_tiny"] += int(g("aice") > C0 and C0 < sf <= PUNY)
                    y["scale_factor"][b, j, i] = C1
                y["fswfac"][b, j, i] = y["scale_factor"][b, j, i]
        for n in range(ncat):
            for j in range(jlo - 1, jhi):
                for i in range(ilo - 1, ihi):
                    if not (tmask[b, j, i] and y["aicen"][b, n, j, i] > PUNY):
                        continue
                    info["listed"] += 1
                    sf = float(y["scale_factor"][b, j, i])
                    for q in ("fswsfcn", "fswintn", "fswthrun"):
                        y[q][b, n, j, i] = sf * float(y[q][b, n, j, i])
                    if pen is not None:
                        for k in range(tr["nilyr"] + 1):
                            pen[b, n, k, j, i] = sf * float(pen[b, n, k, j, i])
                    for k in range(tr["nslyr"]):
                        y["Sswabsn"][b, n, k, j, i] = sf * float(y["Sswabsn"][b, n, k, j, i])
                    for k in range(tr["nilyr"]):
                        y["Iswabsn"][b, n, k, j, i] = sf * float(y["Iswabsn"][b, n, k, j, i])
    return infos
