"""numpy / Python restatement of step_therm1 (source/ice_step_mod.F90:154-733) written from the Fortran in its loop order -- the checker of
evpk_step_therm1 (tests/test_therm1s_gpu.py), independent of the HIP code:
  per block: aice_init / aicen_init / vicen_init (:272-285); frzmlt_bottom_lateral (source/ice_therm_vertical.F90:611-834, AusCOM branch
  cpchr = -cp_ocn rhow chio); then PER CATEGORY, as the reference runs them: the cell list (:378-389), atmo_boundary_layer
  (source/ice_atmo.F90:82-483; 'ice', highfreq and formdrag .false.), the AusCOM strairxn = strairyn = 0 without calc_strair (:458-464),
  increment_age, update_FYarea, thermo_vertical (tests/nptherm1.py), fswabsn (:565-571), compute_ponds_cesm
  (source/ice_meltpond_cesm.F90:61-197), merge_fluxes (source/ice_flux.F90:681-831).
The device runs the part in front of thermo_vertical for every category first; this file keeps the reference's interleaving, so that
comparing the two checks the claim that the two orders give the same result.

**PARITY IS UNPINNED**: no reference-built record of these routines exists; this file is held to the Fortran by reading.

The math functions are parameters: PORTS (npridge.dev_exp and tests/npfmath2.py: the device's bits) or LIBM (math.exp / log / atan / pow).
min / max are a comparison and a select; sign(a, b) is copysign; x**2 is x*x; sqrt is IEEE.  Stated departures, shared with the device
(include/evpk.h): the cell lists of the category loop and of compute_ponds_cesm require tmask; the eight per-category results of
atmo_boundary_layer are planes (nb, ncat, ny, nx), zero wherever the cell is not listed; Cdn_atm_ratio_n is zero without calc_strair.
The frain / fsnow scaling of :294-314 (ACCESS) is left out.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx).
"""
from __future__ import annotations

import math

import numpy as np

from . import npfmath2 as f2
from . import nptherm1
from .npridge import dev_exp

PUNY = 1.0e-11
C0, C1, C2, C5, C8, C10, C16, P5, P01 = 0.0, 1.0, 2.0, 5.0, 8.0, 10.0, 16.0, 0.5, 0.01
# drivers/cice/ice_constants.F90; source/ice_therm_vertical.F90:682-687; source/ice_atmo.F90:196; source/ice_meltpond_cesm.F90:116-119
VONKAR, ZREF, ICERUF, ZVIR, CP_AIR, CP_WV, GRAVIT, LSUB = 0.4, 10.0, 0.0005, 0.606, 1005.0, 1.81e3, 9.80616, 2.835e6
PI = 3.14159265358979323846
PIH, SECDAY, RHOFRESH, TIMELT = 0.5 * PI, 86400.0, 1000.0, 0.0
CP_OCN, TFFRESH, TTTICE, QQQICE, EMISSIVITY = nptherm1.CP_OCN, nptherm1.TFFRESH, nptherm1.TTTICE, nptherm1.QQQICE, nptherm1.EMISSIVITY
M1, M2, FLOEDIAM, FLOESHAPE, ZTRF = 1.6e-6, 1.36, 300.0, 0.66, 2.0
CPVIR = CP_WV / CP_AIR - C1
TD, REXP, DPTHHI = 2.0, 0.01, 0.9

PORTS = dict(exp=dev_exp, log=f2.evpk_log, atan=f2.evpk_atan, pow=f2.evpk_pow_pos)
LIBM = dict(exp=math.exp, log=math.log, atan=math.atan, pow=math.pow)

PERCAT8 = ["shcoef", "lhcoef", "strairxn", "strairyn", "Cdn_atm_ratio_n", "Trefn", "Qrefn", "Urefn"]
# merge_fluxes: (cumulative plane, per-category plane) in the order of its statements
MERGE = [("strairxT", "strairxn"), ("strairyT", "strairyn"), ("Cdn_atm_ratio", "Cdn_atm_ratio_n"), ("fsurf", "fsurfn"), ("fcondtop", "fcondtopn"),
         ("fsens", "fsensn"), ("flat", "flatn"), ("fswabs", "fswabsn"), ("flwout", "flwoutn"), ("evap", "evapn"), ("Tref", "Trefn"), ("Qref", "Qrefn"),
         ("Uref", "Urefn"), ("fresh", "freshn"), ("fsalt", "fsaltn"), ("fhocn", "fhocnn"), ("fswthru", "fswthrun"), ("meltt", "melttn"),
         ("meltb", "meltbn"), ("melts", "meltsn"), ("congel", "congeln"), ("snoice", "snoicen")]
MERGED = [m for m, _ in MERGE]
OUT2D = ["rside", "fbot", "Tbot", "aice_init"]
OUT3D = ["aicen_init", "vicen_init"] + PERCAT8
INFO_KEYS = ["frzmlt_neg", "frzmlt_pos", "fbot_product", "fbot_frzmlt", "ustar_below", "ustar_above", "deltaT_zero", "deltaT_pos", "xtmp_limits",
             "xtmp_one", "rside_one", "wind_below", "wind_above", "stable", "unstable", "hol_clamped", "hol_free", "delq_pos", "delq_neg",
             "zlvl_not_zref", "in_lmask_n", "in_lmask_s", "in_neither", "fy_reset", "pond_thin", "pond_grow", "pond_frozen", "pond_capped",
             "listed", "merged"]

_min, _max = nptherm1._min, nptherm1._max


def params(x, conduct=0, **kw):
    """nptherm1.params plus the scalars of the rest of step_therm1, from an input dict of tests/golden/therm1svec.py"""
    p = nptherm1.params(x, conduct)
    for k in ("chio", "ustar_min", "natmiter", "calc_strair", "hi_min", "pndaspect", "rfracmin", "rfracmax"):
        p[k] = x[k]
    p.update(kw)
    return p


def frzmlt_bottom_lateral(blk, p, y, b, M, info, sig):
    ilo, ihi, jlo, jhi = blk
    tr = p["tr"]
    nilyr, nslyr, nt_qice, nt_qsno = tr["nilyr"], tr["nslyr"], tr["nt_qice"] - 1, tr["nt_qsno"] - 1
    dt, rhow = p["dt"], p["rhow"]
    ncat = y["aicen"].shape[1]
    cpchr = -((CP_OCN * rhow) * p["chio"])
    rside, Tbot, fbot = y["rside"][b], y["Tbot"][b], y["fbot"][b]
    rside[:] = C0
    Tbot[:] = y["Tf"][b]
    fbot[:] = C0
    cells = [(j, i) for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi) if y["aice"][b, j, i] > PUNY and y["frzmlt"][b, j, i] < C0]
    fside = {}
    for (j, i) in cells:
        fside[j, i] = C0
        frz = float(y["frzmlt"][b, j, i])
        deltaT = _max(float(y["sst"][b, j, i]) - float(Tbot[j, i]), C0)
        sx, sy = float(y["strocnxT"][b, j, i]), float(y["strocnyT"][b, j, i])
        ustar = math.sqrt(math.sqrt(sx * sx + sy * sy) / rhow)
        info["ustar_below" if ustar < p["ustar_min"] else "ustar_above"] += 1
        ustar = _max(ustar, p["ustar_min"])
        fb = (cpchr * deltaT) * ustar
        info["fbot_frzmlt" if frz > fb else "fbot_product"] += 1
        s1 = frz > fb
        fb = _max(fb, frz)
        fbot[j, i] = fb
        info["deltaT_zero" if deltaT == C0 else "deltaT_pos"] += 1
        wlat = M1 * M["pow"](deltaT, M2)
        rs = ((wlat * dt) * PI) / (FLOESHAPE * FLOEDIAM)
        s2 = rs > C1
        info["rside_one"] += int(s2)
        rs = _max(C0, _min(rs, C1))
        rside[j, i] = rs
        sig[b, j, i] = (s1, s2)
    for n in range(ncat):
        etot = {c: C0 for c in cells}
        for k in range(nslyr):
            for (j, i) in cells:
                etot[j, i] = etot[j, i] + (float(y["trcrn"][b, n, nt_qsno + k, j, i]) * float(y["vsnon"][b, n, j, i])) / float(nslyr)
        for k in range(nilyr):
            for (j, i) in cells:
                etot[j, i] = etot[j, i] + (float(y["trcrn"][b, n, nt_qice + k, j, i]) * float(y["vicen"][b, n, j, i])) / float(nilyr)
        for (j, i) in cells:
            fside[j, i] = fside[j, i] + (float(rside[j, i]) * etot[j, i]) / dt
    for (j, i) in cells:
        xtmp = float(y["frzmlt"][b, j, i]) / ((float(fbot[j, i]) + fside[j, i]) + PUNY)
        s3 = xtmp < C1
        info["xtmp_limits" if s3 else "xtmp_one"] += 1
        xtmp = _min(xtmp, C1)
        fbot[j, i] = float(fbot[j, i]) * xtmp
        rside[j, i] = float(rside[j, i]) * xtmp
        sig[b, j, i] = sig[b, j, i] + (s3,)
    info["frzmlt_neg"] += len(cells)
    info["frzmlt_pos"] += sum(1 for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi) if y["aice"][b, j, i] > PUNY and y["frzmlt"][b, j, i] > C0)


def atmo_boundary_layer(J, I, p, y, b, n, M, info, sig):
    log, atan, exp = M["log"], M["atan"], M["exp"]
    psimhu = lambda xd: (log(((C1 + xd * (C2 + xd)) * (C1 + xd * xd)) / C8) - C2 * atan(xd)) + PIH
    psixhu = lambda xd: C2 * log((C1 + xd * xd) / C2)
    al2 = log(ZREF / ZTRF)
    nt_Tsfc = p["tr"]["nt_Tsfc"] - 1
    for q in PERCAT8:                                    # (:240-252, :384-389 and the stated departure: zero where not listed)
        y[q][b, n] = C0
    for j, i in zip(J, I):
        g = lambda q: float(y[q][b, j, i])
        potT, Qa, rhoa, uatm, vatm, wind, zlvl = g("potT"), g("Qa"), g("rhoa"), g("uatm"), g("vatm"), g("wind"), g("zlvl")
        info["wind_below" if wind < C1 else "wind_above"] += 1
        info["zlvl_not_zref"] += int(zlvl != ZREF)
        vmag = _max(C1, wind)
        rdn = VONKAR / log(ZREF / ICERUF)
        y["Cdn_atm"][b, j, i] = rdn * rdn
        TsfK = float(y["trcrn"][b, n, nt_Tsfc, j, i]) + TFFRESH
        qsat = QQQICE * exp(-TTTICE / TsfK)
        ssq = qsat / rhoa
        thva = potT * (C1 + ZVIR * Qa)
        delt = potT - TsfK
        delq = Qa - ssq
        info["delq_pos" if delq > C0 else "delq_neg"] += 1
        alz = log(zlvl / ZREF)
        cp = CP_AIR * (C1 + CPVIR * ssq)
        rhn = ren = rdn
        ustar, tstar, qstar = rdn * vmag, rhn * delt, ren * delq
        s = []
        for _ in range(p["natmiter"]):
            hol = (((VONKAR * GRAVIT) * zlvl) * (tstar / thva + qstar / (C1 / ZVIR + Qa))) / (ustar * ustar)
            clamped = abs(hol) > C10
            hol = math.copysign(_min(abs(hol), C10), hol)
            stable = P5 + math.copysign(P5, hol)
            s.append((stable, clamped))
            xqq = _max(math.sqrt(abs(C1 - C16 * hol)), C1)
            xqq = math.sqrt(xqq)
            psimhs = -((0.7 * hol + (0.75 * (hol - 14.3)) * exp(-0.35 * hol)) + 10.7)
            psimh = psimhs * stable + (C1 - stable) * psimhu(xqq)
            psixh = psimhs * stable + (C1 - stable) * psixhu(xqq)
            rd = rdn / (C1 + (rdn / VONKAR) * (alz - psimh))
            rh = rhn / (C1 + (rhn / VONKAR) * (alz - psixh))
            re = ren / (C1 + (ren / VONKAR) * (alz - psixh))
            ustar, tstar, qstar = rd * vmag, rh * delt, re * delq
        info["stable" if stable == C1 else "unstable"] += 1
        info["hol_clamped" if clamped else "hol_free"] += 1
        sig[b, n, j, i] = tuple(s)
        if p["calc_strair"]:
            tau = (rhoa * ustar) * rd
            y["strairxn"][b, n, j, i] = tau * uatm
            y["strairyn"][b, n, j, i] = tau * vatm
            y["Cdn_atm_ratio_n"][b, n, j, i] = ((rd * rd) / rdn) / rdn
        y["shcoef"][b, n, j, i] = (((rhoa * ustar) * cp) * rh) + C1
        y["lhcoef"][b, n, j, i] = ((rhoa * ustar) * LSUB) * re
        hol = (hol * ZTRF) / zlvl
        xqq = _max(C1, math.sqrt(abs(C1 - C16 * hol)))
        xqq = math.sqrt(xqq)
        psix2 = ((-C5 * hol) * stable) + (C1 - stable) * psixhu(xqq)
        fac = (rh / VONKAR) * (((alz + al2) - psixh) + psix2)
        Tref = potT - delt * fac
        y["Trefn"][b, n, j, i] = Tref - P01 * ZTRF
        fac = (re / VONKAR) * (((alz + al2) - psixh) + psix2)
        y["Qrefn"][b, n, j, i] = Qa - delq * fac
        y["Urefn"][b, n, j, i] = (vmag * rd) / rdn


def compute_ponds_cesm(blk, tmask, p, y, b, n, M, info):
    ilo, ihi, jlo, jhi = blk
    tr = p["tr"]
    nt_Tsfc, nt_apnd, nt_hpnd = tr["nt_Tsfc"] - 1, tr["nt_apnd"] - 1, tr["nt_hpnd"] - 1
    dt, rhoi, rhos = p["dt"], p["rhoi"], p["rhos"]
    t = y["trcrn"][b, n]
    for j in range(jlo - 1, jhi):
        for i in range(ilo - 1, ihi):
            aicen = float(y["aicen"][b, n, j, i])
            if not (tmask[b, j, i] and aicen > PUNY):
                continue
            rfrac = p["rfracmin"] + (p["rfracmax"] - p["rfracmin"]) * aicen
            volpn = (float(t[nt_hpnd, j, i]) * float(t[nt_apnd, j, i])) * aicen
            hi = float(y["vicen"][b, n, j, i]) / aicen
            if hi < p["hi_min"]:
                apondn = hpondn = C0
                info["pond_thin"] += 1
            else:
                volpn = volpn + ((rfrac / RHOFRESH) * ((float(y["melttn"][b, n, j, i]) * rhoi + float(y["meltsn"][b, n, j, i]) * rhos)
                                                       + float(y["frain"][b, j, i]) * dt)) * aicen
                Tp = TIMELT - TD
                dTs = _max(Tp - float(t[nt_Tsfc, j, i]), C0)
                info["pond_frozen" if dTs > C0 else "pond_grow"] += 1
                volpn = volpn * M["exp"]((REXP * dTs) / Tp)
                volpn = _max(volpn, C0)
                apondn = _min(math.sqrt(volpn / (p["pndaspect"] * aicen)), C1)
                hpondn = p["pndaspect"] * apondn
                apondn = apondn * aicen
                info["pond_capped"] += int(DPTHHI * hi < hpondn)
                hpondn = _min(hpondn, DPTHHI * hi)
            t[nt_apnd, j, i] = apondn / aicen
            t[nt_hpnd, j, i] = hpondn


def merge_fluxes(J, I, y, b, n, info):
    for j, i in zip(J, I):
        w = float(y["aicen_init"][b, n, j, i])
        fswthrun = float(y["fswthrun"][b, n, j, i])
        fswabsn = (float(y["fswsfcn"][b, n, j, i]) + float(y["fswintn"][b, n, j, i])) + fswthrun
        for m, q in MERGE:
            if q == "fswabsn":
                v = fswabsn
            elif q == "flwoutn":
                v = float(y[q][b, n, j, i]) - (C1 - EMISSIVITY) * float(y["flw"][b, j, i])
            else:
                v = float(y[q][b, n, j, i])
            y[m][b, j, i] = float(y[m][b, j, i]) + v * w
        info["merged"] += 1


def step(blocks, tmask, p, y, M=PORTS, iters=None):
    """step_therm1 on every block.  blocks: (ilo, ihi, jlo, jhi) 1-based; y: dict of the arrays, rewritten in place (fbot, Tbot and the eight
    per-category planes of atmo_boundary_layer are members of y).  Returns (infos per block, stop, sig): stop None or (reason, block,
    category, i, j) as nptherm1.step; sig: the branches taken, per frzmlt cell and per listed (cell, category)"""
    ncat = y["aicen"].shape[1]
    tr = p["tr"]
    infos, sig = [], {}
    saved = nptherm1.dev_exp
    nptherm1.dev_exp = M["exp"]                           # (thermo_vertical's exp with the rest)
    try:
        with np.errstate(all="ignore"):
            for b, blk in enumerate(blocks):
                ilo, ihi, jlo, jhi = blk
                info = {k: 0 for k in list(nptherm1.INFO_KEYS) + INFO_KEYS}
                infos.append(info)
                y["aice_init"][b] = y["aice"][b]
                y["aicen_init"][b] = y["aicen"][b]
                y["vicen_init"][b] = y["vicen"][b]
                frzmlt_bottom_lateral(blk, p, y, b, M, info, sig)
                fy_n = y["yday"] >= 259.0 and y["yday"] < 259.0 + p["dt"] / SECDAY
                fy_s = y["yday"] >= 75.0 and y["yday"] < 75.0 + p["dt"] / SECDAY
                for n in range(ncat):
                    for q in nptherm1.OUT15:
                        y[q][b, n] = C0
                    J, I = [], []
                    for j in range(jlo - 1, jhi):
                        for i in range(ilo - 1, ihi):
                            if tmask[b, j, i] and y["aicen"][b, n, j, i] > PUNY:
                                J.append(j); I.append(i)
                    info["listed"] += len(J)
                    info["cells"] += len(J)
                    atmo_boundary_layer(J, I, p, y, b, n, M, info, sig)
                    if not p["calc_strair"]:
                        y["strairxn"][b, n] = C0
                        y["strairyn"][b, n] = C0
                    if tr.get("tr_iage"):
                        for j, i in zip(J, I):
                            y["trcrn"][b, n, tr["nt_iage"] - 1, j, i] = float(y["trcrn"][b, n, tr["nt_iage"] - 1, j, i]) + p["dt"]
                    if tr.get("tr_FY"):
                        for j, i in zip(J, I):
                            ln, ls = bool(y["lmask_n"][b, j, i]), bool(y["lmask_s"][b, j, i])
                            info["in_lmask_n" if ln else "in_lmask_s" if ls else "in_neither"] += 1
                            if (fy_n and ln) or (fy_s and ls):
                                y["trcrn"][b, n, tr["nt_FY"] - 1, j, i] = C0
                                info["fy_reset"] += 1
                    if J:
                        stop = nptherm1.thermo_vertical(J, I, p, y, b, n, info, iters)
                        if stop is not None:
                            return infos, (stop[0], b + 1, n + 1, stop[1], stop[2]), sig
                    if tr.get("tr_pond_cesm"):
                        compute_ponds_cesm(blk, tmask, p, y, b, n, M, info)
                    merge_fluxes(J, I, y, b, n, info)
    finally:
        nptherm1.dev_exp = saved
    return infos, None, sig
