"""numpy / Python restatement of thermo_vertical (source/ice_therm_vertical.F90:79-531) as step_therm1 calls it per block and category
(source/ice_step_mod.F90:364-540), BL99 path (ktherm = 1, heat_capacity, calc_Tsfc, l_brine all .true.) -- written from the Fortran and
independent of the HIP code: the category loop outside, one cell list per block and category, the Fortran's loop order (layer loops
outside the cell loops where the Fortran has them) and its scalar operation order.  The temperature iteration runs block-wide with
`converged` per cell, as the reference does (a converged cell is no longer touched).
  init_vertical_profile (:845-1273), calculate_Tin_from_qin (ice_therm_shared.F90:62-90)
  temperature_changes (ice_therm_bl99.F90:51-928), conductivity (:940-1062), surface_heat_flux / dsurface_heat_flux_dTsf
  (ice_therm_shared.F90:98-226), get_matrix_elements_calc_Tsfc (:1172-1480), tridiag_solver (:1763-1840)
  thickness_changes (:1283-2020), freeboard (:2031-2170), adjust_enthalpy (:2177-2280)
  conservation_check_vthermo (:2283-2406), the flux lines :482-503, update_state_vthermo (:2417-2540)

**PARITY IS UNPINNED for all of thermo_vertical**: there is no reference-built record of it, so this file is held to the Fortran by
reading, not by a fixture.

min / max are a comparison and a select; exp is npridge.dev_exp; x**2, x**3, x**4 are x*x, x*x*x, (x*x)*(x*x); sqrt is IEEE.  ktherm = 1
makes qmlt, emlt_atm, emlt_ocn and fadvocn zero: the statements that only feed them are left out, the additions of those zeros are kept.
Stated departure, shared with the device (include/evpk.h): the cell list is physical cells with tmask and aicen > puny.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), Sswabsn (nb, ncat, nslyr,
ny, nx), Iswabsn (nb, ncat, nilyr, ny, nx).
"""
from __future__ import annotations

import math

import numpy as np

from .npridge import dev_exp

F = np.float64
PUNY = 1.0e-11
C0, C1, C2, C4, P1, P5, P001 = 0.0, 1.0, 2.0, 4.0, 0.1, 0.5, 0.001
# drivers/cice/ice_constants.F90, source/ice_therm_bl99.F90:27-28, :148-152, source/ice_therm_shared.F90:31
CP_OCN, LVAP, TFFRESH, TTTICE, QQQICE, EMISSIVITY, STEFAN = 4218.0, 2.501e6, 273.15, 5897.8, 11637800.0, 0.95, 567.0e-10
DEPRESST, KSNO, KICE, BETAK, KIMIN, TSF_ERRMAX, FERRMAX, NITERMAX = 0.054, 0.30, 2.03, 0.13, 0.10, 5.0e-4, 1.0e-3, 500
FRAC_SW, DTEMP = 0.9, 0.02

OUT15 = ["flwoutn", "evapn", "freshn", "fsaltn", "fhocnn", "fsensn", "flatn", "fsurfn", "fcondtopn", "melttn", "meltsn", "meltbn", "congeln",
         "snoicen", "dsnown"]
STOP_REASONS = {1: "zTsn > Tmax", 2: "zTsn < Tmin", 3: "zSin < min_salin", 4: "zTin > Tmlts", 5: "zTin < Tmin", 6: "no convergence",
                7: "ferr > ferrmax"}
INFO_KEYS = ["cells", "unlisted_in_ice_cell", "l_snow", "no_snow", "cold_surface", "melting_surface", "tsf_reset", "cond1", "cond2", "cond3",
             "cond4", "cond5", "cond5_reduce_kh", "iter1", "iter2_3", "iter_gt3", "iswabs_moved", "sswabs_moved", "tsn_reset", "tin_reset",
             "cond_snow", "cond_ice", "sublim_snow_to_ice", "topmelt_in_snow", "topmelt_to_ice", "grow_unclamped", "grow_clamped", "botmelt",
             "botmelt_snow", "vanished", "snowfall_bare", "snowfall_snow", "no_snowfall", "freeboard", "mlt_onset_set", "mlt_onset_kept",
             "frz_onset_set", "frz_onset_kept", "fpond_changed", "limited_tin"]


def _min(x, y):
    return y if y < x else x


def _max(x, y):
    return y if y > x else x


def params(x, conduct=0, **kw):
    """the scalar arguments of one call from an input dict of tests/golden/therm1vec.py"""
    k = x["k"]
    p = dict(dt=float(x["dt"]), yday=float(x["yday"]), conduct=int(conduct), min_salin=float(x["min_salin"]), rhoi=float(k["rhoi"]),
             rhos=float(k["rhos"]), rhow=float(x["rhow"]), cp_ice=float(k["cp_ice"]), Lfresh=float(k["Lfresh"]), hs_min=float(k["hs_min"]),
             Tmin=float(k["Tmin"]), salinity=float(k["ice_ref_salinity"]), tr=dict(x["tracers"]))
    p.update(kw)
    return p


def calculate_Tin_from_qin(qin, Tmltk, p):
    aa1 = p["cp_ice"]
    bb1 = (CP_OCN - p["cp_ice"]) * Tmltk - qin / p["rhoi"] - p["Lfresh"]
    cc1 = p["Lfresh"] * Tmltk
    return _min((-bb1 - float(np.sqrt(F(bb1 * bb1 - C4 * aa1 * cc1)))) / (C2 * aa1), Tmltk)


def adjust_enthalpy(nlyr, z1, z2, hlyr, hn, qn):
    """:2228-2270 for one cell; z1, z2 (nlyr + 1), qn (nlyr) rewritten"""
    rhlyr = C0
    if hn > PUNY:
        rhlyr = C1 / hlyr
    hq = [C0] * nlyr
    k1 = k2 = 1
    while k1 <= nlyr and k2 <= nlyr:
        hovlp = _min(z1[k1], z2[k2]) - _max(z1[k1 - 1], z2[k2 - 1])
        hovlp = _max(hovlp, C0)
        hq[k2 - 1] = hq[k2 - 1] + hovlp * qn[k1 - 1]
        if z1[k1] > z2[k2]:
            k2 += 1
        else:
            k1 += 1
    for k in range(nlyr):
        qn[k] = hq[k] * rhlyr


def thermo_vertical(J, I, p, y, b, n, info, iters=None):
    """one thermo_vertical call: block b, category n (0-based), the cell list (J, I) (0-based).  y: dict of the full arrays, rewritten in
    place.  Returns None or (reason, i, j) 1-based.  iters: optional list that receives (b, n, j, i, niter)"""
    with np.errstate(all="ignore"):
        return _thermo_vertical(J, I, p, y, b, n, info, iters)


def _thermo_vertical(J, I, p, y, b, n, info, iters):
    tr = p["tr"]
    nilyr, nslyr = tr["nilyr"], tr["nslyr"]
    nt_Tsfc, nt_qice, nt_qsno, nt_sice = tr["nt_Tsfc"] - 1, tr["nt_qice"] - 1, tr["nt_qsno"] - 1, tr["nt_sice"] - 1
    topo = bool(tr.get("tr_pond_topo"))
    dt, rhoi, rhos, rhow, cp_ice, Lfresh = p["dt"], p["rhoi"], p["rhos"], p["rhow"], p["cp_ice"], p["Lfresh"]
    hs_min, Tmin, puny = p["hs_min"], p["Tmin"], PUNY
    rnslyr, rnilyr = float(nslyr), float(nilyr)
    ic = len(J)
    aicen, vicen, vsnon, trcrn = y["aicen"][b, n], y["vicen"][b, n], y["vsnon"][b, n], y["trcrn"][b, n]
    g2 = lambda q: y[q][b]
    flw, potT, Qa, rhoa, fsnow, fbot, Tbot = (g2(q) for q in ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot"))
    shcoef, lhcoef = y["shcoef"][b, n], y["lhcoef"][b, n]
    fswsfc, fswint, Sswabs, Iswabs = y["fswsfcn"][b, n], y["fswintn"][b, n], y["Sswabsn"][b, n], y["Iswabsn"][b, n]
    mlt_onset, frz_onset = y["mlt_onset"][b], y["frz_onset"][b]
    o = {q: y[q][b, n] for q in OUT15}
    flwoutn, evapn, freshn, fsaltn, fhocnn, fsensn, flatn, fsurfn, fcondtopn = (o[q] for q in OUT15[:9])
    meltt, melts, meltb, congel, snoice, dsnow = (o[q] for q in OUT15[9:])
    # (the zeroing of :251-280 and ice_step_mod.F90:366-371 is the caller's, on every cell of the block)
    R = range(ic)

    # ---- init_vertical_profile ----
    Tsf = [C0] * ic; hin = [C0] * ic; hsn = [C0] * ic; hilyr = [C0] * ic; hslyr = [C0] * ic; einit = [C0] * ic
    zqsn = np.zeros((ic, nslyr)); zTsn = np.zeros((ic, nslyr)); zqin = np.zeros((ic, nilyr)); zTin = np.zeros((ic, nilyr))
    zSin = np.zeros((ic, nilyr)); Tmlts = np.zeros((ic, nilyr))
    for ij in R:
        i, j = I[ij], J[ij]
        Tsf[ij] = float(trcrn[nt_Tsfc, j, i])
        hin[ij] = float(vicen[j, i]) / float(aicen[j, i])
        hsn[ij] = float(vsnon[j, i]) / float(aicen[j, i])
        hilyr[ij] = hin[ij] / rnilyr
        hslyr[ij] = hsn[ij] / rnslyr
    tsno_high = tsno_low = False

    def snow_tmax(ij, k):
        if hslyr[ij] > hs_min / rnslyr:
            return -float(zqsn[ij, k]) * puny * rnslyr / (rhos * cp_ice * float(vsnon[J[ij], I[ij]]))
        return puny
    for k in range(nslyr):
        for ij in R:
            i, j = I[ij], J[ij]
            if hslyr[ij] > hs_min / rnslyr:
                zqsn[ij, k] = trcrn[nt_qsno + k, j, i]
            else:
                zqsn[ij, k] = -rhos * Lfresh
            Tmax = snow_tmax(ij, k)
            zTsn[ij, k] = (Lfresh + float(zqsn[ij, k]) / rhos) / cp_ice
            if zTsn[ij, k] > Tmax:
                tsno_high = True
            elif zTsn[ij, k] < Tmin:
                tsno_low = True
    if tsno_high:
        for k in range(nslyr):
            for ij in R:
                if zTsn[ij, k] > snow_tmax(ij, k):
                    return (1, I[ij] + 1, J[ij] + 1)
    if tsno_low:
        for k in range(nslyr):
            for ij in R:
                if zTsn[ij, k] < Tmin:
                    return (2, I[ij] + 1, J[ij] + 1)
    for k in range(nslyr):
        for ij in R:
            if zTsn[ij, k] > C0:
                zTsn[ij, k] = C0
                zqsn[ij, k] = -rhos * Lfresh
                info["tsn_reset"] += 1
            einit[ij] = einit[ij] + hslyr[ij] * float(zqsn[ij, k])
    tice_high = tice_low = False
    for k in range(nilyr):
        for ij in R:
            i, j = I[ij], J[ij]
            zSin[ij, k] = trcrn[nt_sice + k, j, i]
            if zSin[ij, k] < p["min_salin"] - puny:
                return (3, i + 1, j + 1)
            Tmlts[ij, k] = -float(zSin[ij, k]) * DEPRESST
            zqin[ij, k] = trcrn[nt_qice + k, j, i]
            zTin[ij, k] = calculate_Tin_from_qin(float(zqin[ij, k]), float(Tmlts[ij, k]), p)
            Tmax = Tmlts[ij, k]
            if zTin[ij, k] > Tmax:
                tice_high = True
            elif zTin[ij, k] < Tmin:
                tice_low = True
        if tice_high:
            for ij in R:
                if zTin[ij, k] > Tmlts[ij, k]:
                    return (4, I[ij] + 1, J[ij] + 1)
        if tice_low:
            for ij in R:
                if zTin[ij, k] < Tmin:
                    return (5, I[ij] + 1, J[ij] + 1)
        for ij in R:
            if zTin[ij, k] > C0:
                zTin[ij, k] = C0
                zqin[ij, k] = -rhoi * Lfresh
                info["tin_reset"] += 1
        for ij in R:
            einit[ij] = einit[ij] + hilyr[ij] * float(zqin[ij, k])
    worki, works = list(hin), list(hsn)

    # ---- temperature_changes ----
    nmat = nslyr + nilyr + 1
    converged = [False] * ic; l_snow = [False] * ic; l_cold = [True] * ic
    fcondbot = [C0] * ic; dTsf_prev = [C0] * ic; dfsens_dT = [C0] * ic; dflat_dT = [C0] * ic; dflwout_dT = [C0] * ic; einex = [C0] * ic
    dt_rhoi_hlyr = [C0] * ic; ferr = [C0] * ic; nit = [0] * ic
    for ij in R:
        dt_rhoi_hlyr[ij] = dt / (rhoi * hilyr[ij])
        if hslyr[ij] > hs_min / float(nslyr):
            l_snow[ij] = True
        info["l_snow" if l_snow[ij] else "no_snow"] += 1
    Tsn_init = zTsn.copy(); Tsn_start = zTsn.copy(); etas = np.zeros((ic, nslyr))
    for k in range(nslyr):
        for ij in R:
            etas[ij, k] = dt / (rhos * cp_ice * hslyr[ij]) if l_snow[ij] else C0
    Tin_init = zTin.copy(); Tin_start = zTin.copy()
    for k in range(nilyr):
        for ij in R:
            Tmlts[ij, k] = -float(zSin[ij, k]) * DEPRESST
    # conductivity
    kh = np.zeros((ic, nmat)); kilyr = np.zeros((ic, nilyr))
    for k in range(nilyr):
        for ij in R:
            S, Tk = float(zSin[ij, k]), float(zTin[ij, k])
            if p["conduct"] == 0:
                v = KICE + BETAK * S / _min(-puny, Tk)
            else:
                v = (2.11 - 0.011 * Tk + 0.09 * S / _min(-puny, Tk)) * rhoi / 917.0
            kilyr[ij, k] = _max(v, KIMIN)
    for ij in R:
        k1, kn = float(kilyr[ij, 0]), float(kilyr[ij, nilyr - 1])
        if l_snow[ij]:
            kh[ij, 0] = C2 * KSNO / hslyr[ij]
            kh[ij, nslyr] = C2 * KSNO * k1 / (KSNO * hilyr[ij] + k1 * hslyr[ij])
        else:
            kh[ij, 0] = C0
            kh[ij, nslyr] = C2 * k1 / hilyr[ij]
        kh[ij, nslyr + nilyr] = C2 * kn / hilyr[ij]
    for k in range(2, nslyr + 1):
        for ij in R:
            kh[ij, k - 1] = C2 * KSNO * KSNO / ((KSNO + KSNO) * hslyr[ij]) if l_snow[ij] else C0
    for k in range(2, nilyr + 1):
        for ij in R:
            ka, kb = float(kilyr[ij, k - 2]), float(kilyr[ij, k - 1])
            kh[ij, k - 1 + nslyr] = C2 * ka * kb / ((ka + kb) * hilyr[ij])
    # excess absorbed shortwave into the surface
    for k in range(nilyr):
        for ij in R:
            i, j = I[ij], J[ij]
            Isw, Ti0, Tm = float(Iswabs[k, j, i]), float(Tin_init[ij, k]), float(Tmlts[ij, k])
            Iswabs_tmp = C0
            if Ti0 <= Tm - DTEMP:
                ci = cp_ice - Lfresh * Tm / (Ti0 * Ti0)
                Iswabs_tmp = _min(Isw, FRAC_SW * (Tm - Ti0) * ci / dt_rhoi_hlyr[ij])
            if Iswabs_tmp < puny:
                Iswabs_tmp = C0
            dswabs = _min(Isw - Iswabs_tmp, float(fswint[j, i]))
            if dswabs != 0.0:
                info["iswabs_moved"] += 1
            fswsfc[j, i] = float(fswsfc[j, i]) + dswabs
            fswint[j, i] = float(fswint[j, i]) - dswabs
            Iswabs[k, j, i] = Iswabs_tmp
    for k in range(nslyr):
        for ij in R:
            if l_snow[ij]:
                i, j = I[ij], J[ij]
                Ssw, Ts0 = float(Sswabs[k, j, i]), float(Tsn_init[ij, k])
                Sswabs_tmp = C0
                if Ts0 <= -DTEMP:
                    Sswabs_tmp = _min(Ssw, -FRAC_SW * Ts0 / float(etas[ij, k]))
                if Sswabs_tmp < puny:
                    Sswabs_tmp = C0
                dswabs = _min(Ssw - Sswabs_tmp, float(fswint[j, i]))
                if dswabs != 0.0:
                    info["sswabs_moved"] += 1
                fswsfc[j, i] = float(fswsfc[j, i]) + dswabs
                fswint[j, i] = float(fswint[j, i]) - dswabs
                Sswabs[k, j, i] = Sswabs_tmp

    all_converged = False
    for niter in range(1, NITERMAX + 1):
        if all_converged:
            break
        solve = [m for m in R if not converged[m]]
        ns = len(solve)
        all_converged = True
        dfsurf_dT = [C0] * ns; avg_Tsi = [C0] * ns; enew = [C0] * ns; Tsf_start = [C0] * ns; dTsf = [C0] * ns
        etai = np.zeros((ns, nilyr))
        for m in solve:
            converged[m] = True
            einex[m] = C0
            nit[m] = niter
        for k in range(nilyr):
            for ij, m in enumerate(solve):
                ci = cp_ice - Lfresh * float(Tmlts[m, k]) / (float(zTin[m, k]) * float(Tin_init[m, k]))
                etai[ij, k] = dt_rhoi_hlyr[m] / ci
        for ij, m in enumerate(solve):
            i, j = I[m], J[m]
            # surface_heat_flux
            TsfK = Tsf[m] + TFFRESH
            tmpvar = C1 / TsfK
            qsat = QQQICE * dev_exp(-TTTICE * tmpvar)
            Qsfc = qsat / float(rhoa[j, i])
            flwdabs = EMISSIVITY * float(flw[j, i])
            flwoutn[j, i] = -EMISSIVITY * STEFAN * ((TsfK * TsfK) * (TsfK * TsfK))
            fsensn[j, i] = float(shcoef[j, i]) * (float(potT[j, i]) - TsfK)
            flatn[j, i] = float(lhcoef[j, i]) * (float(Qa[j, i]) - Qsfc)
            fsurfn[j, i] = float(fswsfc[j, i]) + flwdabs + float(flwoutn[j, i]) + float(fsensn[j, i]) + float(flatn[j, i])
            # dsurface_heat_flux_dTsf
            dQsfc_dTsf = TTTICE * tmpvar * tmpvar * (qsat / float(rhoa[j, i]))
            dflwout_dT[m] = -EMISSIVITY * STEFAN * C4 * (TsfK * TsfK * TsfK)
            dfsens_dT[m] = -float(shcoef[j, i])
            dflat_dT[m] = -float(lhcoef[j, i]) * dQsfc_dTsf
            dfsurf_dT[ij] = dflwout_dT[m] + dfsens_dT[m] + dflat_dT[m]
            if l_snow[m]:
                fcondtopn[j, i] = float(kh[m, 0]) * (Tsf[m] - float(zTsn[m, 0]))
            else:
                fcondtopn[j, i] = float(kh[m, nslyr]) * (Tsf[m] - float(zTin[m, 0]))
            if Tsf[m] >= C0 and fsurfn[j, i] < fcondtopn[j, i]:
                Tsf[m] = -puny
                info["tsf_reset"] += 1
            Tsf_start[ij] = Tsf[m]
            l_cold[m] = Tsf[m] < C0
            info["cold_surface" if l_cold[m] else "melting_surface"] += 1
        # get_matrix_elements_calc_Tsfc
        sb = np.zeros((ns, nmat)); dg = np.zeros((ns, nmat)); sp = np.zeros((ns, nmat)); rh = np.zeros((ns, nmat))
        for k in range(nslyr + 1):
            for ij in range(ns):
                sb[ij, k] = C0; dg[ij, k] = C1; sp[ij, k] = C0; rh[ij, k] = C0
        g = lambda a, r, c: float(a[r, c])
        for ij, m in enumerate(solve):
            i, j = I[m], J[m]
            if l_cold[m]:
                kr = 0 if l_snow[m] else nslyr
                sb[ij, kr] = C0
                dg[ij, kr] = dfsurf_dT[ij] - g(kh, m, kr)
                sp[ij, kr] = g(kh, m, kr)
                rh[ij, kr] = dfsurf_dT[ij] * Tsf[m] - float(fsurfn[j, i])
            if l_snow[m]:
                e = g(etas, m, 0)
                if l_cold[m]:
                    sb[ij, 1] = -e * g(kh, m, 0)
                    sp[ij, 1] = -e * g(kh, m, 1)
                    dg[ij, 1] = C1 + e * (g(kh, m, 0) + g(kh, m, 1))
                    rh[ij, 1] = g(Tsn_init, m, 0) + e * float(Sswabs[0, j, i])
                else:
                    sb[ij, 1] = C0
                    sp[ij, 1] = -e * g(kh, m, 1)
                    dg[ij, 1] = C1 + e * (g(kh, m, 0) + g(kh, m, 1))
                    rh[ij, 1] = g(Tsn_init, m, 0) + e * g(kh, m, 0) * Tsf[m] + e * float(Sswabs[0, j, i])
        for k in range(2, nslyr + 1):
            for ij, m in enumerate(solve):
                i, j = I[m], J[m]
                if l_snow[m]:
                    e = g(etas, m, k - 1)
                    sb[ij, k] = -e * g(kh, m, k - 1)
                    sp[ij, k] = -e * g(kh, m, k)
                    dg[ij, k] = C1 + e * (g(kh, m, k - 1) + g(kh, m, k))
                    rh[ij, k] = g(Tsn_init, m, k - 1) + e * float(Sswabs[k - 1, j, i])
        if nilyr > 1:
            k, kr = nslyr, nslyr + 1
            for ij, m in enumerate(solve):
                i, j = I[m], J[m]
                e = g(etai, ij, 0)
                if l_snow[m] or l_cold[m]:
                    sb[ij, kr] = -e * g(kh, m, k)
                    sp[ij, kr] = -e * g(kh, m, k + 1)
                    dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                    rh[ij, kr] = g(Tin_init, m, 0) + e * float(Iswabs[0, j, i])
                else:
                    sb[ij, kr] = C0
                    sp[ij, kr] = -e * g(kh, m, k + 1)
                    dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                    rh[ij, kr] = g(Tin_init, m, 0) + e * float(Iswabs[0, j, i]) + e * g(kh, m, k) * Tsf[m]
            ki, k, kr = nilyr - 1, nilyr - 1 + nslyr, nilyr + nslyr
            for ij, m in enumerate(solve):
                i, j = I[m], J[m]
                e = g(etai, ij, ki)
                sb[ij, kr] = -e * g(kh, m, k)
                sp[ij, kr] = C0
                dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                rh[ij, kr] = g(Tin_init, m, ki) + e * float(Iswabs[ki, j, i]) + e * g(kh, m, k + 1) * float(Tbot[j, i])
        else:
            k, kr = nslyr, nslyr + 1
            for ij, m in enumerate(solve):
                i, j = I[m], J[m]
                e = g(etai, ij, 0)
                if l_snow[m] or l_cold[m]:
                    sb[ij, kr] = -e * g(kh, m, k)
                    sp[ij, kr] = C0
                    dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                    rh[ij, kr] = g(Tin_init, m, 0) + e * float(Iswabs[0, j, i]) + e * g(kh, m, k + 1) * float(Tbot[j, i])
                else:
                    sb[ij, kr] = C0
                    sp[ij, kr] = C0
                    dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                    rh[ij, kr] = (g(Tin_init, m, 0) + e * float(Iswabs[0, j, i]) + e * g(kh, m, k) * Tsf[m]
                                  + e * g(kh, m, k + 1) * float(Tbot[j, i]))
        for ki in range(2, nilyr):
            k, kr = ki - 1 + nslyr, ki + nslyr
            for ij, m in enumerate(solve):
                i, j = I[m], J[m]
                e = g(etai, ij, ki - 1)
                sb[ij, kr] = -e * g(kh, m, k)
                sp[ij, kr] = -e * g(kh, m, k + 1)
                dg[ij, kr] = C1 + e * (g(kh, m, k) + g(kh, m, k + 1))
                rh[ij, kr] = g(Tin_init, m, ki - 1) + e * float(Iswabs[ki - 1, j, i])
        # tridiag_solver
        Tmat = np.zeros((ns, nmat)); wgamma = np.zeros((ns, nmat)); wbeta = [C0] * ns
        for ij in range(ns):
            wbeta[ij] = g(dg, ij, 0)
            Tmat[ij, 0] = g(rh, ij, 0) / wbeta[ij]
        for k in range(1, nmat):
            for ij in range(ns):
                wgamma[ij, k] = g(sp, ij, k - 1) / wbeta[ij]
                wbeta[ij] = g(dg, ij, k) - g(sb, ij, k) * g(wgamma, ij, k)
                Tmat[ij, k] = (g(rh, ij, k) - g(sb, ij, k) * g(Tmat, ij, k - 1)) / wbeta[ij]
        for k in range(nmat - 2, -1, -1):
            for ij in range(ns):
                Tmat[ij, k] = g(Tmat, ij, k) - g(wgamma, ij, k + 1) * g(Tmat, ij, k + 1)
        # conditions 1 and 2
        for ij, m in enumerate(solve):
            if l_cold[m]:
                Tsf[m] = g(Tmat, ij, 0) if l_snow[m] else g(Tmat, ij, nslyr)
            else:
                Tsf[m] = C0
            dTsf[ij] = Tsf[m] - Tsf_start[ij]
            avg_Tsf = C0
            if Tsf[m] > puny:
                Tsf[m] = C0
                dTsf[ij] = -Tsf_start[ij]
                avg_Tsi[ij] = C1
                converged[m] = False
                all_converged = False
                info["cond1"] += 1
            elif (niter > 1 and Tsf_start[ij] <= -puny and abs(dTsf[ij]) > puny and abs(dTsf_prev[m]) > puny
                  and -dTsf[ij] / (dTsf_prev[m] + puny * puny) > P5):
                avg_Tsf = C1
                avg_Tsi[ij] = C1
                dTsf[ij] = P5 * dTsf[ij]
                converged[m] = False
                all_converged = False
                info["cond2"] += 1
            Tsf[m] = Tsf[m] + avg_Tsf * P5 * (Tsf_start[ij] - Tsf[m])
        for k in range(nslyr):
            for ij, m in enumerate(solve):
                v = g(Tmat, ij, k + 1) if l_snow[m] else C0
                v = _min(v, C0)
                v = v + avg_Tsi[ij] * P5 * (g(Tsn_start, m, k) - v)
                zTsn[m, k] = v
                zqsn[m, k] = -rhos * (Lfresh - cp_ice * v)
                enew[ij] = enew[ij] + hslyr[m] * g(zqsn, m, k)
                Tsn_start[m, k] = v
        dqmat = np.zeros((ic, nilyr)); reduce_kh = np.zeros((ic, nilyr), dtype=bool)
        for k in range(nilyr):
            for ij, m in enumerate(solve):
                v, Tm = g(Tmat, ij, k + 1 + nslyr), g(Tmlts, m, k)
                if v > Tm - puny:
                    dTmat = v - Tm
                    dqmat[m, k] = rhoi * dTmat * (cp_ice - Lfresh * Tm / (v * v))
                    v = Tm
                    reduce_kh[m, k] = True
                    info["limited_tin"] += 1
                v = v + avg_Tsi[ij] * P5 * (g(Tin_start, m, k) - v)
                zTin[m, k] = v
                zqin[m, k] = -rhoi * (cp_ice * (Tm - v) + Lfresh * (C1 - Tm / v) - CP_OCN * Tm)
                enew[ij] = enew[ij] + hilyr[m] * g(zqin, m, k)
                einex[m] = einex[m] + hilyr[m] * g(dqmat, m, k)
                Tin_start[m, k] = v
        # conditions 3 and 4
        for ij, m in enumerate(solve):
            i, j = I[m], J[m]
            if abs(dTsf[ij]) > TSF_ERRMAX:
                converged[m] = False
                all_converged = False
                info["cond3"] += 1
            fsurfn[j, i] = float(fsurfn[j, i]) + dTsf[ij] * dfsurf_dT[ij]
            if l_snow[m]:
                fcondtopn[j, i] = g(kh, m, 0) * (Tsf[m] - g(zTsn, m, 0))
            else:
                fcondtopn[j, i] = g(kh, m, nslyr) * (Tsf[m] - g(zTin, m, 0))
            if Tsf[m] >= C0 and fsurfn[j, i] < fcondtopn[j, i]:
                converged[m] = False
                all_converged = False
                info["cond4"] += 1
            dTsf_prev[m] = dTsf[ij]
        # condition 5
        for ij, m in enumerate(solve):
            i, j = I[m], J[m]
            fcondbot[m] = g(kh, m, nslyr + nilyr) * (g(zTin, m, nilyr - 1) - float(Tbot[j, i]))
            fcondbot[m] = fcondbot[m] + einex[m] / dt
            ferr[m] = abs((enew[ij] - einit[m]) / dt - (float(fcondtopn[j, i]) - fcondbot[m] + float(fswint[j, i])))
            if ferr[m] > 0.9 * FERRMAX:
                converged[m] = False
                all_converged = False
                info["cond5"] += 1
                red = False
                for k in range(nilyr):
                    if reduce_kh[m, k] and dqmat[m, k] > C0:
                        frac = _max(0.5 * (C1 - ferr[m] / abs(float(fcondtopn[j, i]) - fcondbot[m])), P1)
                        kh[m, k + nslyr + 1] = g(kh, m, k + nslyr + 1) * frac
                        kh[m, k + nslyr] = kh[m, k + nslyr + 1]
                        red = True
                if red:
                    info["cond5_reduce_kh"] += 1
    if not all_converged:
        for ij in R:
            if not converged[ij]:
                return (6, I[ij] + 1, J[ij] + 1)
    for ij in R:
        i, j = I[ij], J[ij]
        flwoutn[j, i] = float(flwoutn[j, i]) + dTsf_prev[ij] * dflwout_dT[ij]
        fsensn[j, i] = float(fsensn[j, i]) + dTsf_prev[ij] * dfsens_dT[ij]
        flatn[j, i] = float(flatn[j, i]) + dTsf_prev[ij] * dflat_dT[ij]
        info["iter1" if nit[ij] == 1 else "iter2_3" if nit[ij] <= 3 else "iter_gt3"] += 1
        if iters is not None:
            iters.append((b, n, j, i, nit[ij]))

    # ---- thickness_changes ----
    hsn_new = [C0] * ic
    dzi = np.zeros((ic, nilyr)); dzs = np.zeros((ic, nslyr)); qm = np.zeros((ic, nilyr))
    for k in range(nilyr):
        for ij in R:
            dzi[ij, k] = hilyr[ij]
    for k in range(nslyr):
        for ij in R:
            dzs[ij, k] = hslyr[ij]
    for k in range(nilyr):
        for ij in R:
            qm[ij, k] = g(zqin, ij, k) - C0
    esub = [C0] * ic; econ = [C0] * ic; etop_mlt = [C0] * ic; ebot_mlt = [C0] * ic; ebot_gro = [C0] * ic
    qbotmax = -P5 * rhoi * Lfresh
    L = nilyr - 1
    for ij in R:
        i, j = I[ij], J[ij]
        wk1 = -float(flatn[j, i]) * dt
        esub[ij] = _max(wk1, C0)
        econ[ij] = _min(wk1, C0)
        wk1 = (float(fsurfn[j, i]) - float(fcondtopn[j, i])) * dt
        etop_mlt[ij] = _max(wk1, C0)
        wk1 = (fcondbot[ij] - float(fbot[j, i])) * dt
        ebot_mlt[ij] = _max(wk1, C0)
        ebot_gro[ij] = _min(wk1, C0)
        evapn[j, i] = C0
        if hsn[ij] > puny:
            dhs = econ[ij] / (g(zqsn, ij, 0) - rhos * LVAP)
            dzs[ij, 0] = g(dzs, ij, 0) + dhs
            evapn[j, i] = float(evapn[j, i]) + dhs * rhos
            if econ[ij] < C0:
                info["cond_snow"] += 1
        else:
            dhi = econ[ij] / (g(qm, ij, 0) - rhoi * LVAP)
            dzi[ij, 0] = g(dzi, ij, 0) + dhi
            evapn[j, i] = float(evapn[j, i]) + dhi * rhoi
            if econ[ij] < C0:
                info["cond_ice"] += 1
        Tm = -g(zSin, ij, L) * DEPRESST
        Tb = float(Tbot[j, i])
        qbot = -rhoi * (cp_ice * (Tm - Tb) + Lfresh * (C1 - Tm / Tb) - CP_OCN * Tm)
        if ebot_gro[ij] < C0:
            info["grow_clamped" if qbotmax < qbot else "grow_unclamped"] += 1
        qbot = _min(qbot, qbotmax)
        dhi = ebot_gro[ij] / qbot
        hqtot = g(dzi, ij, L) * g(zqin, ij, L) + dhi * qbot
        dzi[ij, L] = g(dzi, ij, L) + dhi
        if dzi[ij, L] > puny:
            zqin[ij, L] = hqtot / g(dzi, ij, L)
            qm[ij, L] = g(zqin, ij, L) - C0
        congel[j, i] = float(congel[j, i]) + dhi
        if dhi > puny:
            info["frz_onset_set" if frz_onset[j, i] < puny else "frz_onset_kept"] += 1
        if dhi > puny and frz_onset[j, i] < puny:
            frz_onset[j, i] = p["yday"]
    sub_snow = [False] * ic; top_snow = [False] * ic; top_ice = [False] * ic
    for k in range(nslyr):
        for ij in R:
            i, j = I[ij], J[ij]
            qsub = g(zqsn, ij, k) - rhos * LVAP
            dhs = _max(-g(dzs, ij, k), esub[ij] / qsub)
            dzs[ij, k] = g(dzs, ij, k) + dhs
            esub[ij] = esub[ij] - dhs * qsub
            esub[ij] = _max(esub[ij], C0)
            evapn[j, i] = float(evapn[j, i]) + dhs * rhos
            if dhs < C0:
                sub_snow[ij] = True
            dhs = _max(-g(dzs, ij, k), etop_mlt[ij] / g(zqsn, ij, k))
            dzs[ij, k] = g(dzs, ij, k) + dhs
            etop_mlt[ij] = etop_mlt[ij] - dhs * g(zqsn, ij, k)
            etop_mlt[ij] = _max(etop_mlt[ij], C0)
            if dhs < -puny:
                top_snow[ij] = True
                info["mlt_onset_set" if mlt_onset[j, i] < puny else "mlt_onset_kept"] += 1
            if dhs < -puny and mlt_onset[j, i] < puny:
                mlt_onset[j, i] = p["yday"]
            melts[j, i] = float(melts[j, i]) - dhs
    for k in range(nilyr):
        for ij in R:
            i, j = I[ij], J[ij]
            qsub = g(qm, ij, k) - rhoi * LVAP
            dhi = _max(-g(dzi, ij, k), esub[ij] / qsub)
            dzi[ij, k] = g(dzi, ij, k) + dhi
            esub[ij] = esub[ij] - dhi * qsub
            esub[ij] = _max(esub[ij], C0)
            evapn[j, i] = float(evapn[j, i]) + dhi * rhoi
            if dhi < C0 and sub_snow[ij] and k == 0:
                info["sublim_snow_to_ice"] += 1
            if qm[ij, k] < C0:
                dhi = _max(-g(dzi, ij, k), etop_mlt[ij] / g(qm, ij, k))
            else:
                qm[ij, k] = C0
                dhi = -g(dzi, ij, k)
            dzi[ij, k] = g(dzi, ij, k) + dhi
            etop_mlt[ij] = _max(etop_mlt[ij] - dhi * g(qm, ij, k), C0)
            if dhi < -puny:
                top_ice[ij] = True
                info["mlt_onset_set" if mlt_onset[j, i] < puny else "mlt_onset_kept"] += 1
            if dhi < -puny and mlt_onset[j, i] < puny:
                mlt_onset[j, i] = p["yday"]
            meltt[j, i] = float(meltt[j, i]) - dhi
    for ij in R:
        if top_snow[ij] and top_ice[ij]:
            info["topmelt_to_ice"] += 1
        elif top_snow[ij]:
            info["topmelt_in_snow"] += 1
    for k in range(nilyr - 1, -1, -1):
        for ij in R:
            i, j = I[ij], J[ij]
            if qm[ij, k] < C0:
                dhi = _max(-g(dzi, ij, k), ebot_mlt[ij] / g(qm, ij, k))
            else:
                qm[ij, k] = C0
                dhi = -g(dzi, ij, k)
            dzi[ij, k] = g(dzi, ij, k) + dhi
            ebot_mlt[ij] = _max(ebot_mlt[ij] - dhi * g(qm, ij, k), C0)
            if dhi < C0 and k == L:
                info["botmelt"] += 1
            meltb[j, i] = float(meltb[j, i]) - dhi
    for k in range(nslyr - 1, -1, -1):
        for ij in R:
            dhs = _max(-g(dzs, ij, k), ebot_mlt[ij] / g(zqsn, ij, k))
            if dhs < C0 and k == nslyr - 1:
                info["botmelt_snow"] += 1
            dzs[ij, k] = g(dzs, ij, k) + dhs
            ebot_mlt[ij] = ebot_mlt[ij] - dhs * g(zqsn, ij, k)
            ebot_mlt[ij] = _max(ebot_mlt[ij], C0)
    for ij in R:
        i, j = I[ij], J[ij]
        fhocnn[j, i] = float(fbot[j, i]) + (esub[ij] + etop_mlt[ij] + ebot_mlt[ij]) / dt
    for ij in R:
        i, j = I[ij], J[ij]
        if fsnow[j, i] > C0:
            info["snowfall_snow" if dzs[ij, 0] > C0 else "snowfall_bare"] += 1
            hsn_new[ij] = float(fsnow[j, i]) / rhos * dt
            zqsnew = -rhos * Lfresh
            hstot = g(dzs, ij, 0) + hsn_new[ij]
            if hstot > C0:
                zqsn[ij, 0] = (g(dzs, ij, 0) * g(zqsn, ij, 0) + hsn_new[ij] * zqsnew) / hstot
                zqsn[ij, 0] = _min(g(zqsn, ij, 0), -rhos * Lfresh)
                dzs[ij, 0] = hstot
        else:
            info["no_snowfall"] += 1
        hin[ij] = C0
        hsn[ij] = C0
    for k in range(nilyr):
        for ij in R:
            hin[ij] = hin[ij] + g(dzi, ij, k)
    for k in range(nslyr):
        for ij in R:
            i, j = I[ij], J[ij]
            hsn[ij] = hsn[ij] + g(dzs, ij, k)
            dsnow[j, i] = float(dsnow[j, i]) + g(dzs, ij, k) - hslyr[ij]
    # freeboard
    dhin = [C0] * ic; dhsn = [C0] * ic; hqs = [C0] * ic
    for ij in R:
        wk1 = hsn[ij] - hin[ij] * (rhow - rhoi) / rhos
        if wk1 > puny and hsn[ij] > puny:
            dhsn[ij] = _min(wk1 * rhoi / rhow, hsn[ij])
            dhin[ij] = dhsn[ij] * rhos / rhoi
    for k in range(nslyr - 1, -1, -1):
        for ij in R:
            i, j = I[ij], J[ij]
            if dhin[ij] > puny:
                dhs = _min(dhsn[ij], g(dzs, ij, k))
                hsn[ij] = hsn[ij] - dhs
                dsnow[j, i] = float(dsnow[j, i]) - dhs
                dzs[ij, k] = g(dzs, ij, k) - dhs
                dhsn[ij] = dhsn[ij] - dhs
                dhsn[ij] = _max(dhsn[ij], C0)
                hqs[ij] = hqs[ij] + dhs * g(zqsn, ij, k)
    for ij in R:
        i, j = I[ij], J[ij]
        if dhin[ij] > puny:
            wk1 = g(dzi, ij, 0) + dhin[ij]
            hin[ij] = hin[ij] + dhin[ij]
            zqin[ij, 0] = (g(dzi, ij, 0) * g(zqin, ij, 0) + hqs[ij]) / wk1
            dzi[ij, 0] = wk1
            snoice[j, i] = float(snoice[j, i]) + dhin[ij]
            info["freeboard"] += 1
    # equal layers
    for ij in R:
        if hin[ij] > C0:
            hilyr[ij] = hin[ij] / float(nilyr)
        else:
            hin[ij] = C0
            hilyr[ij] = C0
        if hsn[ij] > C0:
            hslyr[ij] = hsn[ij] / float(nslyr)
        else:
            hsn[ij] = C0
            hslyr[ij] = C0
    for ij in R:
        z1 = [C0] * (nilyr + 1); z2 = [C0] * (nilyr + 1)
        z1[nilyr] = hin[ij]; z2[nilyr] = hin[ij]
        for k in range(nilyr - 1):
            z1[k + 1] = z1[k] + g(dzi, ij, k)
            z2[k + 1] = z2[k] + hilyr[ij]
        q = [g(zqin, ij, k) for k in range(nilyr)]
        adjust_enthalpy(nilyr, z1, z2, hilyr[ij], hin[ij], q)
        zqin[ij, :] = q
    if nslyr > 1:
        for ij in R:
            z1 = [C0] * (nslyr + 1); z2 = [C0] * (nslyr + 1)
            z1[nslyr] = hsn[ij]; z2[nslyr] = hsn[ij]
            for k in range(nslyr - 1):
                z1[k + 1] = z1[k] + g(dzs, ij, k)
                z2[k + 1] = z2[k] + hslyr[ij]
            q = [g(zqsn, ij, k) for k in range(nslyr)]
            adjust_enthalpy(nslyr, z1, z2, hslyr[ij], hsn[ij], q)
            zqsn[ij, :] = q
    efinal = [C0] * ic
    for ij in R:
        i, j = I[ij], J[ij]
        efinal[ij] = -float(evapn[j, i]) * LVAP
        evapn[j, i] = float(evapn[j, i]) / dt
    for k in range(nslyr):
        for ij in R:
            efinal[ij] = efinal[ij] + hslyr[ij] * g(zqsn, ij, k)
    for k in range(nilyr):
        for ij in R:
            efinal[ij] = efinal[ij] + hilyr[ij] * g(zqin, ij, k)
    for ij in R:
        i, j = I[ij], J[ij]
        fhocnn[j, i] = float(fhocnn[j, i]) + C0 / dt
        efinal[ij] = efinal[ij] + C0

    # ---- conservation_check_vthermo ----
    for ij in R:
        i, j = I[ij], J[ij]
        einp = (float(fsurfn[j, i]) - float(flatn[j, i]) + float(fswint[j, i]) - float(fhocnn[j, i]) - float(fsnow[j, i]) * Lfresh - C0) * dt
        fe = abs(efinal[ij] - einit[ij] - einp) / dt
        if fe > FERRMAX:
            return (7, i + 1, j + 1)

    # ---- the fluxes to the ocean (:482-503) ----
    for ij in R:
        i, j = I[ij], J[ij]
        dhi = hin[ij] - worki[ij]
        dhs = hsn[ij] - works[ij] - hsn_new[ij]
        freshn[j, i] = float(freshn[j, i]) + float(evapn[j, i]) - (rhoi * dhi + rhos * dhs) / dt
        fsaltn[j, i] = float(fsaltn[j, i]) - rhoi * dhi * p["salinity"] * P001 / dt
        fhocnn[j, i] = float(fhocnn[j, i]) + C0
        if hin[ij] == C0:
            info["vanished"] += 1
            if topo:
                before = float(y["fpond"][b, j, i])
                y["fpond"][b, j, i] = before - float(aicen[j, i]) * float(trcrn[tr["nt_apnd"] - 1, j, i]) * float(trcrn[tr["nt_hpnd"] - 1, j, i])
                if y["fpond"][b, j, i] != before:
                    info["fpond_changed"] += 1

    # ---- update_state_vthermo, Tf = Tbot ----
    for ij in R:
        i, j = I[ij], J[ij]
        if hin[ij] > C0:
            vicen[j, i] = float(aicen[j, i]) * hin[ij]
            vsnon[j, i] = float(aicen[j, i]) * hsn[ij]
            trcrn[nt_Tsfc, j, i] = Tsf[ij]
        else:
            aicen[j, i] = C0
            vicen[j, i] = C0
            vsnon[j, i] = C0
            trcrn[nt_Tsfc, j, i] = Tbot[j, i]
    for k in range(nilyr):
        for ij in R:
            trcrn[nt_qice + k, J[ij], I[ij]] = zqin[ij, k] if hin[ij] > C0 else C0
    for k in range(nslyr):
        for ij in R:
            trcrn[nt_qsno + k, J[ij], I[ij]] = zqsn[ij, k] if hin[ij] > C0 else C0
    return None


def step(blocks, tmask, p, y, iters=None):
    """every block and category as step_therm1 runs them: block outside, category inside (ice_step_mod.F90:364-540).  blocks: (ilo, ihi, jlo,
    jhi) 1-based; y: dict of the arrays, rewritten in place.  Returns (infos per block, stop): stop None or (reason, block, category, i, j)"""
    ncat = y["aicen"].shape[1]
    infos = []
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        info = {k: 0 for k in INFO_KEYS}
        infos.append(info)
        listed_any = np.zeros(y["aicen"].shape[2:], dtype=bool)
        lists = []
        for n in range(ncat):
            for q in OUT15:
                y[q][b, n] = 0.0
            J, I = [], []
            for j in range(jlo - 1, jhi):
                for i in range(ilo - 1, ihi):
                    if tmask[b, j, i] and y["aicen"][b, n, j, i] > PUNY:
                        J.append(j); I.append(i)
                        listed_any[j, i] = True
            lists.append((J, I))
        for n in range(ncat):
            J, I = lists[n]
            m = np.zeros_like(listed_any)
            m[J, I] = True
            info["unlisted_in_ice_cell"] += int((listed_any & ~m).sum())
            info["cells"] += len(J)
            if not J:
                continue
            # (the list is taken from the aicen of entry: a category changes its own area only, and only to zero)
            stop = thermo_vertical(J, I, p, y, b, n, info, iters)
            if stop is not None:
                return infos, (stop[0], b + 1, n + 1, stop[1], stop[2])
    return infos, None
