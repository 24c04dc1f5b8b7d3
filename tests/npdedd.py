"""numpy restatement of the Delta-Eddington shortwave of ice_step, written from the Fortran -- the checker of evpk_step_radiation_dedd
(tests/test_dedd_gpu.py), independent of the HIP code:
  run_dEdd          source/ice_shortwave.F90:1251-1577 per category as the reference runs it, with shortwave_dEdd_set_snow (:3782-3883),
                    shortwave_dEdd_set_pond (:3893-3958), shortwave_dEdd (:1607-2024), compute_dEdd (:2034-3261), solution_dEdd (:3270-3772)
  coupling_prep     the albedo lines, drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586

Parity: run_dEdd and below are held to reference-built records (tests/golden/ref_sw_d_*.npz, tests/test_shortwave_ref.py: bit for bit on
LIBM); the call order and the coupling_prep lines are held to the Fortran by reading.

Vectorised over the listed cells of one category of one block (the Fortran's ij loops); the loops over surface types, bands, layers and
Gaussian angles are the Fortran's.  Every numpy operation is one IEEE operation per element, in the Fortran's order; a branch is a mask
and a select.  The math function is a parameter: PORTS (dev_exp_v, the array version of npridge.dev_exp: the device's bits) or LIBM
(math.exp).  min / max are a comparison and a select.  Stated departures, shared with the device (include/evpk.h): the cell lists require
tmask; a cell that is not listed holds zero in apeffn and snowfracn; compute_coszen stays with the caller (coszen is in / out).
The tables below are this file's own copy, typed from the Fortran in ITS layout (one row per radius, the three bands side by side).

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), Sswabsn (nb, ncat, nslyr, ny,
nx), Iswabsn (nb, ncat, nilyr, ny, nx), fswpenln (nb, ncat, nilyr + 1, ny, nx) or None.
"""
from __future__ import annotations

import math

import numpy as np

PUNY = 1.0e-11
C0, C1, C2, C3, C4, P5, P25, P75, C1P5, P01 = 0.0, 1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 0.75, 1.5, 0.01
NSPINT, NMBRAD, NGMAX = 3, 32, 8

# ---- this file's copy of the tables (source/ice_shortwave.F90) ----
RSNW_TAB = np.array([5., 7., 10., 15., 20., 30., 40., 50., 65., 80., 100., 120., 140., 170., 200., 240., 290., 350., 420., 500., 570., 660.,
                     760., 870., 1000., 1100., 1250., 1400., 1600., 1800., 2000., 2500.])                               # :2368-2376
_QS = """2.131798 2.187756 2.267358  2.104499 2.148345 2.236078  2.081580 2.116885 2.175067  2.062595 2.088937 2.130242
2.051403 2.072422 2.106610  2.039223 2.055389 2.080586  2.032383 2.045751 2.066394  2.027920 2.039388 2.057224
2.023444 2.033137 2.048055  2.020412 2.028840 2.041874  2.017608 2.024863 2.036046  2.015592 2.022021 2.031954
2.014083 2.019887 2.028853  2.012368 2.017471 2.025353  2.011092 2.015675 2.022759  2.009837 2.013897 2.020168
2.008668 2.012252 2.017781  2.007627 2.010813 2.015678  2.006764 2.009577 2.013880  2.006037 2.008520 2.012382
2.005528 2.007807 2.011307  2.005025 2.007079 2.010280  2.004562 2.006440 2.009333  2.004155 2.005898 2.008523
2.003794 2.005379 2.007795  2.003555 2.005041 2.007329  2.003264 2.004624 2.006729  2.003037 2.004291 2.006230
2.002776 2.003929 2.005700  2.002590 2.003627 2.005276  2.002395 2.003391 2.004904  2.002071 2.002922 2.004241"""      # :2380-2413
_WS = """0.9999994 0.9999673 0.9954589  0.9999992 0.9999547 0.9938576  0.9999990 0.9999382 0.9917989  0.9999985 0.9999123 0.9889724
0.9999979 0.9998844 0.9866190  0.9999970 0.9998317 0.9823021  0.9999960 0.9997800 0.9785269  0.9999951 0.9997288 0.9751601
0.9999936 0.9996531 0.9706974  0.9999922 0.9995783 0.9667577  0.9999903 0.9994798 0.9621007  0.9999885 0.9993825 0.9579541
0.9999866 0.9992862 0.9541924  0.9999838 0.9991434 0.9490959  0.9999810 0.9990025 0.9444940  0.9999772 0.9988171 0.9389141
0.9999726 0.9985890 0.9325819  0.9999670 0.9983199 0.9256405  0.9999605 0.9980117 0.9181533  0.9999530 0.9976663 0.9101540
0.9999465 0.9973693 0.9035031  0.9999382 0.9969939 0.8953134  0.9999289 0.9965848 0.8865789  0.9999188 0.9961434 0.8773350
0.9999068 0.9956323 0.8668233  0.9998975 0.9952464 0.8589990  0.9998837 0.9946782 0.8476493  0.9998699 0.9941218 0.8367318
0.9998515 0.9933966 0.8227881  0.9998332 0.9926888 0.8095131  0.9998148 0.9919968 0.7968620  0.9997691 0.9903277 0.7677887"""  # :2417-2450
_GS = """0.859913 0.848003 0.824415  0.867130 0.858150 0.848445  0.873381 0.867221 0.861714  0.878368 0.874879 0.874036
0.881462 0.879661 0.881299  0.884361 0.883903 0.890184  0.885937 0.886256 0.895393  0.886931 0.887769 0.899072
0.887894 0.889255 0.903285  0.888515 0.890236 0.906588  0.889073 0.891127 0.910152  0.889452 0.891750 0.913100
0.889730 0.892213 0.915621  0.890026 0.892723 0.918831  0.890238 0.893099 0.921540  0.890441 0.893474 0.924581
0.890618 0.893816 0.927701  0.890762 0.894123 0.930737  0.890881 0.894397 0.933568  0.890975 0.894645 0.936148
0.891035 0.894822 0.937989  0.891097 0.895020 0.939949  0.891147 0.895212 0.941727  0.891189 0.895399 0.943339
0.891225 0.895601 0.944915  0.891248 0.895745 0.945950  0.891277 0.895951 0.947288  0.891299 0.896142 0.948438
0.891323 0.896388 0.949762  0.891340 0.896623 0.950916  0.891356 0.896851 0.951945  0.891386 0.897399 0.954156"""      # :2454-2487


def _rows(text):
    return np.array([float(w) for w in text.split()]).reshape(NMBRAD, NSPINT)          # [radius, band], the Fortran's order in memory


QS_TAB, WS_TAB, GS_TAB = _rows(_QS), _rows(_WS), _rows(_GS)
MEAN = dict(                                                                            # :2496-2532, [band]
    ki_ssl_mn=[1000.1, 1003.7, 7042.], wi_ssl_mn=[.9999, .9963, .9088], gi_ssl_mn=[.94, .94, .94],
    ki_dl_mn=[100.2, 107.7, 1309.], wi_dl_mn=[.9980, .9287, .0305], gi_dl_mn=[.94, .94, .94],
    ki_int_mn=[20.2, 27.7, 1445.], wi_int_mn=[.9901, .7223, .0277], gi_int_mn=[.94, .94, .94],
    ki_p_ssl_mn=[70.2, 77.7, 1309.], wi_p_ssl_mn=[.9972, .9009, .0305], gi_p_ssl_mn=[.94, .94, .94],
    ki_p_int_mn=[20.2, 27.7, 1445.], wi_p_int_mn=[.9901, .7223, .0277], gi_p_int_mn=[.94, .94, .94],
    kw=[0.20, 12.0, 729.], ww=[0.00, 0.00, 0.00], gw=[0.00, 0.00, 0.00])
GAUSPT = [.9894009, .9445750, .8656312, .7554044, .6178762, .4580168, .2816036, .0950125]        # :3475-3485
GAUSWT = [.0271525, .0622535, .0951585, .1246290, .1495960, .1691565, .1826034, .1894506]
# the scalars, in the order of the library's "scalars" table (cice5_amd.evpk.DEDD_SCALAR_NAMES)
HI_SSL, HS_SSL, HPMIN, HP0, HS_MIN, TIMELT = 0.050, 0.040, 0.005, 0.200, 1.e-4, 0.0    # :139-144, ice_constants.F90:91, :65
RSNW_FRESH, RSNW_NONMELT, RSNW_SIG, DT_PND, PND_FAC = 100., 500., 250., 1.0, 0.3       # :3832-3834, :3932, :3954
CP67, CP78, CP01 = 0.67, 0.78, 0.01                                                    # :2262-2266
RHOI, FR_MAX, FR_MIN, FP_ICE, FM_ICE, FP_PND, FM_PND = 917.0, 1.00, 0.80, 0.15, 0.15, 2.00, 0.50                       # :2535-2543
TRMIN, REFINDX, CP063, CP455 = 0.001, 1.310, 0.063, 0.455                              # :3397, :3431-3433
EXP_MIN = float.fromhex("0x1.7cd79b5647c9bp-15")                                       # the double nearest to e^-10 (:1376, :1383)
SCALARS = [HI_SSL, HS_SSL, HPMIN, HP0, HS_MIN, TIMELT, RSNW_FRESH, RSNW_NONMELT, RSNW_SIG, DT_PND, PND_FAC, CP67, CP78, CP01, RHOI, FR_MAX,
           FR_MIN, FP_ICE, FM_ICE, FP_PND, FM_PND, TRMIN, REFINDX, CP063, CP455, EXP_MIN, 30.0, 0.50]

NAMELIST = ["R_ice", "R_pnd", "R_snw", "dT_mlt", "rsnw_mlt", "kalg", "hs0", "pndaspect", "awtvdr", "awtidr", "awtvdf", "awtidf"]
OUT3D = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun", "albpndn", "apeffn", "snowfracn"]
OUT_LAYERS = ["Sswabsn", "Iswabsn", "fswpenln"]
OUT2D = ["alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "scale_factor", "albpnd", "apeff_ai"]
INFO_KEYS = ["listed", "lit", "night_on_ice", "three_types", "fi_nonpos", "hs_lt_hsmin", "hs_mid", "hs_ge_hs0", "hs0_off", "hp_lt_hpmin",
             "hp_trans", "hp_gt_hp0", "trmin_skipped", "extins_clamped", "trnlay_clamped", "dfdir_clamped", "dfdif_clamped", "coszen_neg_lit",
             "coszen_gt_p01", "coszen_small", "fnidr_zero_lit", "fT_zero", "fT_mid", "tab_low", "tab_high", "tab_inside", "rsnw_nm_fresh",
             "R_ice_neg", "R_pnd_neg", "kalg_zero", "set_pond", "cesm_infiltrated", "exp_calls"]


def dev_exp_v(x):
    """npridge.dev_exp, element for element, on an array: the three range-reduction branches are masks"""
    ln2HI, ln2LO, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5_ = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        big = ax > 0.34657359027997264
        mid = big & (ax < 1.0397207708399179)
        tiny = ~big & (ax < 3.725290298461914e-09)
        half = np.where(x < 0.0, -0.5, 0.5)
        kf = np.where(mid, np.where(x < 0.0, -1.0, 1.0), np.where(big, np.trunc(invln2 * x + half), 0.0))
        kf = np.where(np.isfinite(kf), kf, 0.0)
        k = np.clip(kf, -2.0e9, 2.0e9).astype(np.int64)
        t = k.astype(np.float64)
        hi = np.where(big, x - t * ln2HI, 0.0)
        lo = np.where(big, t * ln2LO, 0.0)
        xr = np.where(big, hi - lo, x)
        tt = xr * xr
        c = xr - tt * (P1 + tt * (P2 + tt * (P3 + tt * (P4 + tt * P5_))))
        r0 = 1.0 - ((xr * c) / (c - 2.0) - xr)
        y = 1.0 - ((lo - (xr * c) / (2.0 - c)) - hi)
        r = np.where(k == 0, r0, np.ldexp(y, np.clip(k, -5000, 5000).astype(np.int32)))
        return np.where(tiny, 1.0 + x, r)


def _libm_exp(x):
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.exp(v) for v in x.ravel()]).reshape(x.shape)


PORTS = dict(exp=dev_exp_v)
LIBM = dict(exp=_libm_exp)


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


def iops(p, info=None):
    """the R_ice / R_pnd adjustment of compute_dEdd (:2655-2721): dict of [band] lists ki_ssl .. gi_p_int"""
    o = {}

    def tune(name, R, fp, fm):
        k, w, g = [], [], []
        for ns in range(NSPINT):
            kmn, wmn = MEAN["k" + name + "_mn"][ns], MEAN["w" + name + "_mn"][ns]
            if R >= C0:
                sigp = kmn * wmn * (C1 + fp * R)
            else:
                sigp = kmn * wmn * (C1 + fm * R)
                sigp = sigp if sigp > C0 else C0
            k.append(sigp + kmn * (C1 - wmn))
            w.append(sigp / k[-1])
            g.append(MEAN["g" + name + "_mn"][ns])
        o["k" + name], o["w" + name], o["g" + name] = k, w, g
    for name in ("i_ssl", "i_dl", "i_int"):
        tune(name, p["R_ice"], FP_ICE, FM_ICE)
    for name in ("i_p_ssl", "i_p_int"):
        tune(name, p["R_pnd"], FP_PND, FM_PND)
    if info is not None:
        info["R_ice_neg"] += int(p["R_ice"] < C0)
        info["R_pnd_neg"] += int(p["R_pnd"] < C0)
    return o


def solution_dEdd(srftyp, nslyr, nilyr, coszen, tau, w0, g, albodr, albodf, exp, info):
    """:3270-3772 on m columns: tau, w0, g lists of klev + 1 arrays; returns the six interface lists (0 .. klevp)"""
    klev = nslyr + nilyr + 1
    klevp = klev + 1
    m = coszen.shape[0]
    z = lambda: np.zeros(m)
    alpha = lambda w, uu, gg, e: P75 * w * uu * ((C1 + gg * (C1 - w)) / (C1 - e * e * uu * uu))
    agamm = lambda w, uu, gg, e: P5 * w * ((C1 + C3 * gg * (C1 - w) * uu * uu) / (C1 - e * e * uu * uu))
    n_ = lambda uu, et: ((uu + C1) * (uu + C1) / et) - ((uu - C1) * (uu - C1) * et)
    u_ = lambda w, gg, e: C1P5 * (C1 - w * gg) / e
    el = lambda w, gg: np.sqrt(C3 * (C1 - w) * (C1 - w * gg))
    taus = lambda w, f, t: (C1 - w * f) * t
    omgs = lambda w, f: (C1 - f) * w / (C1 - w * f)
    asys = lambda gg, f: (gg - f) / (C1 - f)
    trndir, trntdr, trndif, rupdir, rupdif, rdndif = ([z() for _ in range(klevp + 1)] for _ in range(6))
    trndir[0] = z() + C1
    trntdr[0] = z() + C1
    trndif[0] = z() + C1
    mu0 = _max(coszen, P01)
    mu0nij = np.sqrt(C1 - ((C1 - mu0 * mu0) / (REFINDX * REFINDX)))
    kfrsnl = nslyr + 2 if srftyp < 2 else 0
    rdir, rdif_a, rdif_b, tdir, tdif_a, tdif_b, trnlay = ([None] * (klev + 1) for _ in range(7))
    for k in range(klev + 1):
        on = trntdr[k] > TRMIN
        info["trmin_skipped"] += int((~on).sum())
        non = int(on.sum())
        tautot, wtot, gtot = tau[k], w0[k], g[k]
        ftot = gtot * gtot
        ts = taus(wtot, ftot, tautot)
        ws = omgs(wtot, ftot)
        gs = asys(gtot, ftot)
        lm = el(ws, gs)
        ue = u_(ws, gs, lm)
        mu0n = mu0 if (srftyp < 2 and k < kfrsnl) else mu0nij
        e1 = exp(-lm * ts)
        info["extins_clamped"] += int((on & (EXP_MIN > e1)).sum())
        extins = _max(EXP_MIN, e1)
        ne = n_(ue, extins)
        rdif = (ue * ue - C1) * (C1 / extins - extins) / ne
        tdif = C4 * ue / ne
        e2 = exp(-ts / mu0n)
        info["trnlay_clamped"] += int((on & (EXP_MIN > e2)).sum())
        trn_k = _max(EXP_MIN, e2)
        alp = alpha(ws, mu0n, gs, lm)
        gam = agamm(ws, mu0n, gs, lm)
        apg = alp + gam
        amg = alp - gam
        rdr_k = apg * rdif + amg * (tdif * trn_k - C1)
        tdr_k = apg * tdif + (amg * rdif - apg + C1) * trn_k
        R1, T1 = rdif, tdif
        swt, smr, smt = C0, z(), z()
        for ng in range(NGMAX):
            mu, gwt = GAUSPT[ng], GAUSWT[ng]
            swt = swt + mu * gwt
            trn = _max(EXP_MIN, exp(-ts / mu))
            alp = alpha(ws, mu, gs, lm)
            gam = agamm(ws, mu, gs, lm)
            apg = alp + gam
            amg = alp - gam
            rdr = apg * R1 + amg * T1 * trn - amg
            tdr = apg * T1 + amg * R1 * trn - apg * trn + trn
            smr = smr + mu * rdr * gwt
            smt = smt + mu * tdr * gwt
        info["exp_calls"] += (2 + NGMAX) * non
        rdif_ak = smr / swt
        tdif_ak = smt / swt
        rdif_bk = rdif_ak
        tdif_bk = tdif_ak
        if k == kfrsnl:
            R1 = (mu0 - REFINDX * mu0n) / (mu0 + REFINDX * mu0n)
            R2 = (REFINDX * mu0 - mu0n) / (REFINDX * mu0 + mu0n)
            T1 = C2 * mu0 / (mu0 + REFINDX * mu0n)
            T2 = C2 * mu0 / (REFINDX * mu0 + mu0n)
            Rf_dir_a = P5 * (R1 * R1 + R2 * R2)
            Tf_dir_a = P5 * (T1 * T1 + T2 * T2) * REFINDX * mu0n / mu0
            Rf_dif_a = CP063
            Tf_dif_a = C1 - Rf_dif_a
            Rf_dif_b = CP455
            Tf_dif_b = C1 - Rf_dif_b
            rintfc = C1 / (C1 - Rf_dif_b * rdif_ak)
            tdr_new = Tf_dir_a * tdr_k + Tf_dir_a * rdr_k * Rf_dif_b * rintfc * tdif_ak
            rdr_new = Rf_dir_a + Tf_dir_a * rdr_k * rintfc * Tf_dif_b
            rdif_a_new = Rf_dif_a + Tf_dif_a * rdif_ak * rintfc * Tf_dif_b
            rdif_bk = rdif_bk + tdif_bk * Rf_dif_b * rintfc * tdif_ak
            tdif_a_new = tdif_ak * rintfc * Tf_dif_a
            tdif_bk = tdif_bk * rintfc * Tf_dif_b
            tdr_k, rdr_k, rdif_ak, tdif_ak = tdr_new, rdr_new, rdif_a_new, tdif_a_new
            trn_k = Tf_dir_a * trn_k
        sel = lambda v: np.where(on, v, C0)
        rdir[k], rdif_a[k], rdif_b[k], tdir[k], tdif_a[k], tdif_b[k], trnlay[k] = (sel(v) for v in (rdr_k, rdif_ak, rdif_bk, tdr_k, tdif_ak, tdif_bk, trn_k))
        trndir[k + 1] = trndir[k] * trnlay[k]
        refkm1 = C1 / (C1 - rdndif[k] * rdif_a[k])
        tdrrdir = trndir[k] * rdir[k]
        tdndif = trntdr[k] - trndir[k]
        trntdr[k + 1] = trndir[k] * tdir[k] + (tdndif + tdrrdir * rdndif[k]) * refkm1 * tdif_a[k]
        rdndif[k + 1] = rdif_b[k] + (tdif_b[k] * rdndif[k] * refkm1 * tdif_a[k])
        trndif[k + 1] = trndif[k] * refkm1 * tdif_a[k]
    rupdir[klevp] = z() + albodr
    rupdif[klevp] = z() + albodf
    for k in range(klev, -1, -1):
        refkp1 = C1 / (C1 - rdif_b[k] * rupdif[k + 1])
        rupdir[k] = rdir[k] + (trnlay[k] * rupdir[k + 1] + (tdir[k] - trnlay[k]) * rupdif[k + 1]) * refkp1 * tdif_b[k]
        rupdif[k] = rdif_a[k] + tdif_a[k] * rupdif[k + 1] * refkp1 * tdif_b[k]
    return trndir, trntdr, trndif, rupdir, rupdif, rdndif


def compute_dEdd(srftyp, p, io, c, exp, info):
    """:2034-3261 on the m columns of one surface type.  c: dict of 1-D arrays fnidr, coszen, swvdr, swvdf, swidr, swidf, hs, rsnw, hi, hp.
    Returns dict avdr, avdf, aidr, aidf, fsfc, fint, fthru, Sabs [nslyr], Iabs [nilyr], fthrul [nilyr + 1]"""
    nilyr, nslyr = p["tr"]["nilyr"], p["tr"]["nslyr"]
    klev = nslyr + nilyr + 1
    klevp = klev + 1
    kii = nslyr + 1
    m = c["hi"].shape[0]
    z = lambda: np.zeros(m)
    fnidr, hs, hi, hp = c["fnidr"], c["hs"], c["hi"], c["hp"]
    rnilyr = C1 / float(nilyr)
    rnslyr = C1 / float(nslyr)
    avdr, avdf, aidr, aidf, fsfc, fint, fthru = (z() for _ in range(7))
    Sabs = [z() for _ in range(nslyr)]
    Iabs = [z() for _ in range(nilyr)]
    fthrul = [z() for _ in range(nilyr + 1)]
    wghtns = [z() + C1, CP67 + (CP78 - CP67) * (C1 - fnidr), None]
    wghtns[2] = C1 - wghtns[1]
    frsnw = (FR_MAX * fnidr + FR_MIN * (C1 - fnidr)) * c["rsnw"]
    dzk = [None] * (klev + 1)
    dz = hs * rnslyr
    dzk[0] = _min(HS_SSL, dz / C2)
    dzk[1] = dz - dzk[0]
    for k in range(2, nslyr + 1):
        dzk[k] = dz
    dz = hi * rnilyr
    dz_ssl = _min(HI_SSL, hi / 30.0)
    dz_ssl = _min(dz_ssl, dz / C2)
    dzk[kii] = dz_ssl
    dzk[kii + 1] = dz - dz_ssl
    for k in range(kii + 2, klev + 1):
        dzk[k] = dz
    ksrf = 1 if srftyp == 1 else nslyr + 2
    for ns in range(NSPINT):
        tau, w0, g = [None] * (klev + 1), [None] * (klev + 1), [None] * (klev + 1)
        if srftyp == 0:
            for k in range(nslyr + 1):
                tau[k], w0[k], g[k] = z(), z(), z()
        elif srftyp == 1:
            below = frsnw < RSNW_TAB[0]
            above = ~below & (frsnw >= RSNW_TAB[NMBRAD - 1])
            Qs = np.where(below, QS_TAB[0, ns], QS_TAB[NMBRAD - 1, ns])
            ws = np.where(below, WS_TAB[0, ns], WS_TAB[NMBRAD - 1, ns])
            gs = np.where(below, GS_TAB[0, ns], GS_TAB[NMBRAD - 1, ns])
            for nr in range(1, NMBRAD):
                inside = ~below & ~above & (RSNW_TAB[nr - 1] <= frsnw) & (frsnw < RSNW_TAB[nr])
                delr = (frsnw - RSNW_TAB[nr - 1]) / (RSNW_TAB[nr] - RSNW_TAB[nr - 1])
                Qs = np.where(inside, QS_TAB[nr - 1, ns] * (C1 - delr) + QS_TAB[nr, ns] * delr, Qs)
                ws = np.where(inside, WS_TAB[nr - 1, ns] * (C1 - delr) + WS_TAB[nr, ns] * delr, ws)
                gs = np.where(inside, GS_TAB[nr - 1, ns] * (C1 - delr) + GS_TAB[nr, ns] * delr, gs)
            if ns == 0:
                info["tab_low"] += int(below.sum())
                info["tab_high"] += int(above.sum())
                info["tab_inside"] += int((~below & ~above).sum())
            ks = Qs * ((p["rhos"] / RHOI) * 3.0 / (4.0 * frsnw * 1.0e-6))
            for k in range(nslyr + 1):
                tau[k], w0[k], g[k] = ks * dzk[k], ws, gs
        else:
            dz = hp / (C1 / rnslyr + C1)
            for k in range(nslyr + 1):
                tau[k], w0[k], g[k] = MEAN["kw"][ns] * dz, z() + MEAN["ww"][ns], z() + MEAN["gw"][ns]
        if srftyp <= 1:
            k = kii
            tau[k], w0[k], g[k] = io["ki_ssl"][ns] * dzk[k], z() + io["wi_ssl"][ns], z() + io["gi_ssl"][ns]
            k = kii + 1
            fs = P25 / rnilyr
            tau[k], w0[k], g[k] = io["ki_dl"][ns] * dzk[k] * fs, z() + io["wi_dl"][ns], z() + io["gi_dl"][ns]
            for k in range(kii + 2, klev):
                tau[k], w0[k], g[k] = io["ki_int"][ns] * dzk[k], z() + io["wi_int"][ns], z() + io["gi_int"][ns]
            k = klev
            kabs = io["ki_int"][ns] * (C1 - io["wi_int"][ns])
            if ns == 0:
                kabs = kabs + p["kalg"] * (0.50 / dzk[k])
                info["kalg_zero"] += m * int(p["kalg"] == C0)
            sig = io["ki_int"][ns] * io["wi_int"][ns]
            tau[k], w0[k], g[k] = (kabs + sig) * dzk[k], z() + (sig / (sig + kabs)), z() + io["gi_int"][ns]
        else:
            k = kii
            tau[k], w0[k], g[k] = io["ki_p_ssl"][ns] * dzk[k], z() + io["wi_p_ssl"][ns], z() + io["gi_p_ssl"][ns]
            for k in range(kii + 1, klev + 1):
                tau[k], w0[k], g[k] = io["ki_p_int"][ns] * dzk[k], z() + io["wi_p_int"][ns], z() + io["gi_p_int"][ns]
            tr = (HPMIN <= hp) & (hp <= HP0)
            if ns == 0:
                info["hp_lt_hpmin"] += int((hp < HPMIN).sum())
                info["hp_trans"] += int(tr.sum())
                info["hp_gt_hp0"] += int((hp > HP0).sum())
            for k in range(kii, klev + 1):
                if k == kii:
                    sig_i = io["ki_ssl"][ns] * io["wi_ssl"][ns]
                    sig_p = io["ki_p_ssl"][ns] * io["wi_p_ssl"][ns]
                    rest = io["ki_p_ssl"][ns] * (C1 - io["wi_p_ssl"][ns])
                elif k == kii + 1:
                    fs = P25 / rnilyr
                    sig_i = io["ki_dl"][ns] * io["wi_dl"][ns] * fs
                    sig_p = io["ki_p_int"][ns] * io["wi_p_int"][ns]
                    rest = io["ki_p_int"][ns] * (C1 - io["wi_p_int"][ns])
                else:
                    sig_i = io["ki_int"][ns] * io["wi_int"][ns]
                    sig_p = io["ki_p_int"][ns] * io["wi_p_int"][ns]
                    rest = io["ki_p_int"][ns] * (C1 - io["wi_p_int"][ns])
                sig = sig_i + (sig_p - sig_i) * (hp / HP0)
                kext = sig + rest
                tau[k] = np.where(tr, kext * dzk[k], tau[k])
                w0[k] = np.where(tr, sig / kext, w0[k])
                g[k] = np.where(tr, io["gi_p_int"][ns], g[k])
        rns = float(ns)
        albodr = CP01 * (C1 - min(rns, C1))
        albodf = CP01 * (C1 - min(rns, C1))
        trndir, trntdr, trndif, rupdir, rupdif, rdndif = solution_dEdd(srftyp, nslyr, nilyr, c["coszen"], tau, w0, g, albodr, albodf, exp, info)
        dfdir, dfdif = [None] * (klevp + 1), [None] * (klevp + 1)
        for k in range(klevp + 1):
            refk = C1 / (C1 - rdndif[k] * rupdif[k])
            d = trndir[k] + (trntdr[k] - trndir[k]) * (C1 - rupdif[k]) * refk - trndir[k] * rupdir[k] * (C1 - rdndif[k]) * refk
            info["dfdir_clamped"] += int((d < PUNY).sum())
            dfdir[k] = np.where(d < PUNY, C0, d)
            d = trndif[k] * (C1 - rupdif[k]) * refk
            info["dfdif_clamped"] += int((d < PUNY).sum())
            dfdif[k] = np.where(d < PUNY, C0, d)
        if ns == 0:
            swdr, swdf = c["swvdr"], c["swvdf"]
            avdr = rupdir[0]
            avdf = rupdif[0]
            tmp_0 = dfdir[0] * swdr + dfdif[0] * swdf
            tmp_ks = dfdir[ksrf] * swdr + dfdif[ksrf] * swdf
            tmp_kl = dfdir[klevp] * swdr + dfdif[klevp] * swdf
            for k in range(nslyr + 2, klevp + 1):
                fthrul[k - nslyr - 2] = dfdir[k] * swdr + dfdif[k] * swdf
            fsfc = fsfc + tmp_0 - tmp_ks
            fint = fint + tmp_ks - tmp_kl
            fthru = fthru + tmp_kl
            if srftyp == 1:
                ki = 0
                for k in range(1, nslyr + 1):
                    km, kp = k, k + 1
                    ki += 1
                    Sabs[ki - 1] = Sabs[ki - 1] + dfdir[km] * swdr + dfdif[km] * swdf - (dfdir[kp] * swdr + dfdif[kp] * swdf)
            ki = 0
            for k in range(nslyr + 2, nslyr + 1 + nilyr + 1):
                km, kp = k, k + 1
                if srftyp == 1 and k == nslyr + 2:
                    km = k - 1
                    kp = km + 2
                ki += 1
                Iabs[ki - 1] = Iabs[ki - 1] + dfdir[km] * swdr + dfdif[km] * swdf - (dfdir[kp] * swdr + dfdif[kp] * swdf)
        else:
            swdr, swdf = c["swidr"], c["swidf"]
            aidr = aidr + rupdir[0] * wghtns[ns]
            aidf = aidf + rupdif[0] * wghtns[ns]
            tmp_0 = dfdir[0] * swdr + dfdif[0] * swdf
            tmp_ks = dfdir[ksrf] * swdr + dfdif[ksrf] * swdf
            tmp_kl = dfdir[klevp] * swdr + dfdif[klevp] * swdf
            tmp_0 = tmp_0 * wghtns[ns]
            tmp_ks = tmp_ks * wghtns[ns]
            tmp_kl = tmp_kl * wghtns[ns]
            fsfc = fsfc + tmp_0 - tmp_ks
            fint = fint + tmp_ks - tmp_kl
            fthru = fthru + tmp_kl
            if srftyp == 1:
                ki = 0
                for k in range(1, nslyr + 1):
                    km, kp = k, k + 1
                    ki += 1
                    Sabs[ki - 1] = Sabs[ki - 1] + (dfdir[km] * swdr + dfdif[km] * swdf - (dfdir[kp] * swdr + dfdif[kp] * swdf)) * wghtns[ns]
            ki = 0
            for k in range(nslyr + 2, nslyr + 1 + nilyr + 1):
                km, kp = k, k + 1
                if srftyp == 1 and k == nslyr + 2:
                    km = k - 1
                    kp = km + 2
                ki += 1
                Iabs[ki - 1] = Iabs[ki - 1] + (dfdir[km] * swdr + dfdif[km] * swdf - (dfdir[kp] * swdr + dfdif[kp] * swdf)) * wghtns[ns]
    return dict(avdr=avdr, avdf=avdf, aidr=aidr, aidf=aidf, fsfc=fsfc, fint=fint, fthru=fthru, Sabs=Sabs, Iabs=Iabs, fthrul=fthrul)


def shortwave_dEdd(p, io, y, b, n, jj, ii, fs, hs, rsnw, fp, hp, exp, info):
    """:1607-2024 on the listed cells (jj, ii) of category n of block b; writes the category's arrays of y and y["coszen"]"""
    nilyr, nslyr = p["tr"]["nilyr"], p["tr"]["nslyr"]
    m = jj.shape[0]
    z = lambda: np.zeros(m)
    aice, vice = y["aicen"][b, n][jj, ii], y["vicen"][b, n][jj, ii]
    swvdr, swvdf, swidr, swidf = (y[q][b][jj, ii] for q in ("swvdr", "swvdf", "swidr", "swidf"))
    alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, albice, albsno, albpnd = (z() for _ in range(10))
    fswpenl = [z() for _ in range(nilyr + 1)]
    Sswabs = [z() for _ in range(nslyr)]
    Iswabs = [z() for _ in range(nilyr)]
    nir = swidr + swidf
    fnidr = np.where(nir > PUNY, swidr / np.where(nir > PUNY, nir, C1), C0)
    netsw = swvdr + swidr + swvdf + swidf
    lit = netsw > PUNY
    cz_in = y["coszen"][b][jj, ii]
    info["lit"] += int(lit.sum())
    info["night_on_ice"] += int((~lit).sum())
    info["coszen_neg_lit"] += int((lit & (cz_in < C0)).sum())
    info["coszen_gt_p01"] += int((lit & (cz_in > P01)).sum())
    info["coszen_small"] += int((lit & (cz_in > PUNY) & (cz_in < P01)).sum())
    info["fnidr_zero_lit"] += int((lit & ~(nir > PUNY)).sum())
    coszen = np.where(lit, _max(PUNY, cz_in), cz_in)
    y["coszen"][b][jj, ii] = coszen
    hi = np.where(lit, vice / aice, C0)
    fi = np.where(lit, C1 - fs - fp, C0)
    conds = [lit & (fi > C0), lit & (fs > C0), lit & (fp > PUNY)]
    info["fi_nonpos"] += int((lit & ~(fi > C0)).sum())
    info["three_types"] += int((conds[0] & conds[1] & conds[2]).sum())
    frac = [fi, fs, fp]
    albs = [albice, albsno, albpnd]
    for srftyp in range(3):
        s = np.nonzero(conds[srftyp])[0]
        if s.size == 0:
            continue
        c = dict(fnidr=fnidr[s], coszen=coszen[s], swvdr=swvdr[s], swvdf=swvdf[s], swidr=swidr[s], swidf=swidf[s],
                 hs=(np.zeros(s.size) if srftyp == 0 else hs[s]), rsnw=rsnw[s], hi=hi[s], hp=hp[s])
        r = compute_dEdd(srftyp, p, io, c, exp, info)
        f = frac[srftyp][s]
        fswsfc[s] = fswsfc[s] + r["fsfc"] * f
        fswint[s] = fswint[s] + r["fint"] * f
        fswthru[s] = fswthru[s] + r["fthru"] * f
        for k in range(nslyr):
            Sswabs[k][s] = Sswabs[k][s] + r["Sabs"][k] * f
        for k in range(nilyr):
            Iswabs[k][s] = Iswabs[k][s] + r["Iabs"][k] * f
        for k in range(nilyr + 1):
            fswpenl[k][s] = fswpenl[k][s] + r["fthrul"][k] * f
        alvdr[s] = alvdr[s] + r["avdr"] * f
        alvdf[s] = alvdf[s] + r["avdf"] * f
        alidr[s] = alidr[s] + r["aidr"] * f
        alidf[s] = alidf[s] + r["aidf"] * f
        albs[srftyp][s] = albs[srftyp][s] + p["awtvdr"] * r["avdr"] + p["awtidr"] * r["aidr"] + p["awtvdf"] * r["avdf"] + p["awtidf"] * r["aidf"]
    for q, v in (("alvdrn", alvdr), ("alvdfn", alvdf), ("alidrn", alidr), ("alidfn", alidf), ("fswsfcn", fswsfc), ("fswintn", fswint),
                 ("fswthrun", fswthru), ("albicen", albice), ("albsnon", albsno), ("albpndn", albpnd)):
        y[q][b, n][jj, ii] = v
    for k in range(nslyr):
        y["Sswabsn"][b, n, k][jj, ii] = Sswabs[k]
    for k in range(nilyr):
        y["Iswabsn"][b, n, k][jj, ii] = Iswabs[k]
    if y.get("fswpenln") is not None:
        for k in range(nilyr + 1):
            y["fswpenln"][b, n, k][jj, ii] = fswpenl[k]


def step_radiation_dedd(blocks, tmask, p, y, M=PORTS):
    """step_radiation (dEdd) and the albedo lines of coupling_prep on every block.  blocks: (ilo, ihi, jlo, jhi) 1-based; p: dict of NAMELIST,
    rhos and tr (nt_Tsfc, nilyr, nslyr, tr_pond_cesm, nt_apnd, nt_hpnd); y: dict of the arrays, coszen in / out, the outputs rewritten in
    place (fswpenln may be None).  Returns the info records per block"""
    exp = M["exp"]
    tr = p["tr"]
    ncat = y["aicen"].shape[1]
    nslyr = tr["nslyr"]
    infos = []
    pen = y.get("fswpenln")
    with np.errstate(all="ignore"):
        for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
            info = {k: 0 for k in INFO_KEYS}
            infos.append(info)
            io = iops(p, info)
            for q in OUT3D + ["Sswabsn", "Iswabsn"]:                                    # ice_step_mod.F90:1408-1423, ice_shortwave.F90:1428-1429
                y[q][b] = C0
            if pen is not None:
                pen[b] = C0
            phys = np.zeros(tmask[b].shape, dtype=bool)
            phys[jlo - 1:jhi, ilo - 1:ihi] = True
            for n in range(ncat):
                jj, ii = np.nonzero(phys & tmask[b].astype(bool) & (y["aicen"][b, n] > PUNY))
                info["listed"] += int(jj.size)
                if jj.size == 0:
                    continue
                aice, vsno = y["aicen"][b, n][jj, ii], y["vsnon"][b, n][jj, ii]
                Tsfc = y["trcrn"][b, n, tr["nt_Tsfc"] - 1][jj, ii]
                # shortwave_dEdd_set_snow
                hs = vsno / aice
                fs = np.where(hs >= HS_MIN, (_min(hs / p["hs0"], C1) if p["hs0"] > PUNY else C1), C0)
                info["hs_lt_hsmin"] += int((hs < HS_MIN).sum())
                if p["hs0"] > PUNY:
                    info["hs_mid"] += int(((hs >= HS_MIN) & (hs < p["hs0"])).sum())
                    info["hs_ge_hs0"] += int(((hs >= HS_MIN) & (hs >= p["hs0"])).sum())
                else:
                    info["hs0_off"] += int((hs >= HS_MIN).sum())
                dTs = TIMELT - Tsfc
                fT = -_min(dTs / p["dT_mlt"] - C1, C0)
                info["fT_zero"] += int((fT == C0).sum())
                info["fT_mid"] += int(((fT > C0) & (fT <= C1)).sum())
                rsnw_nm = RSNW_NONMELT - p["R_snw"] * RSNW_SIG
                info["rsnw_nm_fresh"] += int(RSNW_FRESH > rsnw_nm) * int(jj.size)
                rsnw_nm = RSNW_FRESH if RSNW_FRESH > rsnw_nm else rsnw_nm
                rsnw_nm = p["rsnw_mlt"] if p["rsnw_mlt"] < rsnw_nm else rsnw_nm
                rsnw = rsnw_nm + (p["rsnw_mlt"] - rsnw_nm) * fT
                rsnw = _max(rsnw, RSNW_FRESH)
                rsnw = _min(rsnw, p["rsnw_mlt"])
                # ponds
                if tr.get("tr_pond_cesm"):
                    fp = y["trcrn"][b, n, tr["nt_apnd"] - 1][jj, ii]
                    hp = y["trcrn"][b, n, tr["nt_hpnd"] - 1][jj, ii]
                    if p["hs0"] > PUNY:
                        inf = hs >= HS_MIN
                        asnow = _min(hs / p["hs0"], C1)
                        fp = np.where(inf, (C1 - asnow) * fp, fp)
                        hp = np.where(inf, p["pndaspect"] * fp, hp)
                        info["cesm_infiltrated"] += int(inf.sum())
                    apeff = fp
                else:
                    dTs = TIMELT - Tsfc
                    fTp = -_min(dTs / DT_PND - C1, C0)
                    apeff = PND_FAC * fTp * (C1 - fs)
                    fp = np.zeros(jj.size)
                    hp = np.zeros(jj.size)
                    info["set_pond"] += int(jj.size)
                y["apeffn"][b, n][jj, ii] = apeff
                y["snowfracn"][b, n][jj, ii] = fs
                shortwave_dEdd(p, io, y, b, n, jj, ii, fs, hs, rsnw, fp, hp, exp, info)
            # coupling_prep (CICE_RunMod.F90:503-548): every cell of the block arrays
            for q in ("alvdf", "alidf", "alvdr", "alidr", "albice", "albsno", "albpnd", "apeff_ai"):
                y[q][b] = C0
            sun = y["coszen"][b] > PUNY
            for n in range(ncat):
                a = y["aicen"][b, n]
                y["alvdf"][b] = y["alvdf"][b] + y["alvdfn"][b, n] * a
                y["alidf"][b] = y["alidf"][b] + y["alidfn"][b, n] * a
                y["alvdr"][b] = y["alvdr"][b] + y["alvdrn"][b, n] * a
                y["alidr"][b] = y["alidr"][b] + y["alidrn"][b, n] * a
                y["albice"][b] = np.where(sun, y["albice"][b] + y["albicen"][b, n] * a, y["albice"][b])
                y["albsno"][b] = np.where(sun, y["albsno"][b] + y["albsnon"][b, n] * a, y["albsno"][b])
                y["albpnd"][b] = np.where(sun, y["albpnd"][b] + y["albpndn"][b, n] * a, y["albpnd"][b])
                y["apeff_ai"][b] = y["apeff_ai"][b] + y["apeffn"][b, n] * a
            y["scale_factor"][b] = (((y["swvdr"][b] * (C1 - y["alvdr"][b]) + y["swvdf"][b] * (C1 - y["alvdf"][b]))
                                     + y["swidr"][b] * (C1 - y["alidr"][b])) + y["swidf"][b] * (C1 - y["alidf"][b]))
    return infos


def exp_count(infos):
    """the exp evaluations of one call: ten per layer that the trmin cut-off lets through"""
    return sum(i["exp_calls"] for i in infos)
