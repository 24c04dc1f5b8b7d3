"""numpy restatement of linear_itd (source/ice_therm_itd.F90:69-859 with fit_line :871-958) as step_therm2 calls it
(source/ice_step_mod.F90:821-871, kitd = 1), written from the Fortran and independent of the HIP code: block by block, in the Fortran's
loop and operation order, with p333 = c1 / c3 and p666 = c2 / c3 as ice_constants defines them.  shift_ice and compute_tracers are
tests/npitd.py's, which tests/test_itd_ref.py holds bit for bit to the reference's own output (one boundary per call there; here all
ncat - 1 boundaries go into one call).  fit_line, the boundary integrals and the whole call are PINNED to reference-built output:
tests/test_therm2_ref.py holds this file bit for bit to the records of the reference's own compiled linear_itd
(tests/golden/ref_litd_*.npz, made by tests/golden/make_ref_therm2.py from oracle/ref/Makefile, target therm2).

The l_conservation_check blocks (compile-time .false.) are left out.  Stated departures, shared with evpk_linear_itd (include/evpk.h):
the cell list takes physical cells with tmask and aice > puny; a boundary left with donor = 0 and daice > 0 (a negative vicen under
aicen > puny) moves nothing, where the reference would index category 0.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx).
"""
from __future__ import annotations

import numpy as np

from . import npitd
from .npitd import PUNY, Tr

F = np.float64
C0, C1, C2, C3, C6, P5 = F(0.0), F(1.0), F(2.0), F(3.0), F(6.0), F(0.5)
P333, P666 = C1 / C3, C2 / C3
HIN_TOP = 999.9                                     # hin_max(ncat) inside linear_itd (:208)

INFO_KEYS = ["up", "down", "hb_both", "hb_lower_only", "hb_upper_only", "hb_none", "flag_hn_ge_hb", "flag_hn1_le_hb", "flag_hb_gt_next",
             "flag_hb_lt_prev", "fit_left", "fit_mid", "fit_right", "fit_flat", "melt_clamped", "melt_unclamped", "melt_none", "dh0_ge_0",
             "small_da", "small_dv", "whole_da", "whole_dv", "hi_min", "no_shift", "unlisted", "listed", "remapped", "fpond_changed"]


def _min(x, y):
    return y if y < x else x


def _max(x, y):
    return y if y > x else x


def fit_line(a, hice, hbL, hbR, info):
    """one cell of fit_line (:917-956): returns g0, g1, hL, hR"""
    if a > PUNY and hbR - hbL > PUNY:
        hL, hR = hbL, hbR
        h13 = P333 * (C2 * hL + hR)
        h23 = P333 * (hL + C2 * hR)
        if hice < h13:
            hR = C3 * hice - C2 * hL
            info["fit_left"] += 1
        elif hice > h23:
            hL = C3 * hice - C2 * hR
            info["fit_right"] += 1
        else:
            info["fit_mid"] += 1
        dhr = C1 / (hR - hL)
        wk1 = C6 * a * dhr
        wk2 = (hice - hL) * dhr
        g0 = wk1 * (P666 - wk2)
        g1 = C2 * dhr * wk1 * (wk2 - P5)
        return g0, g1, hL, hR
    if a > PUNY:
        info["fit_flat"] += 1
    return C0, C0, C0, C0


def linear_itd_block(J, I, ntrcr, dep, tr, hin_max, hi_min, k, ai, vi, a, v, s, t, aice, aice0, fpond, info):
    """one linear_itd call on the listed cells (J, I) of one block.  ai, vi, a, v, s (ncat, ny, nx); t (ncat, ntrcr_dim, ny, nx);
    aice, aice0, fpond (ny, nx).  Returns (reason, i, j) or None."""
    ncat, ic = a.shape[0], len(J)
    hin = np.array(hin_max, dtype=np.float64)
    hin[ncat] = HIN_TOP
    hi_min = F(hi_min)
    rl = F(k["rhos"]) * F(k["Lfresh"])
    remap = np.ones(ic, dtype=bool)
    hicen = np.zeros((ic, ncat))
    donor = np.zeros((ic, ncat), dtype=np.int64)
    daice = np.zeros((ic, ncat))
    dvice = np.zeros((ic, ncat))
    with np.errstate(all="ignore"):
        for m in range(ic):
            j, i = J[m], I[m]
            hi0 = np.zeros(ncat); h = np.zeros(ncat); dh = np.zeros(ncat)
            for n in range(ncat):                                                       # :308-328
                hi0[n] = vi[n, j, i] / ai[n, j, i] if ai[n, j, i] > PUNY else C0
                if a[n, j, i] > PUNY:
                    h[n] = v[n, j, i] / a[n, j, i]
                    dh[n] = h[n] - hi0[n]
            hb = np.zeros(ncat + 1)
            hb[0] = hin[0]
            for n in range(1, ncat):                                                    # boundary n between categories n and n + 1 (:339-436)
                lo, up = n - 1, n
                if hi0[lo] > PUNY and hi0[up] > PUNY:
                    slope = (dh[up] - dh[lo]) / (hi0[up] - hi0[lo])
                    hb[n] = hin[n] + dh[lo] + slope * (hin[n] - hi0[lo])
                    info["hb_both"] += 1
                elif hi0[lo] > PUNY:
                    hb[n] = hin[n] + dh[lo]
                    info["hb_lower_only"] += 1
                elif hi0[up] > PUNY:
                    hb[n] = hin[n] + dh[up]
                    info["hb_upper_only"] += 1
                else:
                    hb[n] = hin[n]
                    info["hb_none"] += 1
                if a[lo, j, i] > PUNY and h[lo] >= hb[n]:
                    remap[m] = False
                    info["flag_hn_ge_hb"] += 1
                elif a[up, j, i] > PUNY and h[up] <= hb[n]:
                    remap[m] = False
                    info["flag_hn1_le_hb"] += 1
                if hb[n] > hin[n + 1]:
                    remap[m] = False
                    info["flag_hb_gt_next"] += 1
                if hb[n] < hin[n - 1]:
                    remap[m] = False
                    info["flag_hb_lt_prev"] += 1
            if a[ncat - 1, j, i] > PUNY:                                                # :445-454
                hb[ncat] = C3 * h[ncat - 1] - C2 * hb[ncat - 1]
            else:
                hb[ncat] = hin[ncat]
            hb[ncat] = _max(hb[ncat], hin[ncat - 1])
            hicen[m] = h
            if not remap[m]:
                continue
            info["remapped"] += 1
            scratch = {q: 0 for q in INFO_KEYS}
            g0 = np.zeros(ncat); g1 = np.zeros(ncat); hL = np.zeros(ncat); hR = np.zeros(ncat)
            g0[0], g1[0], hL[0], hR[0] = fit_line(a[0, j, i], hi0[0], hb[0], hin[1], scratch)       # :482-492
            if a[0, j, i] > PUNY:                                                       # :501-548
                dh0 = dh[0]
                if dh0 < C0:
                    dh0 = _min(-dh0, hin[1])
                    etamax = _min(dh0, hR[0]) - hL[0]
                    if etamax > C0:
                        x1 = etamax
                        x2 = P5 * etamax * etamax
                        da0 = g1[0] * x2 + g0[0] * x1
                        damax = a[0, j, i] * (C1 - h[0] / hi0[0])
                        info["melt_clamped" if damax < da0 else "melt_unclamped"] += 1
                        da0 = _min(da0, damax)
                        h[0] = h[0] * a[0, j, i] / (a[0, j, i] - da0)
                        a[0, j, i] = a[0, j, i] - da0
                        if tr.tr_pond_topo:
                            f0 = fpond[j, i]
                            fpond[j, i] = fpond[j, i] - (da0 * t[0, tr.nt_apnd - 1, j, i] * t[0, tr.nt_hpnd - 1, j, i])
                            info["fpond_changed"] += int(fpond[j, i] != f0)
                    else:
                        info["melt_none"] += 1
                else:
                    hb[0] = _min(dh0, hin[1])
                    info["dh0_ge_0"] += 1
            hicen[m] = h
            for n in range(ncat):                                                       # :554-563
                g0[n], g1[n], hL[n], hR[n] = fit_line(a[n, j, i], h[n], hb[n], hb[n + 1], info)
            for n in range(1, ncat):                                                    # :577-647
                q = n - 1                                                               # the column of donor / daice / dvice
                if hb[n] > hin[n]:
                    nd = n - 1
                    etamin = _max(hin[n], hL[nd]) - hL[nd]
                    etamax = _min(hb[n], hR[nd]) - hL[nd]
                else:
                    nd = n
                    etamin = C0
                    etamax = _min(hin[n], hR[nd]) - hL[nd]
                donor[m, q] = nd + 1
                if etamax > etamin:
                    x1 = etamax - etamin
                    wk1 = etamin * etamin
                    wk2 = etamax * etamax
                    x2 = P5 * (wk2 - wk1)
                    wk1 = wk1 * etamin
                    wk2 = wk2 * etamax
                    x3 = P333 * (wk2 - wk1)
                    daice[m, q] = g1[nd] * x2 + g0[nd] * x1
                    dvice[m, q] = g1[nd] * x3 + g0[nd] * x2 + daice[m, q] * hL[nd]
                and_, vnd = a[nd, j, i], v[nd, j, i]
                if daice[m, q] < and_ * PUNY:
                    info["small_da"] += int(daice[m, q] != 0.0)
                    daice[m, q] = 0.0; dvice[m, q] = 0.0; donor[m, q] = 0
                if dvice[m, q] < vnd * PUNY:
                    info["small_dv"] += int(donor[m, q] != 0)
                    daice[m, q] = 0.0; dvice[m, q] = 0.0; donor[m, q] = 0
                if daice[m, q] > and_ * (C1 - PUNY):
                    info["whole_da"] += int(donor[m, q] != 0)
                    daice[m, q] = and_; dvice[m, q] = vnd
                if dvice[m, q] > vnd * (C1 - PUNY):
                    info["whole_dv"] += int(donor[m, q] != 0 and daice[m, q] != and_)
                    daice[m, q] = and_; dvice[m, q] = vnd
                if donor[m, q] == 0:                                                    # (departure: the reference would index category 0)
                    daice[m, q] = 0.0; dvice[m, q] = 0.0
                elif daice[m, q] > 0.0:
                    info["up" if nd == n - 1 else "down"] += 1
    info["no_shift"] += int((~(daice > 0.0).any(axis=1)).sum())
    R = np.nonzero(remap)[0]
    for n in range(ncat):                                                               # :659-667
        for l in range(tr.nslyr):
            t[n, tr.nt_qsno - 1 + l, J[R], I[R]] = t[n, tr.nt_qsno - 1 + l, J[R], I[R]] + rl
    stop = npitd.shift_ice(J, I, ntrcr, dep, tr, a, v, s, t, hicen, donor, daice, dvice, k["Tocnfrz"])
    for n in range(ncat):                                                               # :682-690
        for l in range(tr.nslyr):
            t[n, tr.nt_qsno - 1 + l, J[R], I[R]] = t[n, tr.nt_qsno - 1 + l, J[R], I[R]] - rl
    if stop:
        return stop
    with np.errstate(all="ignore"):
        for m in R:                                                                     # :701-718
            j, i = J[m], I[m]
            if hi_min > C0 and a[0, j, i] > PUNY and hicen[m, 0] < hi_min:
                da0 = a[0, j, i] * (C1 - hicen[m, 0] / hi_min)
                a[0, j, i] = a[0, j, i] - da0
                hicen[m, 0] = hi_min
                info["hi_min"] += 1
                if tr.tr_pond_topo:
                    f0 = fpond[j, i]
                    fpond[j, i] = fpond[j, i] - (da0 * t[0, tr.nt_apnd - 1, j, i] * t[0, tr.nt_hpnd - 1, j, i])
                    info["fpond_changed"] += int(fpond[j, i] != f0)
    aggregate_area(a, aice, aice0)
    return None


def aggregate_area(a, aice, aice0):
    aice[:] = 0.0                                                                       # ice_itd.F90:489-506
    for n in range(a.shape[0]):
        aice[:] = aice + a[n]
    aice0[:] = np.maximum(1.0 - aice, 0.0)


def linear_itd(blocks, tmask, ntrcr, dep, tr, hin_max, hi_min, k, aicen_init, vicen_init, aicen, vicen, vsnon, trcrn, aice, aice0,
               fpond=None):
    """step_therm2:821-871 for every block in turn.  tmask (nb, ny, nx) int.  Returns (infos, stop): one info record of counts per block
    (INFO_KEYS; 'listed' 0 for a block that is not touched), stop = (reason, block, i, j) of the lowest block that stops, or None."""
    tr = tr if isinstance(tr, Tr) else Tr(tr)
    nb, ncat, ny, nx = aicen.shape
    if trcrn is None:
        trcrn = np.zeros((nb, ncat, 0, ny, nx))
    infos, stop = [], None
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        info = {q: 0 for q in INFO_KEYS}
        infos.append(info)
        aggregate_area(aicen[b], aice[b], aice0[b])
        phys = [(j, i) for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi)]
        lst = [(j, i) for j, i in phys if tmask[b, j, i] != 0 and aice[b, j, i] > PUNY]
        if not lst:
            continue
        info["listed"] = len(lst)
        info["unlisted"] = sum(1 for j, i in phys if tmask[b, j, i] != 0) - len(lst)
        J = np.array([c[0] for c in lst], dtype=np.int64)
        I = np.array([c[1] for c in lst], dtype=np.int64)
        fp = fpond[b] if fpond is not None else None
        st = linear_itd_block(J, I, ntrcr, dep, tr, hin_max, hi_min, k, aicen_init[b], vicen_init[b], aicen[b], vicen[b], vsnon[b], trcrn[b],
                              aice[b], aice0[b], fp, info)
        if st and stop is None:
            stop = (st[0], b + 1, st[1], st[2])
    return infos, stop
