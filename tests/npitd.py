"""numpy restatement of cleanup_itd (source/ice_itd.F90:1514-1769 with aggregate_area :468, rebin :516, shift_ice :815, compute_tracers
:1359, zap_small_areas :1778, zap_snow :2170, zap_snow_temperature :2274), aggregate (:246-458) and the tendency lines of step_dynamics
(ice_step_mod.F90:1183-1189), written from the Fortran and independent of the HIP code: block by block, with the reference's cell
lists, its per-block shiftflag, its loop order and its association of every product.  limit_aice = .true., heat_capacity = .true.,
no aerosols, nbtrcr = 0.  tests/test_itd_ref.py holds it bit for bit against the reference's own output (tests/golden/ref_itd_*.npz).

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), trcr (nb, ntrcr_dim, ny, nx).
Like the reference the restatement zeroes trcrn(:,:,1:ntrcr,n) of a whole block slice inside compute_tracers (:1401).
Stop reasons (evpk.h): 1 area out of bounds (:1650), 2 shift_ice negative daice (:1045), 3 negative dvice (:1066), 4 daice > aicen (:1089),
5 dvice > vicen (:1112), 6 zap: negative aicen (:1881), 7 zap: excess area (:2025).
"""
from __future__ import annotations

import numpy as np

PUNY = 1.0e-11
P001 = 0.001
CONSTANTS = dict(Tocnfrz=-1.8, ice_ref_salinity=5.0, hs_min=1.0e-4, cp_ice=2106.0, Lfresh=2.835e6 - 2.501e6, Tmin=-100.0, puny=PUNY,
                 rhoi=917.0, rhos=330.0)


class Tr:
    """the tracer indices of ice_state, 1-based, 0 = not in use"""
    NAMES = ("nt_Tsfc", "nt_qice", "nilyr", "nt_qsno", "nslyr", "nt_alvl", "nt_apnd", "nt_hpnd", "nt_fbri", "tr_pond_cesm", "tr_pond_lvl",
             "tr_pond_topo", "tr_brine")

    def __init__(self, d):
        for k in self.NAMES:
            setattr(self, k, int(d.get(k, 0)))
        self.nt_iage = int(d.get("nt_iage", 0))


def _products(dep, tr, base_a, base_v, base_s, t, it):
    """aicen * trcrn etc. with the association of shift_ice (:919-975): base first, then the parents alvl, apnd / fbri, then the tracer"""
    d = dep[it]
    x = t[it]
    if d == 0:
        return base_a * x
    if d == 1:
        return base_v * x
    if d == 2:
        return base_s * x
    if d == 2 + tr.nt_alvl:
        return base_a * t[tr.nt_alvl - 1] * x
    if d == 2 + tr.nt_apnd and (tr.tr_pond_cesm or tr.tr_pond_topo):
        return base_a * t[tr.nt_apnd - 1] * x
    if d == 2 + tr.nt_apnd and tr.tr_pond_lvl:
        return base_a * t[tr.nt_alvl - 1] * t[tr.nt_apnd - 1] * x
    if d == 2 + tr.nt_fbri:
        return base_v * t[tr.nt_fbri - 1] * x
    return None


def compute_tracers(J, I, ntrcr, dep, tr, atr, a, v, s, t, Tocnfrz):
    """atr (icells, ntrcr); a, v, s (ny, nx); t (ntrcr_dim, ny, nx) of one category"""
    t[:ntrcr] = 0.0                                                     # :1401
    an, vn, sn = a[J, I], v[J, I], s[J, I]
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(ntrcr):
            d = dep[it]
            at = atr[:, it]
            if it + 1 == tr.nt_Tsfc:
                r = np.where(an > PUNY, at / an, Tocnfrz)
            elif d == 0:
                r = np.where(an > PUNY, at / an, 0.0)
            elif d == 1:
                r = np.where(vn > 0.0, at / vn, 1.0 if it + 1 == tr.nt_fbri else 0.0)
            elif d == 2:
                r = np.where(sn > 0.0, at / sn, 0.0)
            elif d == 2 + tr.nt_alvl:
                dd = t[tr.nt_alvl - 1, J, I] * an
                r = np.where(dd > 0.0, at / dd, 0.0)
            elif d == 2 + tr.nt_apnd and (tr.tr_pond_cesm or tr.tr_pond_topo):
                dd = t[tr.nt_apnd - 1, J, I] * an
                r = np.where(dd > 0.0, at / dd, 0.0)
            elif d == 2 + tr.nt_apnd and tr.tr_pond_lvl:
                dd = t[tr.nt_alvl - 1, J, I] * t[tr.nt_apnd - 1, J, I] * an
                r = np.where(dd > 0.0, at / dd, 0.0)
            elif d == 2 + tr.nt_fbri:
                dd = t[tr.nt_fbri - 1, J, I] * vn
                r = np.where(dd > 0.0, at / dd, 0.0)
            else:
                continue
            t[it, J, I] = r


def shift_ice(J, I, ntrcr, dep, tr, a, v, s, t, hicen, donor, daice, dvice, Tocnfrz):
    """a, v, s (ncat, ny, nx); t (ncat, ntrcr_dim, ny, nx); hicen, donor, daice, dvice (icells, ncat).  Returns (reason, i, j) or None."""
    ncat, ic = a.shape[0], len(J)
    atr = np.zeros((ic, ntrcr, ncat))
    for n in range(ncat):
        tl = [t[n, k, J, I] for k in range(ntrcr)]
        for it in range(ntrcr):
            p = _products(dep, tr, a[n, J, I], v[n, J, I], s[n, J, I], tl, it)
            if p is not None:
                atr[:, it, n] = p
    for n in range(ncat - 1):
        neg_a = neg_v = big_a = big_v = False
        for m in range(ic):
            if donor[m, n] <= 0:
                continue
            nd = donor[m, n] - 1
            j, i = J[m], I[m]
            if daice[m, n] < 0.0:
                if daice[m, n] > -PUNY * a[nd, j, i]:
                    daice[m, n] = 0.0; dvice[m, n] = 0.0
                else:
                    neg_a = True
            if dvice[m, n] < 0.0:
                if dvice[m, n] > -PUNY * v[nd, j, i]:
                    daice[m, n] = 0.0; dvice[m, n] = 0.0
                else:
                    neg_v = True
            if daice[m, n] > a[nd, j, i] * (1.0 - PUNY):
                if daice[m, n] < a[nd, j, i] * (1.0 + PUNY):
                    daice[m, n] = a[nd, j, i]; dvice[m, n] = v[nd, j, i]
                else:
                    big_a = True
            if dvice[m, n] > v[nd, j, i] * (1.0 - PUNY):
                if dvice[m, n] < v[nd, j, i] * (1.0 + PUNY):
                    daice[m, n] = a[nd, j, i]; dvice[m, n] = v[nd, j, i]
                else:
                    big_v = True
        # the error loops do not exit: the LAST failing cell of the list is reported (:1040-1126)
        for flag, reason in ((neg_a, 2), (neg_v, 3), (big_a, 4), (big_v, 5)):
            if not flag:
                continue
            stop = None
            for m in range(ic):
                if donor[m, n] <= 0:
                    continue
                nd = donor[m, n] - 1
                j, i = J[m], I[m]
                bad = (daice[m, n] <= -PUNY * a[nd, j, i] if reason == 2 else dvice[m, n] <= -PUNY * v[nd, j, i] if reason == 3 else
                       daice[m, n] >= a[nd, j, i] * (1.0 + PUNY) if reason == 4 else dvice[m, n] >= v[nd, j, i] * (1.0 + PUNY))
                if bad:
                    stop = (reason, int(i) + 1, int(j) + 1)
            if stop:
                return stop
        for m in range(ic):                                             # :1132-1214
            if not daice[m, n] > 0.0:
                continue
            j, i = J[m], I[m]
            nd = donor[m, n] - 1
            worka = daice[m, n] / a[nd, j, i]
            nr = nd + 1 if nd == n else n
            a[nd, j, i] = a[nd, j, i] - daice[m, n]
            a[nr, j, i] = a[nr, j, i] + daice[m, n]
            v[nd, j, i] = v[nd, j, i] - dvice[m, n]
            v[nr, j, i] = v[nr, j, i] + dvice[m, n]
            dvsnow = s[nd, j, i] * worka
            s[nd, j, i] = s[nd, j, i] - dvsnow
            s[nr, j, i] = s[nr, j, i] + dvsnow
            tl = [t[nd, k, j, i] for k in range(ntrcr)]
            for it in range(ntrcr):
                p = _products(dep, tr, daice[m, n], dvice[m, n], dvsnow, tl, it)
                if p is None:
                    continue
                atr[m, it, nd] = atr[m, it, nd] - p
                atr[m, it, nr] = atr[m, it, nr] + p
    for n in range(ncat):
        an, vn = a[n, J, I], v[n, J, I]
        with np.errstate(divide="ignore", invalid="ignore"):
            hicen[:, n] = np.where(an > PUNY, vn / an, 0.0)
        compute_tracers(J, I, ntrcr, dep, tr, atr[:, :, n], a[n], v[n], s[n], t[n], Tocnfrz)
    return None


def rebin(J, I, ntrcr, dep, tr, hin_max, a, v, s, t, Tocnfrz, info):
    ncat, ic = a.shape[0], len(J)
    donor = np.zeros((ic, ncat), dtype=np.int64)
    daice = np.zeros((ic, ncat))
    dvice = np.zeros((ic, ncat))
    hicen = np.zeros((ic, ncat))
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(ncat):
            an, vn = a[n, J, I], v[n, J, I]
            hicen[:, n] = np.where(an > PUNY, vn / an, 0.0)
        a1 = a[0, J, I]
        adj = (a1 > PUNY) & (hicen[:, 0] <= hin_max[0]) & (hin_max[0] > 0.0)          # :605-610
        a[0, J[adj], I[adj]] = v[0, J[adj], I[adj]] / hin_max[0]
        hicen[adj, 0] = hin_max[0]
    info["adjusted"] = (J[adj], I[adj])
    info["boundaries"] = []                  # per shifting boundary: (pass, n, donors (bool per listed cell))
    for up in (True, False):
        for n in (range(ncat - 1) if up else range(ncat - 2, -1, -1)):                  # boundary n + 1
            nd = n if up else n + 1
            an, vn = a[nd, J, I], v[nd, J, I]
            sel = (an > PUNY) & ((hicen[:, nd] > hin_max[n + 1]) if up else (hicen[:, nd] <= hin_max[n + 1]))
            if not sel.any():
                continue
            donor[sel, n] = nd + 1
            daice[sel, n] = an[sel]
            dvice[sel, n] = vn[sel]
            info["boundaries"].append(("up" if up else "down", n + 1, sel.copy()))
            stop = shift_ice(J, I, ntrcr, dep, tr, a, v, s, t, hicen, donor, daice, dvice, Tocnfrz)
            if stop:
                return stop
            donor[:, n] = 0; daice[:, n] = 0.0; dvice[:, n] = 0.0
    return None


def zap_snow(cells, n, dt, tr, k, t, s, dfresh, dfhocn):
    for j, i in cells:
        for l in range(tr.nslyr):
            xtmp = t[n, tr.nt_qsno - 1 + l, j, i] / dt * s[n, j, i] / float(tr.nslyr)
            dfhocn[j, i] = dfhocn[j, i] + xtmp
            t[n, tr.nt_qsno - 1 + l, j, i] = 0.0
        xtmp = (k["rhos"] * s[n, j, i]) / dt
        dfresh[j, i] = dfresh[j, i] + xtmp
        s[n, j, i] = 0.0


def cleanup_block(blk, dt, ntrcr, dep, tr, hin_max, k, a, v, s, t, aice0, aice, first_ice, dflux, info):
    """one cleanup_itd call.  a, v, s (ncat, ny, nx), t (ncat, ntrcr_dim, ny, nx), aice0 / aice (ny, nx), first_ice (ncat, ny, nx) int32,
    dflux: dict of (ny, nx) dfpond, dfresh, dfsalt, dfhocn (zeroed here).  Returns (reason, i, j) or None."""
    ilo, ihi, jlo, jhi = blk
    ncat = a.shape[0]
    Tocnfrz = k["Tocnfrz"]
    for q in dflux.values():
        q[:] = 0.0
    aice[:] = 0.0                                                        # aggregate_area (:489-506)
    for n in range(ncat):
        aice[:] = aice + a[n]
    aice0[:] = np.maximum(1.0 - aice, 0.0)
    phys = [(j, i) for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi)]
    stop = None
    for j, i in phys:                                                    # :1648-1655 (no exit: the last one)
        if aice[j, i] > 1.0 + PUNY or aice[j, i] < -PUNY:
            stop = (1, i + 1, j + 1)
    if stop:
        return stop
    lst = [(j, i) for j, i in phys if aice[j, i] > PUNY]
    J = np.array([c[0] for c in lst], dtype=np.int64)
    I = np.array([c[1] for c in lst], dtype=np.int64)
    info["listed"] = (J, I)
    stop = rebin(J, I, ntrcr, dep, tr, hin_max, a, v, s, t, Tocnfrz, info)
    if stop:
        return stop
    dfpond, dfresh, dfsalt, dfhocn = dflux["dfpond"], dflux["dfresh"], dflux["dfsalt"], dflux["dfhocn"]
    info["zap1"] = []
    for n in range(ncat):                                                # zap_small_areas I (:1872-2015)
        cells = []
        for j, i in phys:
            if a[n, j, i] < -PUNY:
                return (6, i + 1, j + 1)
            if abs(a[n, j, i]) != 0.0 and abs(a[n, j, i]) <= PUNY:
                cells.append((j, i))
        if not cells:
            continue
        info["zap1"] += [(n, j, i, float(a[n, j, i])) for j, i in cells]
        if tr.tr_pond_topo:
            for j, i in cells:
                xtmp = a[n, j, i] * t[n, tr.nt_apnd - 1, j, i] * t[n, tr.nt_hpnd - 1, j, i]
                dfpond[j, i] = dfpond[j, i] - xtmp
        for l in range(tr.nilyr):
            for j, i in cells:
                xtmp = t[n, tr.nt_qice - 1 + l, j, i] / dt * v[n, j, i] / float(tr.nilyr)
                dfhocn[j, i] = dfhocn[j, i] + xtmp
                t[n, tr.nt_qice - 1 + l, j, i] = 0.0
        for j, i in cells:
            xtmp = (k["rhoi"] * v[n, j, i]) / dt
            dfresh[j, i] = dfresh[j, i] + xtmp
            xtmp = k["rhoi"] * v[n, j, i] * k["ice_ref_salinity"] * P001 / dt
            dfsalt[j, i] = dfsalt[j, i] + xtmp
            aice0[j, i] = aice0[j, i] + a[n, j, i]
            a[n, j, i] = 0.0
            v[n, j, i] = 0.0
            t[n, tr.nt_Tsfc - 1, j, i] = Tocnfrz
        zap_snow(cells, n, dt, tr, k, t, s, dfresh, dfhocn)
        for it in range(1, ntrcr):                                       # tracers 2 .. ntrcr (:1991-2007)
            for j, i in cells:
                t[n, it, j, i] = 1.0 if (tr.tr_brine and it + 1 == tr.nt_fbri) else 0.0
        for j, i in cells:
            first_ice[n, j, i] = 1
    cells = []                                                           # II (:2022-2164)
    for j, i in phys:
        if aice[j, i] > 1.0 + PUNY:
            return (7, i + 1, j + 1)
        if aice[j, i] > 1.0 and aice[j, i] < 1.0 + PUNY:
            cells.append((j, i))
    info["zap2"] = list(cells)
    if cells:
        for n in range(ncat):
            for j, i in cells:
                ai = aice[j, i]
                if tr.tr_pond_topo:
                    xtmp = a[n, j, i] * t[n, tr.nt_apnd - 1, j, i] * t[n, tr.nt_hpnd - 1, j, i] * (ai - 1.0) / ai
                    dfpond[j, i] = dfpond[j, i] - xtmp
                for l in range(tr.nilyr):
                    xtmp = t[n, tr.nt_qice - 1 + l, j, i] * v[n, j, i] / float(tr.nilyr) * (ai - 1.0) / ai / dt
                    dfhocn[j, i] = dfhocn[j, i] + xtmp
                for l in range(tr.nslyr):
                    xtmp = t[n, tr.nt_qsno - 1 + l, j, i] * s[n, j, i] / float(tr.nslyr) * (ai - 1.0) / ai / dt
                    dfhocn[j, i] = dfhocn[j, i] + xtmp
                xtmp = (k["rhoi"] * v[n, j, i] + k["rhos"] * s[n, j, i]) * (ai - 1.0) / ai / dt
                dfresh[j, i] = dfresh[j, i] + xtmp
                xtmp = k["rhoi"] * v[n, j, i] * k["ice_ref_salinity"] * P001 * (ai - 1.0) / ai / dt
                dfsalt[j, i] = dfsalt[j, i] + xtmp
                a[n, j, i] = a[n, j, i] * (1.0 / ai)
                v[n, j, i] = v[n, j, i] * (1.0 / ai)
                s[n, j, i] = s[n, j, i] * (1.0 / ai)
        for j, i in cells:
            aice[j, i] = 1.0
            aice0[j, i] = 0.0
    info["zapT"] = []                                                    # zap_snow_temperature (:2341-2413)
    rnslyr = float(tr.nslyr)
    for n in range(ncat):
        cells = []
        for j, i in phys:
            l_zap = False
            if a[n, j, i] > PUNY:
                hsn = s[n, j, i] / a[n, j, i]
                for l in range(tr.nslyr):
                    if hsn > k["hs_min"]:
                        zqsn = t[n, tr.nt_qsno - 1 + l, j, i]
                        Tmax = -zqsn * PUNY * rnslyr / (k["rhos"] * k["cp_ice"] * s[n, j, i])
                    else:
                        zqsn = -k["rhos"] * k["Lfresh"]
                        Tmax = PUNY
                    zTsn = (k["Lfresh"] + zqsn / k["rhos"]) / k["cp_ice"]
                    if zTsn < k["Tmin"] or zTsn > Tmax:
                        l_zap = True
                        info["zapT"].append((n, j, i, "cold" if zTsn < k["Tmin"] else "warm"))
                    elif hsn <= k["hs_min"] and s[n, j, i] > 0.0:
                        info.setdefault("thin_kept", []).append((n, j, i))
            if l_zap:
                cells.append((j, i))
        if cells:
            zap_snow(cells, n, dt, tr, k, t, s, dfresh, dfhocn)
    return None


def cleanup_itd(blocks, dt, ntrcr, dep, tr, hin_max, k, aicen, vicen, vsnon, trcrn, aice0, aice, fluxes=None, first_ice=None):
    """every block in turn, as step_ridge.  fluxes: dict with any of fpond, fresh, fsalt, fhocn (nb, ny, nx), incremented.
    Returns (infos, stop) with stop = (reason, block, i, j) of the lowest block that stops, or None."""
    tr = tr if isinstance(tr, Tr) else Tr(tr)
    nb, ncat, ny, nx = aicen.shape
    infos, stop = [], None
    fi = first_ice if first_ice is not None else np.zeros((nb, ncat, ny, nx), dtype=np.int32)
    for b, blk in enumerate(blocks):
        info = {}
        d = {q: np.zeros((ny, nx)) for q in ("dfpond", "dfresh", "dfsalt", "dfhocn")}
        st = cleanup_block(blk, dt, ntrcr, dep, tr, hin_max, k, aicen[b], vicen[b], vsnon[b], trcrn[b], aice0[b], aice[b], fi[b], d, info)
        infos.append(info)
        if st:
            if stop is None:
                stop = (st[0], b + 1, st[1], st[2])
            continue
        for name, q in (("fpond", "dfpond"), ("fresh", "dfresh"), ("fsalt", "dfsalt"), ("fhocn", "dfhocn")):
            if fluxes is not None and fluxes.get(name) is not None:
                fluxes[name][b] = fluxes[name][b] + d[q]
    return infos, stop


def aggregate(dt, ntrcr, dep, tr, tmask, blocks, aicen, vicen, vsnon, trcrn, aice, vice, vsno, aice0, trcr, daidtd=None, dvidtd=None,
              dagedtd=None, Tocnfrz=-1.8):
    """aggregate (:246-458) on every cell of every block (tmask: every cell of the block arrays), then the tendencies on physical cells"""
    tr = tr if isinstance(tr, Tr) else Tr(tr)
    nb, ncat, ny, nx = aicen.shape
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        aice0[b] = 1.0; aice[b] = 0.0; vice[b] = 0.0; vsno[b] = 0.0
        J, I = np.nonzero(tmask[b] != 0)
        if len(J):
            atr = np.zeros((len(J), ntrcr))
            for n in range(ncat):
                a, v, s = aicen[b, n, J, I], vicen[b, n, J, I], vsnon[b, n, J, I]
                aice[b, J, I] = aice[b, J, I] + a
                vice[b, J, I] = vice[b, J, I] + v
                vsno[b, J, I] = vsno[b, J, I] + s
                t = [trcrn[b, n, q, J, I] for q in range(ntrcr)]
                for it in range(ntrcr):                                   # the tracer first, then the parents, then the base (:356-431)
                    d = dep[it]
                    if d == 0:
                        p = t[it] * a
                    elif d == 1:
                        p = t[it] * v
                    elif d == 2:
                        p = t[it] * s
                    elif d == 2 + tr.nt_alvl:
                        p = t[it] * t[tr.nt_alvl - 1] * a
                    elif d == 2 + tr.nt_apnd and (tr.tr_pond_cesm or tr.tr_pond_topo):
                        p = t[it] * t[tr.nt_apnd - 1] * a
                    elif d == 2 + tr.nt_apnd and tr.tr_pond_lvl:
                        p = t[it] * t[tr.nt_apnd - 1] * t[tr.nt_alvl - 1] * a
                    elif d == 2 + tr.nt_fbri:
                        p = t[it] * t[tr.nt_fbri - 1] * v
                    else:
                        continue
                    atr[:, it] = atr[:, it] + p
            aice0[b, J, I] = np.maximum(1.0 - aice[b, J, I], 0.0)
            compute_tracers(J, I, ntrcr, dep, tr, atr, aice[b], vice[b], vsno[b], trcr[b], Tocnfrz)
        sl = (b, slice(jlo - 1, jhi), slice(ilo - 1, ihi))
        if dvidtd is not None:
            dvidtd[sl] = (vice[sl] - dvidtd[sl]) / dt
        if daidtd is not None:
            daidtd[sl] = (aice[sl] - daidtd[sl]) / dt
        if dagedtd is not None and tr.nt_iage > 0:
            q = (b, tr.nt_iage - 1, slice(jlo - 1, jhi), slice(ilo - 1, ihi))
            dagedtd[sl] = (trcr[q] - dagedtd[sl]) / dt
