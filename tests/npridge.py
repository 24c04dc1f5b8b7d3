"""ridge_ice (source/ice_mechred.F90:101-746) restated in Python for one block: the cell list of step_ridge, list-wide loops in the
Fortran's order, block-wide iteration (ridge_check's single flag), the Fortran's operation order in every expression.  Python floats
are IEEE doubles and nothing is fused, so the result is bit-comparable with a -ffp-contract=off build given the same exp().

`exp` is a parameter: math.exp (libm), or dev_exp below -- a port of the device's fixed algorithm (csrc/evpk_kernels.hip dev_exp: the
same operations in the same order, math.ldexp).

Differences from the Fortran that the callers account for: compute_tracers zeroes trcrn(:,:,:,n) of the WHOLE block slice
(ice_itd.F90:1401) -- here, as in the library, unlisted cells keep their values; there is no nt_Tsfc (the reference driver sets it to 0).
"""
from __future__ import annotations

import math

import numpy as np

PUNY = 1.0e-11
CS, FSNOWRDG, GSTAR, ASTAR, MAXRAFT = 0.25, 0.5, 0.15, 0.05, 1.0          # ice_mechred.F90:66-76
NITERMAX = 20
BIG = 1.0e8
STOP_AICE0, STOP_ARDG, STOP_NITER, STOP_ASUM = 1, 2, 3, 4

TRACER_FIELDS = ["nt_qsno", "nslyr", "nt_alvl", "nt_vlvl", "nt_apnd", "nt_hpnd", "nt_fbri", "tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo"]
DIAG_2D = ["dardg1dt", "dardg2dt", "dvirdgdt", "opening", "fpond", "fresh", "fhocn"]
DIAG_3D = ["dardg1ndt", "dardg2ndt", "dvirdgndt", "aparticn", "krdgn", "araftn", "vraftn", "aredistn", "vredistn"]


def dev_exp(x: float) -> float:
    ln2HI, ln2LO, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    x = float(x)
    ax = abs(x)
    hi = lo = 0.0
    k = 0
    if ax > 0.34657359027997264:
        if ax < 1.0397207708399179:
            k = -1 if x < 0.0 else 1
            hi = x - float(k) * ln2HI
            lo = float(k) * ln2LO
        else:
            k = int(invln2 * x + (-0.5 if x < 0.0 else 0.5))          # (int): truncation toward zero, as the C cast
            t = float(k)
            hi = x - t * ln2HI
            lo = t * ln2LO
        x = hi - lo
    elif ax < 3.725290298461914e-09:
        return 1.0 + x
    t = x * x
    c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    return math.ldexp(y, k)


def _sign1(x: float) -> float:
    return math.copysign(1.0, x)


def ridge_itd(a0, a, v, krdg_partic, mu_rdg, exp, mraft):
    """one cell; a, v: lists 1..ncat (index 0 unused).  Returns aksum, apartic[0..ncat], hrmin, hrexp, krdg[1..ncat]; updates mraft"""
    ncat = len(a) - 1
    Gstari, astari = 1.0 / GSTAR, 1.0 / ASTAR
    G = [0.0] * (ncat + 2)                      # G[n + 1] = Gsum(n), n = -1..ncat
    apartic = [0.0] * (ncat + 1)
    hrmin = [0.0] * (ncat + 1); hrexp = [0.0] * (ncat + 1); krdg = [1.0] * (ncat + 1)
    G[1] = a0 if a0 > PUNY else G[0]
    for n in range(1, ncat + 1):
        G[n + 1] = G[n] + a[n] if a[n] > PUNY else G[n]
    work = 1.0 / G[ncat + 1]
    for n in range(0, ncat + 1):
        G[n + 1] = G[n + 1] * work
    if krdg_partic == 0:
        for n in range(0, ncat + 1):
            g1, g0 = G[n + 1], G[n]
            if g1 < GSTAR:
                apartic[n] = Gstari * (g1 - g0) * (2.0 - (g0 + g1) * Gstari)
            elif g0 < GSTAR:
                apartic[n] = Gstari * (GSTAR - g0) * (2.0 - (g0 + GSTAR) * Gstari)
    else:
        xtmp = 1.0 / (1.0 - exp(-astari))
        for n in range(-1, ncat + 1):
            G[n + 1] = exp(-G[n + 1] * astari) * xtmp
        for n in range(0, ncat + 1):
            apartic[n] = G[n] - G[n + 1]
    for n in range(1, ncat + 1):                # krdg_redist = 1
        if a[n] > PUNY:
            hi = v[n] / a[n]
            hi = max(hi, PUNY)
            hrmin[n] = min(2.0 * hi, hi + MAXRAFT)
            hrexp[n] = mu_rdg * math.sqrt(hi)
            krdg[n] = (hrmin[n] + hrexp[n]) / hi
            m = max(0.0, _sign1(hi + MAXRAFT - hrmin[n]))
            xt = m * ((2.0 * hi + hrexp[n]) / hi - krdg[n])
            mraft[n] = max(0.0, _sign1(PUNY - abs(xt)))
    aksum = apartic[0]
    for n in range(1, ncat + 1):
        aksum = aksum + apartic[n] * (1.0 - 1.0 / krdg[n])
    return aksum, apartic, hrmin, hrexp, krdg


def tracer_tables(ntrcr, trcr_depend, tr):
    """per tracer (0-based): acc -- how atrcrn is built and moved (0 area, 1 ice volume, 2 snow volume, 3 aicen*alvl, 4 aicen*apnd,
    5 aicen*alvl*apnd, 6 vicen*fbri, -1 no rule), in the order of the reference's elseif chain (:1456-1513)"""
    acc = []
    pond_at = bool(tr["tr_pond_cesm"] or tr["tr_pond_topo"])
    for it in range(1, ntrcr + 1):
        dep = int(trcr_depend[it - 1])
        if dep == 0: acc.append(0)
        elif dep == 1: acc.append(1)
        elif dep == 2: acc.append(2)
        elif tr["nt_fbri"] > 0 and dep == 2 + tr["nt_fbri"]: acc.append(6)
        elif tr["nt_alvl"] > 0 and dep == 2 + tr["nt_alvl"]: acc.append(3)
        elif tr["nt_apnd"] > 0 and dep == 2 + tr["nt_apnd"] and pond_at: acc.append(4)
        elif tr["nt_apnd"] > 0 and dep == 2 + tr["nt_apnd"] and tr["tr_pond_lvl"]: acc.append(5)
        else: acc.append(-1)
    return acc


def ridge_ice_block(dt, ndtd, krdg_partic, mu_rdg, rhos, hin_max, tmask, ilo, ihi, jlo, jhi, rdg_conv, rdg_shear, aice0, aicen, vicen,
                    vsnon, trcrn, ntrcr, trcr_depend, tracers, diag=None, exp=math.exp, per_cell_iteration=False):
    """One block, in place.  Arrays: tmask, rdg_*, aice0 (ny, nx); aicen, vicen, vsnon (ncat, ny, nx); trcrn (ncat, ntrcr_dim, ny, nx);
    diag: dict name -> array or None.  ilo..jhi 1-based.  per_cell_iteration: NOT the reference -- a cell repeats only while it is not
    converged itself (what the block-wide flag is tested against).
    Returns dict(stop=None or (reason, i, j), repeats=number of 'Repeat ridging' passes, conv1=(ny, nx) bool: listed cells that were
    converged after the first pass, cells=the list, sig=per listed cell the outcomes of its data-dependent comparisons in order:
    two runs took the same branches in a cell iff its sig is equal)."""
    tr = {k: int(tracers.get(k, 0)) for k in TRACER_FIELDS}
    diag = diag or {}
    ncat = aicen.shape[0]
    hin = [float(h) for h in hin_max]
    hin[ncat] = BIG                                                     # ridge_prep (:864)
    cells = [(i, j) for j in range(jlo, jhi + 1) for i in range(ilo, ihi + 1) if tmask[j - 1, i - 1]]
    out = dict(stop=None, repeats=0, conv1=np.zeros(aice0.shape, dtype=bool), sig=[], cells=[])
    if not cells:
        return out
    acc = tracer_tables(ntrcr, trcr_depend, tr)
    nc = len(cells)
    out["cells"] = cells
    Z = lambda: [0.0] * nc
    msnow, esnow, mpond, ardg1, ardg2, virdg, aopen = Z(), Z(), Z(), Z(), Z(), Z(), Z()
    ardg1nn = [[0.0] * (ncat + 1) for _ in range(nc)]
    ardg2nn = [[0.0] * (ncat + 1) for _ in range(nc)]
    virdgnn = [[0.0] * (ncat + 1) for _ in range(nc)]
    mraftn = [[0.0] * (ncat + 1) for _ in range(nc)]
    asum, closing_net, opning = Z(), Z(), Z()
    active = [True] * nc
    out["sig"] = sig = [[] for _ in range(nc)]               # per cell: the outcome of every data-dependent comparison, in order
    for m, (i, j) in enumerate(cells):                                  # asum_ridging, ridge_prep
        s = float(aice0[j - 1, i - 1])
        for n in range(ncat):
            s = s + float(aicen[n, j - 1, i - 1])
        asum[m] = s
        closing_net[m] = CS * float(rdg_shear[j - 1, i - 1]) + float(rdg_conv[j - 1, i - 1])
        divu_adv = (1.0 - s) / dt
        if divu_adv < 0.0:
            closing_net[m] = max(closing_net[m], -divu_adv)
        opning[m] = closing_net[m] + divu_adv

    def shift(m, i, j):
        """ridge_itd + ridge_shift of one cell; returns a stop tuple or None"""
        J, I = j - 1, i - 1
        S = sig[m].append
        a = [0.0] + [float(aicen[n, J, I]) for n in range(ncat)]
        v = [0.0] + [float(vicen[n, J, I]) for n in range(ncat)]
        sn = [0.0] + [float(vsnon[n, J, I]) for n in range(ncat)]
        a0 = float(aice0[J, I])
        aksum, apartic, hrmin, hrexp, krdg = ridge_itd(a0, a, v, krdg_partic, mu_rdg, exp, mraftn[m])
        for n in range(1, ncat + 1):
            if diag.get("aparticn") is not None: diag["aparticn"][n - 1, J, I] = apartic[n]
            if diag.get("krdgn") is not None: diag["krdgn"][n - 1, J, I] = krdg[n]
        told = [[float(trcrn[n, it, J, I]) for it in range(ntrcr)] for n in range(ncat)]
        pa = lambda n, nt: told[n][nt - 1] if nt else 0.0
        atr = [[0.0] * ntrcr for _ in range(ncat)]
        for n in range(ncat):
            for it in range(ntrcr):
                t = told[n][it]
                q = acc[it]
                if q == 0: w = a[n + 1] * t
                elif q == 1: w = v[n + 1] * t
                elif q == 2: w = sn[n + 1] * t
                elif q == 3: w = a[n + 1] * pa(n, tr["nt_alvl"]) * t
                elif q == 4: w = a[n + 1] * pa(n, tr["nt_apnd"]) * t
                elif q == 5: w = a[n + 1] * pa(n, tr["nt_alvl"]) * pa(n, tr["nt_apnd"]) * t
                elif q == 6: w = v[n + 1] * pa(n, tr["nt_fbri"]) * t
                else: w = 0.0
                atr[n][it] = w
        closing_gross = closing_net[m] / aksum
        if apartic[0] > 0.0:
            wk1 = apartic[0] * closing_gross * dt
            S(wk1 > a0)
            if wk1 > a0:
                tmpfac = a0 / wk1
                closing_gross = closing_gross * tmpfac
                opning[m] = opning[m] * tmpfac
                out["tmpfac0"] = out.get("tmpfac0", 0) + 1
        for n in range(1, ncat + 1):
            if a[n] > PUNY and apartic[n] > 0.0:
                wk1 = apartic[n] * closing_gross * dt
                S(wk1 > a[n])
                if wk1 > a[n]:
                    tmpfac = a[n] / wk1
                    closing_gross = closing_gross * tmpfac
                    opning[m] = opning[m] * tmpfac
                    out["tmpfacn"] = out.get("tmpfacn", 0) + 1
        a0 = a0 - apartic[0] * closing_gross * dt + opning[m] * dt
        S(a0 < 0.0)
        if a0 < -PUNY:
            aice0[J, I] = a0
            return (STOP_AICE0, 0, 0, i, j)
        elif a0 < 0.0:
            a0 = 0.0
            out["clamp"] = out.get("clamp", 0) + 1
        aice0[J, I] = a0
        aopen[m] = opning[m] * dt
        ai, vi, si = list(a), list(v), list(sn)
        for n in range(1, ncat + 1):
            S(ai[n] > PUNY and apartic[n] > 0.0 and closing_gross > 0.0)
            if not (ai[n] > PUNY and apartic[n] > 0.0 and closing_gross > 0.0):
                continue
            S(apartic[n] * closing_gross * dt > ai[n])
            ardg1n = apartic[n] * closing_gross * dt
            if ardg1n > ai[n] + PUNY:
                return (STOP_ARDG, 1, n, i, j)
            ardg1n = min(ai[n], ardg1n)
            ardg2n = ardg1n / krdg[n]
            afrac = ardg1n / ai[n]
            virdgn = vi[n] * afrac
            vsrdgn = si[n] * afrac
            a[n] = a[n] - ardg1n; v[n] = v[n] - virdgn; sn[n] = sn[n] - vsrdgn
            ardg1[m] = ardg1[m] + ardg1n; ardg2[m] = ardg2[m] + ardg2n; virdg[m] = virdg[m] + virdgn
            ardg1nn[m][n] = ardg1n; ardg2nn[m][n] = ardg2n; virdgnn[m][n] = virdgn
            msnow[m] = msnow[m] + rhos * vsrdgn * (1.0 - FSNOWRDG)
            T = told[n - 1]
            if tr["tr_pond_topo"]:
                mpond[m] = mpond[m] + ardg1n * T[tr["nt_apnd"] - 1] * T[tr["nt_hpnd"] - 1]
            for k in range(1, tr["nslyr"] + 1):
                esrdgn = vsrdgn * T[tr["nt_qsno"] + k - 2] / float(tr["nslyr"])
                esnow[m] = esnow[m] + esrdgn * (1.0 - FSNOWRDG)
            for it in range(ntrcr):
                t = T[it]
                q = acc[it]
                if q == 0: atr[n - 1][it] = atr[n - 1][it] - ardg1n * t
                elif q == 1: atr[n - 1][it] = atr[n - 1][it] - virdgn * t
                elif q == 2: atr[n - 1][it] = atr[n - 1][it] - vsrdgn * t
                elif q == 3: atr[n - 1][it] = atr[n - 1][it] - ardg1n * pa(n - 1, tr["nt_alvl"]) * t
                elif q == 4: atr[n - 1][it] = atr[n - 1][it] - ardg1n * pa(n - 1, tr["nt_apnd"]) * t
                elif q == 5: atr[n - 1][it] = atr[n - 1][it] - ardg1n * pa(n - 1, tr["nt_alvl"]) * pa(n - 1, tr["nt_apnd"]) * t
                elif q == 6: atr[n - 1][it] = atr[n - 1][it] - virdgn * t * pa(n - 1, tr["nt_fbri"])
            hi1, hexp = hrmin[n], hrexp[n]
            for nr in range(1, ncat + 1):
                if nr < ncat:
                    if hi1 >= hin[nr]:
                        farea = fvol = 0.0
                    else:
                        hL = max(hi1, hin[nr - 1]); hR = hin[nr]
                        expL = exp(-(hL - hi1) / hexp); expR = exp(-(hR - hi1) / hexp)
                        farea = expL - expR
                        fvol = ((hL + hexp) * expL - (hR + hexp) * expR) / (hi1 + hexp)
                else:
                    hL = max(hi1, hin[nr - 1])
                    expL = exp(-(hL - hi1) / hexp)
                    farea = expL
                    fvol = (hL + hexp) * expL / (hi1 + hexp)
                if n == 1:
                    if diag.get("aredistn") is not None: diag["aredistn"][nr - 1, J, I] = farea * ardg2n
                    if diag.get("vredistn") is not None: diag["vredistn"][nr - 1, J, I] = fvol * virdgn
                a[nr] = a[nr] + farea * ardg2n
                v[nr] = v[nr] + fvol * virdgn
                sn[nr] = sn[nr] + fvol * vsrdgn * FSNOWRDG
                for it in range(ntrcr):
                    t = T[it]
                    q = acc[it]
                    if q == 0:
                        if it + 1 != tr["nt_alvl"]: atr[nr - 1][it] = atr[nr - 1][it] + farea * ardg2n * t
                    elif q == 1:
                        if it + 1 != tr["nt_vlvl"]: atr[nr - 1][it] = atr[nr - 1][it] + fvol * virdgn * t
                    elif q == 2: atr[nr - 1][it] = atr[nr - 1][it] + fvol * vsrdgn * FSNOWRDG * t
                    elif q == 6: atr[nr - 1][it] = atr[nr - 1][it] + fvol * virdgn * pa(n - 1, tr["nt_fbri"]) * t
        for n in range(ncat):                                           # compute_tracers (ice_itd.F90:1401-1499), nt_Tsfc = 0
            an, vn, sv = a[n + 1], v[n + 1], sn[n + 1]
            S((an > PUNY, vn > 0.0, sv > 0.0))
            new = [0.0] * ntrcr
            nv = lambda nt: new[nt - 1] if nt else 0.0
            for it in range(ntrcr):
                at = atr[n][it]
                q = acc[it]
                if q == 0: r = at / an if an > PUNY else 0.0
                elif q == 1: r = at / vn if vn > 0.0 else (1.0 if it + 1 == tr["nt_fbri"] else 0.0)
                elif q == 2: r = at / sv if sv > 0.0 else 0.0
                elif q == 3: d = nv(tr["nt_alvl"]) * an; r = at / d if d > 0.0 else 0.0
                elif q == 4: d = nv(tr["nt_apnd"]) * an; r = at / d if d > 0.0 else 0.0
                elif q == 5: d = nv(tr["nt_alvl"]) * nv(tr["nt_apnd"]) * an; r = at / d if d > 0.0 else 0.0
                elif q == 6: d = nv(tr["nt_fbri"]) * vn; r = at / d if d > 0.0 else 0.0
                else: r = 0.0
                new[it] = r
            for it in range(ntrcr):
                trcrn[n, it, J, I] = new[it]
            aicen[n, J, I] = an; vicen[n, J, I] = vn; vsnon[n, J, I] = sv
        return None

    for niter in range(1, NITERMAX + 1):
        # the reference runs ridge_shift's loops list-wide, so the first stop it meets is: the aice0 loop over the cells, then n outer /
        # cells inner; the cells of a pass are independent, so a per-cell walk gives the same state where no cell stops
        stops = []
        for m, (i, j) in enumerate(cells):
            if not active[m]:
                continue
            st = shift(m, i, j)
            if st:
                stops.append((st[1], st[2], m, st))
        if stops:
            st = min(stops)[3]
            out["stop"] = (st[0], st[3], st[4])
            return out
        iterate = False
        for m, (i, j) in enumerate(cells):                              # asum_ridging + ridge_check
            if not active[m]:
                continue
            s = float(aice0[j - 1, i - 1])
            for n in range(ncat):
                s = s + float(aicen[n, j - 1, i - 1])
            asum[m] = s
            sig[m].append(abs(s - 1.0) < PUNY)
            if abs(s - 1.0) < PUNY:
                closing_net[m] = 0.0; opning[m] = 0.0
                if niter == 1:
                    out["conv1"][j - 1, i - 1] = True
                if per_cell_iteration:
                    active[m] = False
            else:
                iterate = True
                divu_adv = (1.0 - s) / dt
                closing_net[m] = max(0.0, -divu_adv)
                opning[m] = max(0.0, divu_adv)
        if not iterate:
            break
        out["repeats"] += 1
        if niter == NITERMAX:
            out["stop"] = (STOP_NITER, 0, 0)
            return out
    dti = 1.0 / dt
    dtt = 1.0 / (ndtd * dt)
    g = lambda k: diag.get(k)
    for m, (i, j) in enumerate(cells):
        J, I = j - 1, i - 1
        if g("dardg1dt") is not None: diag["dardg1dt"][J, I] = ardg1[m] * dti
        if g("dardg2dt") is not None: diag["dardg2dt"][J, I] = ardg2[m] * dti
        if g("dvirdgdt") is not None: diag["dvirdgdt"][J, I] = virdg[m] * dti
        if g("opening") is not None: diag["opening"][J, I] = aopen[m] * dti
        for n in range(1, ncat + 1):
            if g("dardg1ndt") is not None: diag["dardg1ndt"][n - 1, J, I] = ardg1nn[m][n] * dti
            if g("dardg2ndt") is not None: diag["dardg2ndt"][n - 1, J, I] = ardg2nn[m][n] * dti
            if g("dvirdgndt") is not None: diag["dvirdgndt"][n - 1, J, I] = virdgnn[m][n] * dti
            if g("araftn") is not None: diag["araftn"][n - 1, J, I] = mraftn[m][n] * ardg2nn[m][n]
            if g("vraftn") is not None: diag["vraftn"][n - 1, J, I] = mraftn[m][n] * virdgnn[m][n]
        if g("fresh") is not None: diag["fresh"][J, I] = diag["fresh"][J, I] + msnow[m] * dtt
        if g("fhocn") is not None: diag["fhocn"][J, I] = diag["fhocn"][J, I] + esnow[m] * dtt
        if g("fpond") is not None: diag["fpond"][J, I] = diag["fpond"][J, I] - mpond[m]
    for m, (i, j) in enumerate(cells):
        if abs(asum[m] - 1.0) > PUNY:
            out["stop"] = (STOP_ASUM, i, j)
            return out
    return out


def ridge_ice(dt, ndtd, krdg_partic, mu_rdg, rhos, hin_max, tmask, blocks, rdg_conv, rdg_shear, aice0, aicen, vicen, vsnon, trcrn, ntrcr,
              trcr_depend, tracers, diag=None, exp=math.exp, per_cell_iteration=False):
    """Every block, arrays with the leading block dimension; blocks: list of (ilo, ihi, jlo, jhi).  Returns the per-block results and
    `stop` = None or (reason, block (1-based), i, j) of the first block that stops (the reference aborts there)."""
    res = []
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        d = None if diag is None else {k: (v[b] if v is not None else None) for k, v in diag.items()}
        r = ridge_ice_block(dt, ndtd, krdg_partic, mu_rdg, rhos, hin_max, tmask[b], ilo, ihi, jlo, jhi, rdg_conv[b], rdg_shear[b], aice0[b],
                            aicen[b], vicen[b], vsnon[b], trcrn[b], ntrcr, trcr_depend, tracers, d, exp, per_cell_iteration)
        res.append(r)
    stop = None
    for b, r in enumerate(res):
        if r["stop"]:
            stop = (r["stop"][0], b + 1, r["stop"][1], r["stop"][2])
            break
    return res, stop
