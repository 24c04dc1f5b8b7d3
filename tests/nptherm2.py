"""numpy restatement of what step_therm2 (source/ice_step_mod.F90:741-995) does around linear_itd: the frain line (:804-809), add_new_ice
(source/ice_therm_itd.F90:1239-1850) with update_vertical_tracers (:967-1033) and the mushy liquidus (source/ice_therm_mushy.F90:43-123,
:3687-3756, :3903-3918), lateral_melt (:1043-1217) and reduce_area (source/ice_itd.F90:743-806) -- written from the Fortran and
independent of the HIP code: block by block, one cell list per block, the Fortran's loop order (the category loop outside the cell loop,
the layer loop where the Fortran has it) and its operation order per cell.  linear_itd is tests/nplitd.py's, cleanup_itd tests/npitd.py's.

PINNED to reference-built output: add_new_ice, update_vertical_tracers, the mushy liquidus, lateral_melt, reduce_area and the chain of
step_therm2 equal the records of the reference's own compiled routines bit for bit, stage by stage (tests/golden/ref_therm2_*.npz, made
by tests/golden/make_ref_therm2.py from oracle/ref/Makefile, target therm2; tests/test_therm2_ref.py).  What stays unpinned: step_therm2's call order
(the driver oracle/ref/ref_therm2.F90 restates it), a horizontally non-uniform salinz (the departure below), aerosols / bgc, and
l_conservation_check = .true.

l_conservation_check = .false. (ice_therm_itd.F90:37): those blocks are left out; tests/test_therm2_host.py makes the same check from
outside.  tr_aero, tr_brine, skl_bgc, nbtrcr: not restated (evpk_step_therm2 refuses them).  Stated departures, shared with the device
(include/evpk.h): lateral_melt lists physical cells with tmask and rside > 0; the ktherm /= 2 surplus loop uses the cell's own salinz
profile where the reference indexes Sprofile with the counter of the compressed surplus list (:1691) -- the same wherever salinz is
horizontally uniform, as init_thermo_vertical fills it.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), salinz (nb, nilyr + 1, ny, nx).
"""
from __future__ import annotations

import numpy as np

from . import npitd, nplitd
from .npitd import PUNY

F = np.float64
C0, C1, C2, C4, P1, P001, C1000 = F(0.0), F(1.0), F(2.0), F(4.0), F(0.1), F(0.001), F(1000.0)
BIGNUM = F(1.0e30)

# ice_therm_mushy.F90:43-123, in that file's expression order
AZ1, BZ1, AZ2, BZ2 = F(-18.48), F(0.0), F(-10.3085), F(62.4)
TB_LIQ, SB_LIQ = F(-7.6362968855167352), F(123.66702800276086)
AZ1P, BZ1P, AZ2P, BZ2P = AZ1 / C1000, BZ1 / C1000, AZ2 / C1000, BZ2 / C1000
J1, K1, L1 = BZ1 / AZ1, C1 / C1000, (C1 + BZ1P) / AZ1
J2, K2, L2 = BZ2 / AZ2, C1 / C1000, (C1 + BZ2P) / AZ2
M1, N1, O1 = AZ1, -AZ1P, -BZ1 / AZ1
M2, N2, O2 = AZ2, -AZ2P, -BZ2 / AZ2

INFO_KEYS = ["cells", "frzmlt_neg", "frzmlt_zero", "thin_frazil", "mid_frazil", "surplus_open", "icefree_thick", "full_zero", "full_tiny",
             "jcells", "kcells", "surplus_empty_cat", "surplus_tiny_v", "surplus_iage", "surplus_vlvl", "surplus_layers", "merge_empty_cat1",
             "merge_v1_le_puny", "merge_v1_gt_puny", "tsfc_clamped", "fy_is_one", "fy_clamped", "pond_at", "pond_lvl", "pond_lvl_skipped",
             "onset_set", "onset_kept", "onset_small_frazil", "si_linear", "si_quadratic", "ti_clamped", "ti_unclamped", "sb_high", "sb_low",
             "rside_nonpos", "rside_part", "rside_one", "fpond_changed", "reduce_hin", "reduce_dhi", "reduce_none", "untouched"]


def _min(x, y):
    return y if y < x else x


def _max(x, y):
    return y if y > x else x


def liquidus_brine_salinity_mush(T):
    t_high = C1 if T > TB_LIQ else C0
    lsubzero = C1 if T <= C0 else C0
    Sbr = ((T + J1) / (K1 * T + L1)) * t_high + ((T + J2) / (K2 * T + L2)) * (C1 - t_high)
    return Sbr * lsubzero


def liquidus_temperature_mush(Sbr):
    t_high = C1 if Sbr <= SB_LIQ else C0
    return ((Sbr / (M1 + N1 * Sbr)) + O1) * t_high + ((Sbr / (M2 + N2 * Sbr)) + O2) * (C1 - t_high)


def liquid_fraction(T, S):
    Sbr = _max(liquidus_brine_salinity_mush(T), F(PUNY))
    return S / _max(Sbr, S)


def enthalpy_mush(T, S, p):
    phi = liquid_fraction(T, S)
    return phi * (p["cp_ocn"] * p["rhow"] - p["cp_ice"] * p["rhoi"]) * T + p["rhoi"] * p["cp_ice"] * T - (C1 - phi) * p["rhoi"] * p["Lfresh"]


def update_vertical_tracers(trc, h1, h2, trc0):
    """:967-1033; trc: the nilyr values, returns the new ones"""
    nilyr = len(trc)
    rnilyr = F(nilyr)
    trc2 = np.zeros(nilyr)
    for k2 in range(1, nilyr + 1):
        x = C0
        z2a = (F(k2 - 1) * h2) / rnilyr
        z2b = (F(k2) * h2) / rnilyr
        for k1 in range(1, nilyr + 1):
            z1a = (F(k1 - 1) * h1) / rnilyr
            z1b = (F(k1) * h1) / rnilyr
            overlap = _max(_min(z1b, z2b) - _max(z1a, z2a), C0)
            x = x + overlap * trc[k1 - 1]
        overlap = _max(_min(h2, z2b) - _max(h1, z2a), C0)
        x = x + overlap * trc0
        trc2[k2 - 1] = (rnilyr * x) / h2
    return trc2


def params(x, ktherm, update_ocn_f=False, **kw):
    """the scalar arguments of one call from an input dict of tests/golden/therm2vec.py"""
    k = x["k"]
    p = dict(dt=F(x["dt"]), ktherm=int(ktherm), update_ocn_f=bool(update_ocn_f), yday=F(x["yday"]), hfrazilmin=F(x["hfrazilmin"]),
             phi_init=F(x["phi_init"]), dSin0_frazil=F(x["dSin0_frazil"]), cp_ocn=F(x["cp_ocn"]), rhow=F(x["rhow"]), rhoi=F(k["rhoi"]),
             rhos=F(k["rhos"]), Lfresh=F(k["Lfresh"]), cp_ice=F(k["cp_ice"]), salinity=F(k["ice_ref_salinity"]), hin_max=np.asarray(x["hin_max"]),
             ntrcr=int(x["ntrcr"]), tr=dict(x["tracers"]), dep=x["trcr_depend"], k=dict(k), use_frz_onset=True)
    p.update(kw)
    return p


def add_new_ice_block(J, I, p, a, v, t, aice0, aice, frzmlt, frazil, frz_onset, fresh, fsalt, Tf, sss, salinz, info):
    """one add_new_ice call on the cell list (J, I) of one block.  a, v (ncat, ny, nx); t (ncat, ntrcr_dim, ny, nx)"""
    tr = p["tr"]
    ncat, ic = a.shape[0], len(J)
    nilyr = tr.get("nilyr", 0) if p["ntrcr"] else 0
    dt, rhoi, Lfresh, puny = p["dt"], p["rhoi"], p["Lfresh"], F(PUNY)
    trc = p["ntrcr"] > 0
    nt = lambda k: tr.get(k, 0) - 1
    tr_iage, tr_FY, tr_lvl = tr.get("nt_iage", 0) > 0, tr.get("nt_FY", 0) > 0, tr.get("nt_alvl", 0) > 0 and tr.get("nt_vlvl", 0) > 0
    mushy = p["ktherm"] == 2
    hi0max = p["hin_max"][1] * F(0.9) if ncat > 1 else BIGNUM
    qi0new = np.zeros(ic); Si0new = np.zeros(ic); Sprofile = np.zeros((ic, nilyr))
    vi0new = np.zeros(ic); ai0new = np.zeros(ic); hsurp = np.zeros(ic)
    jl, kl = [], []
    with np.errstate(all="ignore"):
        for m in range(ic):                                                             # :1461-1493
            j, i = J[m], I[m]
            if mushy:
                s = sss[j, i]
                if s > C2 * p["dSin0_frazil"]:
                    Si0new[m] = s - p["dSin0_frazil"]
                    info["si_linear"] += 1
                else:
                    Si0new[m] = s * s / (C4 * p["dSin0_frazil"])
                    info["si_quadratic"] += 1
                Sprofile[m, :] = Si0new[m]
                Sbr = Si0new[m] / p["phi_init"]
                info["sb_high" if Sbr <= SB_LIQ else "sb_low"] += 1
                Tl = liquidus_temperature_mush(Sbr)
                info["ti_clamped" if -P1 < Tl else "ti_unclamped"] += 1
                Ti = _min(Tl, -P1)
                qi0new[m] = enthalpy_mush(Ti, Si0new[m], p)
            else:
                for k in range(nilyr):
                    Sprofile[m, k] = salinz[k, j, i]
                qi0new[m] = -rhoi * Lfresh
        for m in range(ic):                                                             # :1502-1598
            j, i = J[m], I[m]
            info["cells"] += 1
            fnew = _max(frzmlt[j, i], C0)
            vi0new[m] = -fnew * dt / qi0new[m]
            frazil[j, i] = vi0new[m]
            if frz_onset is not None and p["use_frz_onset"]:
                if frazil[j, i] > puny and frz_onset[j, i] < puny:
                    frz_onset[j, i] = p["yday"]
                    info["onset_set"] += 1
                elif frazil[j, i] > puny:
                    info["onset_kept"] += 1
                elif frazil[j, i] > C0:
                    info["onset_small_frazil"] += 1
            if p["update_ocn_f"]:
                dfresh = -rhoi * vi0new[m] / dt
                dfsalt = p["salinity"] * P001 * dfresh
                fresh[j, i] = fresh[j, i] + dfresh
                fsalt[j, i] = fsalt[j, i] + dfsalt
            elif mushy:
                vi0tmp = fnew * dt / (rhoi * Lfresh)
                dfresh = -rhoi * (vi0new[m] - vi0tmp) / dt
                dfsalt = p["salinity"] * P001 * dfresh
                fresh[j, i] = fresh[j, i] + dfresh
                fsalt[j, i] = fsalt[j, i] + dfsalt
            if frzmlt[j, i] < C0:
                info["frzmlt_neg"] += 1
            elif frzmlt[j, i] == C0:
                info["frzmlt_zero"] += 1
            if vi0new[m] > C0:
                if aice0[j, i] > puny:
                    q = vi0new[m] / aice0[j, i]
                    hi0new = _max(q, p["hfrazilmin"])
                    if hi0new > hi0max and aice0[j, i] + puny < C1:
                        hi0new = hi0max
                        ai0new[m] = aice0[j, i]
                        vsurp = vi0new[m] - ai0new[m] * hi0new
                        hsurp[m] = vsurp / aice[j, i]
                        vi0new[m] = ai0new[m] * hi0new
                        info["surplus_open"] += 1
                    else:
                        ai0new[m] = vi0new[m] / hi0new
                        info["icefree_thick" if hi0new > hi0max else "thin_frazil" if hi0new == p["hfrazilmin"] and not q > hi0new else "mid_frazil"] += 1
                else:
                    hsurp[m] = vi0new[m] / aice[j, i]
                    vi0new[m] = C0
                    info["full_zero" if aice0[j, i] == C0 else "full_tiny"] += 1
            if vi0new[m] > C0:
                jl.append(m)
            if hsurp[m] > C0:
                kl.append(m)
        info["jcells"] += len(jl)
        info["kcells"] += len(kl)
        for n in range(ncat):                                                           # :1613-1698
            for m in kl:
                j, i = J[m], I[m]
                vsurp = hsurp[m] * a[n, j, i]
                vtmp = v[n, j, i] + vsurp
                if a[n, j, i] == C0 and v[n, j, i] == C0:
                    info["surplus_empty_cat"] += 1
                if C0 < v[n, j, i] <= puny:
                    info["surplus_tiny_v"] += 1
                if trc and tr_iage and vtmp > puny:
                    t[n, nt("nt_iage"), j, i] = (t[n, nt("nt_iage"), j, i] * v[n, j, i] + dt * vsurp) / vtmp
                    info["surplus_iage"] += 1
                if trc and tr_lvl and v[n, j, i] > puny:
                    t[n, nt("nt_vlvl"), j, i] = (t[n, nt("nt_vlvl"), j, i] * v[n, j, i] + t[n, nt("nt_alvl"), j, i] * vsurp) / vtmp
                    info["surplus_vlvl"] += 1
                v[n, j, i] = vtmp
            if mushy:
                for m in kl:
                    j, i = J[m], I[m]
                    vsurp = hsurp[m] * a[n, j, i]
                    vtmp = v[n, j, i] - vsurp
                    if trc and v[n, j, i] > C0:
                        q0, s0 = nt("nt_qice"), nt("nt_sice")
                        t[n, q0:q0 + nilyr, j, i] = update_vertical_tracers(t[n, q0:q0 + nilyr, j, i].copy(), vtmp, v[n, j, i], qi0new[m])
                        t[n, s0:s0 + nilyr, j, i] = update_vertical_tracers(t[n, s0:s0 + nilyr, j, i].copy(), vtmp, v[n, j, i], Si0new[m])
                        info["surplus_layers"] += 1
            else:
                for k in range(nilyr):
                    for m in kl:
                        j, i = J[m], I[m]
                        vsurp = hsurp[m] * a[n, j, i]
                        vtmp = v[n, j, i] - vsurp
                        if trc and v[n, j, i] > C0:
                            q, s = nt("nt_qice") + k, nt("nt_sice") + k
                            t[n, q, j, i] = (t[n, q, j, i] * vtmp + qi0new[m] * vsurp) / v[n, j, i]
                            t[n, s, j, i] = (t[n, s, j, i] * vtmp + Sprofile[m, k] * vsurp) / v[n, j, i]      # (departure: the cell's own profile)
                            info["surplus_layers"] += int(k == 0)
        vice1 = {}
        for m in jl:                                                                    # :1710-1765
            j, i = J[m], I[m]
            area1 = a[0, j, i]
            vice1[m] = v[0, j, i]
            a[0, j, i] = a[0, j, i] + ai0new[m]
            aice0[j, i] = aice0[j, i] - ai0new[m]
            v[0, j, i] = v[0, j, i] + vi0new[m]
            info["merge_empty_cat1"] += int(area1 == C0)
            if not trc:
                continue
            T0 = (t[0, nt("nt_Tsfc"), j, i] * area1 + Tf[j, i] * ai0new[m]) / a[0, j, i]
            info["tsfc_clamped"] += int(T0 > C0)
            t[0, nt("nt_Tsfc"), j, i] = _min(T0, C0)
            if tr_FY:
                info["fy_is_one"] += int(t[0, nt("nt_FY"), j, i] == C1 and area1 > C0)
                fy = (t[0, nt("nt_FY"), j, i] * area1 + ai0new[m]) / a[0, j, i]
                info["fy_clamped"] += int(fy > C1)
                t[0, nt("nt_FY"), j, i] = _min(fy, C1)
            if v[0, j, i] > puny:
                info["merge_v1_gt_puny"] += 1
                if tr_iage:
                    t[0, nt("nt_iage"), j, i] = (t[0, nt("nt_iage"), j, i] * vice1[m] + dt * vi0new[m]) / v[0, j, i]
                alvl = C0
                if tr_lvl:
                    alvl = t[0, nt("nt_alvl"), j, i]
                    t[0, nt("nt_alvl"), j, i] = (t[0, nt("nt_alvl"), j, i] * area1 + ai0new[m]) / a[0, j, i]
                    t[0, nt("nt_vlvl"), j, i] = (t[0, nt("nt_vlvl"), j, i] * vice1[m] + vi0new[m]) / v[0, j, i]
                if (tr.get("tr_pond_cesm") or tr.get("tr_pond_topo")) and tr.get("nt_apnd", 0) > 0:
                    t[0, nt("nt_apnd"), j, i] = t[0, nt("nt_apnd"), j, i] * area1 / a[0, j, i]
                    info["pond_at"] += 1
                elif tr.get("tr_pond_lvl") and tr.get("nt_apnd", 0) > 0:
                    if t[0, nt("nt_alvl"), j, i] > puny:
                        t[0, nt("nt_apnd"), j, i] = t[0, nt("nt_apnd"), j, i] * alvl * area1 / (t[0, nt("nt_alvl"), j, i] * a[0, j, i])
                        info["pond_lvl"] += 1
                    else:
                        info["pond_lvl_skipped"] += 1
            else:
                info["merge_v1_le_puny"] += 1
        for k in range(nilyr):                                                          # :1767-1788
            for m in jl:
                j, i = J[m], I[m]
                if trc and v[0, j, i] > C0:
                    q, s = nt("nt_qice") + k, nt("nt_sice") + k
                    t[0, q, j, i] = (t[0, q, j, i] * vice1[m] + qi0new[m] * vi0new[m]) / v[0, j, i]
                    t[0, s, j, i] = (t[0, s, j, i] * vice1[m] + Sprofile[m, k] * vi0new[m]) / v[0, j, i]
    return dict(qi0new=qi0new, Si0new=Si0new, vi0new=vi0new, ai0new=ai0new, hsurp=hsurp)


def lateral_melt_block(J, I, p, a, v, s, t, rside, meltl, fpond, fresh, fsalt, fhocn, info):
    """:1108-1215 on the cell list (J, I): the cells with rside > 0"""
    tr = p["tr"]
    ncat = a.shape[0]
    trc = p["ntrcr"] > 0
    nilyr, nslyr = (tr.get("nilyr", 0), tr.get("nslyr", 0)) if trc else (0, 0)
    dt, rhoi, rhos = p["dt"], p["rhoi"], p["rhos"]
    with np.errstate(all="ignore"):
        for n in range(ncat):
            for j, i in zip(J, I):
                rs = rside[j, i]
                dfresh = (rhos * s[n, j, i] + rhoi * v[n, j, i]) * rs / dt
                dfsalt = rhoi * v[n, j, i] * p["salinity"] * P001 * rs / dt
                fresh[j, i] = fresh[j, i] + dfresh
                fsalt[j, i] = fsalt[j, i] + dfsalt
                if tr.get("tr_pond_topo"):
                    dfpond = a[n, j, i] * t[n, tr["nt_apnd"] - 1, j, i] * t[n, tr["nt_hpnd"] - 1, j, i] * rs
                    f0 = fpond[j, i]
                    fpond[j, i] = fpond[j, i] - dfpond
                    info["fpond_changed"] += int(fpond[j, i] != f0)
                meltl[j, i] = meltl[j, i] + v[n, j, i] * rs
                a[n, j, i] = a[n, j, i] * (C1 - rs)
                v[n, j, i] = v[n, j, i] * (C1 - rs)
                s[n, j, i] = s[n, j, i] * (C1 - rs)
            for k in range(nilyr):
                for j, i in zip(J, I):
                    dfhocn = t[n, tr["nt_qice"] - 1 + k, j, i] * rside[j, i] / dt * v[n, j, i] / F(nilyr)
                    fhocn[j, i] = fhocn[j, i] + dfhocn
            for k in range(nslyr):
                for j, i in zip(J, I):
                    dfhocn = t[n, tr["nt_qsno"] - 1 + k, j, i] * rside[j, i] / dt * s[n, j, i] / F(nslyr)
                    fhocn[j, i] = fhocn[j, i] + dfhocn


def reduce_area_block(J, I, hin0, a, v, ai, vi, info):
    """ice_itd.F90:776-804 on the tmask cells (J, I); a, v, ai, vi (ny, nx): category 1"""
    with np.errstate(all="ignore"):
        for j, i in zip(J, I):
            hi0 = vi[j, i] / ai[j, i] if ai[j, i] > C0 else C0
            hi1 = v[j, i] / a[j, i] if a[j, i] > C0 else C0
            did = False
            if hi1 <= hin0 and hin0 > C0:
                a[j, i] = v[j, i] / hin0
                hi1 = F(hin0)
                info["reduce_hin"] += 1
                did = True
            if a[j, i] > C0:
                dhi = hi1 - hi0
                if dhi < C0:
                    hi1 = v[j, i] / a[j, i]
                    a[j, i] = C2 * v[j, i] / (hi1 + hi0)
                    info["reduce_dhi"] += 1
                    did = True
            info["reduce_none"] += int(not did)


def new_ice_lateral_melt(blocks, tmask, p, y, debug=None, after_new_ice=None):
    """ice_step_mod.F90:875-960 for every block in turn, on the arrays of the dict y (in place): aicen_init, vicen_init, aicen, vicen, vsnon,
    trcrn, aice, aice0, frzmlt, Tf, sss, rside, salinz, frazil, frz_onset (or None), meltl, fpond (or None), fresh, fsalt, fhocn.
    Returns one info record of counts per block (INFO_KEYS).  debug: a list that receives add_new_ice's locals per block.
    after_new_ice: called with the block number once add_new_ice has run on it and before lateral_melt does."""
    nb, ncat, ny, nx = y["aicen"].shape
    trcrn = y["trcrn"] if y.get("trcrn") is not None else np.zeros((nb, ncat, 0, ny, nx))
    infos = []
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        info = {q: 0 for q in INFO_KEYS}
        infos.append(info)
        phys = [(j, i) for j in range(jlo - 1, jhi) for i in range(ilo - 1, ihi)]
        lst = [(j, i) for j, i in phys if tmask[b, j, i] != 0]
        J = np.array([c[0] for c in lst], dtype=np.int64)
        I = np.array([c[1] for c in lst], dtype=np.int64)
        fo = y["frz_onset"][b] if y.get("frz_onset") is not None else None
        loc = add_new_ice_block(J, I, p, y["aicen"][b], y["vicen"][b], trcrn[b], y["aice0"][b], y["aice"][b], y["frzmlt"][b], y["frazil"][b], fo,
                                y["fresh"][b], y["fsalt"][b], y["Tf"][b], y["sss"][b], y["salinz"][b], info)
        if debug is not None:
            debug.append(dict(loc, J=J, I=I))
        if after_new_ice is not None:
            after_new_ice(b)
        ml = [(j, i) for j, i in lst if y["rside"][b, j, i] > C0]                       # (departure: tmask cells)
        for j, i in lst:
            r = y["rside"][b, j, i]
            info["rside_nonpos" if not r > C0 else "rside_one" if r == C1 else "rside_part"] += 1
            info["untouched"] += int(not r > C0 and not y["frzmlt"][b, j, i] > C0)
        Jm = np.array([c[0] for c in ml], dtype=np.int64)
        Im = np.array([c[1] for c in ml], dtype=np.int64)
        fp = y["fpond"][b] if y.get("fpond") is not None else None
        lateral_melt_block(Jm, Im, p, y["aicen"][b], y["vicen"][b], y["vsnon"][b], trcrn[b], y["rside"][b], y["meltl"][b], fp, y["fresh"][b],
                           y["fsalt"][b], y["fhocn"][b], info)
        if ncat == 1:
            reduce_area_block(J, I, p["hin_max"][0], y["aicen"][b, 0], y["vicen"][b, 0], y["aicen_init"][b, 0], y["vicen_init"][b, 0], info)
    return infos


SNAP = ["aicen", "vicen", "vsnon", "trcrn", "aice", "aice0", "frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn"]


def step_therm2(blocks, tmask, p, y, kitd, hi_min, first_ice=None, stages=None):
    """step_therm2 for every block: the frain line on every cell, aggregate_area, linear_itd (kitd = 1), add_new_ice, lateral_melt,
    reduce_area, cleanup_itd.  Every block runs one stage before any block runs the next, which equals the reference's block loop: no
    stage looks beyond its block.  Returns (infos, stop): stop = (stage, reason, block, i, j) or None.
    stages: a list that receives copies of the arrays of SNAP (and first_ice) after linear_itd, after add_new_ice, after lateral_melt /
    reduce_area and after cleanup_itd -- what tests/test_therm2_ref.py holds to the reference's record stage by stage."""
    tr = p["tr"]

    def snap():
        one = {q: y[q].copy() for q in SNAP if y.get(q) is not None}
        if first_ice is not None:
            one["first_ice"] = first_ice.copy()
        return one
    if y.get("frain") is not None:
        y["fresh"][:] = y["fresh"] + y["frain"] * y["aice"]                             # ice_step_mod.F90:804-809, ghost cells included
    for b in range(y["aicen"].shape[0]):
        nplitd.aggregate_area(y["aicen"][b], y["aice"][b], y["aice0"][b])
    if kitd == 1:
        _, stop = nplitd.linear_itd(blocks, tmask, p["ntrcr"], p["dep"], tr, p["hin_max"], hi_min, p["k"], y["aicen_init"], y["vicen_init"],
                                    y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["aice0"], y.get("fpond"))
        if stop:
            return None, (1,) + tuple(stop)
    hook = None
    if stages is not None:
        stages.append(snap())
        mid = snap()                                                                    # block by block: as add_new_ice leaves it

        def hook(b):
            for q in mid:
                mid[q][b] = first_ice[b] if q == "first_ice" else y[q][b]
    infos = new_ice_lateral_melt(blocks, tmask, p, y, after_new_ice=hook)
    if stages is not None:
        stages.append(mid)
        stages.append(snap())
    fl = {q: y[q] for q in ("fpond", "fresh", "fsalt", "fhocn") if y.get(q) is not None}
    _, stop = npitd.cleanup_itd(blocks, p["dt"], p["ntrcr"], p["dep"], tr, p["hin_max"], p["k"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"],
                                y["aice0"], y["aice"], fl, first_ice)
    if stages is not None:
        stages.append(snap())
    if stop:
        return infos, (3,) + tuple(stop)
    return infos, None
