"""numpy / Python restatement of the level-ice melt pond scheme (tr_pond_lvl), written from the Fortran -- the checker of
evpk_step_therm1_lvl and evpk_step_radiation_dedd_lvl (tests/test_pondlvl_gpu.py), independent of the HIP code:
  compute_ponds_lvl with brine_permeability (source/ice_meltpond_lvl.F90:79-404) and calculate_Tin_from_qin under l_brine
  (source/ice_therm_shared.F90:62-90), as step_therm1 calls it per category (source/ice_step_mod.F90:623-642);
  the tr_pond_lvl block of run_dEdd (source/ice_shortwave.F90:1450-1514).
It composes with the existing checkers and edits none of them.

Thermodynamics (step_therm1_lvl): tests/nptherm1s.step runs first with no pond scheme, then compute_ponds_lvl is applied per block and
category.  That is the reference's result, not a reordering: within the category loop of step_therm1 nothing reads a pond tracer after
the pond call -- merge_fluxes takes the per-category fluxes and aicen_init -- and nothing of category n is touched again once its
thermo_vertical has returned, so the state, melttn, meltsn and fsurfn that compute_ponds_lvl(n) reads after the whole loop are those it
reads inside it; the routine writes only apnd, hpnd, ipnd of its own category and ffracn.
Shortwave (step_radiation_dedd_lvl): its own category loop -- shortwave_dEdd_set_snow as tests/npdedd.step_radiation_dedd has it, the
level-ice block, npdedd.shortwave_dEdd with the modified fs, hs, fp, hp, then the coupling_prep lines.

Parity: the tr_pond_lvl block of run_dEdd and compute_ponds_lvl / brine_permeability are held to reference-built records
(tests/golden/ref_sw_v_*.npz, ref_sw_p_*.npz, tests/test_shortwave_ref.py: bit for bit on LIBM); step_therm1_lvl as a whole is not.

min / max are a comparison and a select; sign(a, b) is copysign; x**3 is (x*x)*x; sqrt is IEEE; exp is a parameter (PORTS: the device's
bits).  Stated departure, shared with the device: compute_ponds_lvl's cell list requires tmask.  ktherm is 1, so the drainage runs
whenever hpondn > 0 and dpscale > puny.

Arrays are the block arrays in C order: (nb, ny, nx), (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx).
"""
from __future__ import annotations

import math

import numpy as np

from . import npdedd, nptherm1, nptherm1s

PUNY = 1.0e-11
C0, C1, C2, C4, C10, P5, P15 = 0.0, 1.0, 2.0, 4.0, 10.0, 0.5, 0.15
TD, REXP = 2.0, 0.01                                      # source/ice_meltpond_lvl.F90:167-169
VISCOSITY_DYN, GRAVIT, RHOFRESH, TIMELT = 1.79e-3, 9.80616, 1000.0, 0.0          # drivers/cice/ice_constants.F90:42, :36, :45, :54
KICE, DEPRESST, CP_OCN, TFFRESH = nptherm1.KICE, nptherm1.DEPRESST, nptherm1.CP_OCN, nptherm1.TFFRESH
HS_MIN, HPMIN = npdedd.HS_MIN, npdedd.HPMIN
FRZPND = {"cesm": 0, "hlid": 1}

THERM_KEYS = ["ponds_listed", "listed_tiny_area", "thin_ice", "cesm_freeze", "cesm_no_freeze", "lid_grows_open", "lid_grows_on_lid",
              "growth_clamped", "warm_air", "lid_melts_ffrac1", "lid_melts_ffrac_lt1", "lid_melts_snow", "volpn_le0", "existing_kept",
              "existing_lost", "new_ponds", "runoff", "freeboard_binds", "freeboard_negative", "drain_perm0", "drain_partial",
              "drain_complete", "dpscale_off"]
SW_KEYS = ["dhs_initialised", "dhs_reset", "linitonly_suppressed", "tapered", "rp_lt_p15", "rp_eq_p15", "tmp_one", "tmp_zero_hsn_reduced",
           "hpn_lt_hpmin", "fsn_cut", "ffracn_mid"]

_min, _max = nptherm1._min, nptherm1._max


def brine_permeability(nilyr, qicen, salin, p):
    """:351-404 with calculate_Tin_from_qin (l_brine); qicen, salin: lists of nilyr floats"""
    rhoi, cp_ice, Lfresh = p["rhoi"], p["cp_ice"], p["Lfresh"]
    cp_ocn = p.get("cp_ocn_build", CP_OCN)                 # (the AusCOM build fixes another value: tests/golden/make_ref_shortwave.py)
    phimin = C0
    for k in range(nilyr):
        Tmlt = (-salin[k]) * DEPRESST
        aa1 = cp_ice
        bb1 = (((cp_ocn - cp_ice) * Tmlt) - qicen[k] / rhoi) - Lfresh
        cc1 = Lfresh * Tmlt
        Tin = _min((-bb1 - math.sqrt(bb1 * bb1 - (C4 * aa1) * cc1)) / (C2 * aa1), Tmlt)
        Sbr = C1 / (1.0e-3 - np.float64(DEPRESST) / np.float64(Tin))
        phi = float(np.float64(salin[k]) / Sbr)
        if phi < 0.05:
            phi = C0
        if k == 0 or phi < phimin:
            phimin = phi
    return 3.0e-8 * ((phimin * phimin) * phimin)


def compute_ponds_lvl(blk, tmask, p, y, b, n, M, info):
    """:79-345 on category n (0-based) of block b, on the state thermo_vertical left"""
    ilo, ihi, jlo, jhi = blk
    tr = p["tr"]
    nt_Tsfc, nt_alvl, nt_apnd, nt_hpnd, nt_ipnd = (tr[k] - 1 for k in ("nt_Tsfc", "nt_alvl", "nt_apnd", "nt_hpnd", "nt_ipnd"))
    nt_qice, nt_sice, nilyr = tr["nt_qice"] - 1, tr["nt_sice"] - 1, tr["nilyr"]
    dt, rhoi, rhos, rhow, Lfresh = p["dt"], p["rhoi"], p["rhos"], p["rhow"], p["Lfresh"]
    pndaspect, dpscale, hlid_scheme = p["pndaspect"], p["dpscale"], FRZPND.get(p["frzpnd"], p["frzpnd"]) == 1
    t = y["trcrn"][b, n]
    y["ffracn"][b, n] = C0                                                               # :175-181, every cell
    with np.errstate(all="ignore"):
        for j in range(jlo - 1, jhi):
            for i in range(ilo - 1, ihi):
                aicen, alvl = float(y["aicen"][b, n, j, i]), float(t[nt_alvl, j, i])
                if not (tmask[b, j, i] and aicen * alvl > PUNY * PUNY):
                    continue
                info["ponds_listed"] += 1
                info["listed_tiny_area"] += int(aicen <= PUNY)
                hpnd0, apnd0 = float(t[nt_hpnd, j, i]), float(t[nt_apnd, j, i])
                volpn = ((hpnd0 * aicen) * alvl) * apnd0
                hi = float(y["vicen"][b, n, j, i]) / aicen
                hs = float(y["vsnon"][b, n, j, i]) / aicen
                hlid = C0
                if hi < p["hi_min"]:
                    apondn = hpondn = volpn = C0
                    info["thin_ice"] += 1
                else:
                    apondn = apnd0 * alvl
                    rfrac = p["rfracmin"] + (p["rfracmax"] - p["rfracmin"]) * aicen
                    dvn = ((rfrac / RHOFRESH) * ((float(y["melttn"][b, n, j, i]) * rhoi + float(y["meltsn"][b, n, j, i]) * rhos)
                                                 + float(y["frain"][b, j, i]) * dt)) * aicen
                    if not hlid_scheme:
                        Tp = TIMELT - TD
                        dTs = _max(Tp - float(t[nt_Tsfc, j, i]), C0)
                        info["cesm_freeze" if dTs > C0 and volpn > C0 else "cesm_no_freeze"] += 1
                        dvn = dvn - volpn * (C1 - M["exp"]((REXP * dTs) / Tp))
                    else:
                        hlid = float(t[nt_ipnd, j, i])
                        if dvn == C0:
                            Ts = float(y["Tair"][b, j, i]) - TFFRESH
                            if Ts < C0:
                                bdt = ((((-C2) * Ts) * KICE) * dt) / (rhoi * Lfresh)
                                dhlid = P5 * math.sqrt(bdt)
                                if hlid > dhlid:
                                    dhlid = (P5 * bdt) / hlid
                                    info["lid_grows_on_lid"] += 1
                                else:
                                    info["lid_grows_open"] += 1
                                cap = (hpnd0 * RHOFRESH) / rhoi
                                info["growth_clamped"] += int(cap < dhlid)
                                dhlid = _min(dhlid, cap)
                                hlid = hlid + dhlid
                            else:
                                dhlid = C0
                                info["warm_air"] += 1
                        else:
                            fsurfn = float(y["fsurfn"][b, n, j, i])
                            dhlid = _max((fsurfn * dt) / (rhoi * Lfresh), C0)
                            dhlid = -_min(dhlid, hlid)
                            hlid = _max(hlid + dhlid, C0)
                            if hs - float(y["dhsn"][b, n, j, i]) < PUNY:
                                ffrac = C1
                                if fsurfn > PUNY:
                                    ffrac = _min((((-dhlid) * rhoi) * Lfresh) / (dt * fsurfn), C1)
                                y["ffracn"][b, n, j, i] = ffrac
                                info["lid_melts_ffrac1" if ffrac == C1 else "lid_melts_ffrac_lt1"] += 1
                            else:
                                info["lid_melts_snow"] += 1
                        alid = apondn * aicen
                        dvn = dvn - ((dhlid * alid) * rhoi) / RHOFRESH
                    volpn = volpn + dvn
                    if volpn <= C0:
                        volpn = C0
                        apondn = C0
                        info["volpn_le0"] += 1
                    if apondn * aicen > PUNY:
                        apondn = _max(C0, _min(alvl, apondn + float(np.float64(0.5 * dvn) / np.float64((pndaspect * apondn) * aicen))))
                        hpondn = C0
                        if apondn > PUNY:
                            hpondn = volpn / (apondn * aicen)
                            info["existing_kept"] += 1
                        else:
                            info["existing_lost"] += 1
                    elif alvl * aicen > C10 * PUNY:
                        apondn = _min(math.sqrt(volpn / (pndaspect * aicen)), alvl)
                        hpondn = pndaspect * apondn
                        info["new_ponds"] += int(volpn > C0)
                    else:
                        apondn = hpondn = C0
                        info["runoff"] += 1
                    apondn = _max(apondn, C0)
                    limit = ((rhow - rhoi) * hi - rhos * hs) / RHOFRESH
                    info["freeboard_binds"] += int(C0 < limit < hpondn)
                    info["freeboard_negative"] += int(limit <= C0 < hpondn and apondn > C0)
                    hpondn = _min(hpondn, limit)
                    apondn = apondn * aicen
                    volpn = hpondn * apondn
                    if volpn <= C0:
                        volpn = apondn = hpondn = hlid = C0
                    if hpondn > C0 and not dpscale > PUNY:
                        info["dpscale_off"] += 1
                    if hpondn > C0 and dpscale > PUNY:
                        draft = (rhos * hs + rhoi * hi) / rhow + hpondn
                        deltah = (hpondn + hi) - draft
                        pressure_head = (GRAVIT * rhow) * _max(deltah, C0)
                        perm = brine_permeability(nilyr, [float(t[nt_qice + k, j, i]) for k in range(nilyr)],
                                                  [float(t[nt_sice + k, j, i]) for k in range(nilyr)], p)
                        drain = (((perm * pressure_head) * dt) / (VISCOSITY_DYN * hi)) * dpscale
                        info["drain_perm0" if perm == C0 else "drain_complete" if drain >= hpondn else "drain_partial"] += 1
                        deltah = _min(drain, hpondn)
                        dvd = (-deltah) * apondn
                        volpn = volpn + dvd
                        apondn = _max(C0, _min(apondn + (0.5 * dvd) / (pndaspect * apondn), alvl * aicen))
                        hpondn = C0
                        if apondn > PUNY:
                            hpondn = volpn / apondn
                t[nt_hpnd, j, i] = hpondn
                t[nt_apnd, j, i] = apondn / (aicen * alvl)
                if hlid_scheme:
                    t[nt_ipnd, j, i] = hlid


def therm_params(x, frzpnd, dpscale, conduct=0, **kw):
    """nptherm1s.params plus frzpnd ('cesm' / 'hlid') and dpscale"""
    p = nptherm1s.params(x, conduct, **kw)
    p["frzpnd"], p["dpscale"] = frzpnd, float(dpscale)
    return p


def apply_ponds(blocks, tmask, p, y, M=nptherm1s.PORTS):
    """compute_ponds_lvl on every block and category of a state nptherm1s.step has left; returns the info records per block"""
    infos = []
    for b, blk in enumerate(blocks):
        info = {k: 0 for k in THERM_KEYS}
        infos.append(info)
        for n in range(y["aicen"].shape[1]):
            compute_ponds_lvl(blk, tmask, p, y, b, n, M, info)
    return infos


def step_therm1_lvl(blocks, tmask, p, y, M=nptherm1s.PORTS, iters=None):
    """step_therm1 under tr_pond_lvl on every block: nptherm1s.step with no pond scheme, then compute_ponds_lvl per category (see the
    module docstring for why this is the reference's result).  y: nptherm1s.step's arrays plus dhsn (read), ffracn (written on every
    cell) and Tair.  Returns (infos, stop, pond infos); after a stop the ponds are not run"""
    q = dict(p, tr=dict(p["tr"], tr_pond_cesm=0))
    infos, stop, _ = nptherm1s.step(blocks, tmask, q, y, M, iters)
    if stop is not None:
        return infos, stop, None
    return infos, None, apply_ponds(blocks, tmask, p, y, M)


def step_radiation_dedd_lvl(blocks, tmask, p, y, M=npdedd.PORTS):
    """step_radiation (dEdd) under tr_pond_lvl and the albedo lines of coupling_prep on every block.  p: npdedd's (NAMELIST, rhos, tr) plus
    hs1, dt and linitonly; y: npdedd.step_radiation_dedd's arrays plus dhsn (in / out on the listed cells), ffracn and fsnow (read).
    Returns (npdedd's info records, the pond info records) per block"""
    exp = M["exp"]
    tr = p["tr"]
    ncat = y["aicen"].shape[1]
    nt_alvl, nt_apnd, nt_hpnd, nt_ipnd = (tr[k] - 1 for k in ("nt_alvl", "nt_apnd", "nt_hpnd", "nt_ipnd"))
    rhos, hs1, dt, init = p["rhos"], p["hs1"], p["dt"], bool(p["linitonly"])
    infos, pinfos = [], []
    pen = y.get("fswpenln")
    with np.errstate(all="ignore"):
        for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
            info = {k: 0 for k in npdedd.INFO_KEYS}
            pinfo = {k: 0 for k in SW_KEYS}
            infos.append(info)
            pinfos.append(pinfo)
            io = npdedd.iops(p, info)
            for q in npdedd.OUT3D + ["Sswabsn", "Iswabsn"]:
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
                t = y["trcrn"][b, n]
                Tsfc = t[tr["nt_Tsfc"] - 1][jj, ii]
                # shortwave_dEdd_set_snow (:3857-3880), as npdedd.step_radiation_dedd
                hs = vsno / aice
                fs = np.where(hs >= HS_MIN, (npdedd._min(hs / p["hs0"], C1) if p["hs0"] > PUNY else C1), C0)
                dTs = npdedd.TIMELT - Tsfc
                fT = -npdedd._min(dTs / p["dT_mlt"] - C1, C0)
                rsnw_nm = npdedd.RSNW_NONMELT - p["R_snw"] * npdedd.RSNW_SIG
                rsnw_nm = npdedd.RSNW_FRESH if npdedd.RSNW_FRESH > rsnw_nm else rsnw_nm
                rsnw_nm = p["rsnw_mlt"] if p["rsnw_mlt"] < rsnw_nm else rsnw_nm
                rsnw = rsnw_nm + (p["rsnw_mlt"] - rsnw_nm) * fT
                rsnw = npdedd._max(rsnw, npdedd.RSNW_FRESH)
                rsnw = npdedd._min(rsnw, p["rsnw_mlt"])
                # the tr_pond_lvl block (:1450-1514)
                alvl, apnd = t[nt_alvl][jj, ii], t[nt_apnd][jj, ii]
                ipn = (alvl * apnd) * t[nt_ipnd][jj, ii]
                dhs = y["dhsn"][b, n][jj, ii]
                snowfall = y["fsnow"][b][jj, ii] * dt
                would = (ipn > PUNY) & (dhs < PUNY) & (snowfall > HS_MIN)
                if not init:
                    dhs = np.where(would, hs - snowfall, dhs)
                    pinfo["dhs_initialised"] += int(would.sum())
                spn = hs - dhs
                gone = ipn * spn < PUNY
                if not init:
                    pinfo["dhs_reset"] += int((gone & (dhs != C0)).sum())
                    dhs = np.where(gone, C0, dhs)
                else:
                    pinfo["linitonly_suppressed"] += int((would | (gone & (dhs != C0))).sum())
                y["dhsn"][b, n][jj, ii] = dhs
                fp = apnd * alvl
                hp = t[nt_hpnd][jj, ii]
                ffr = y["ffracn"][b, n][jj, ii]
                pinfo["ffracn_mid"] += int(((ffr > C0) & (ffr < C1)).sum())
                fp = (C1 - ffr) * fp
                taper = (dhs > PUNY) & (spn >= PUNY) & (hs1 > PUNY)
                asnow = npdedd._min(spn / hs1, C1) if hs1 > PUNY else np.zeros(jj.size)
                fp = np.where(taper, (C1 - asnow) * fp, fp)
                pinfo["tapered"] += int((taper & (fp > C0)).sum())
                deep = hp > PUNY
                rp = (RHOFRESH * hp) / (RHOFRESH * hp + rhos * hs)
                hide = deep & (rp < P15)
                soak = deep & ~hide
                hmx = (hs * (RHOFRESH - rhos)) / RHOFRESH
                tmp = npdedd._max(C0, np.copysign(C1, hp - hmx))
                hpi = (RHOFRESH * hp + (rhos * hs) * tmp) / (RHOFRESH - rhos * (C1 - tmp))
                hs_new = hs - (hpi * fp) * (C1 - tmp)
                pinfo["rp_lt_p15"] += int(hide.sum())
                pinfo["rp_eq_p15"] += int((soak & (rp == P15) & (fp > C0)).sum())
                pinfo["tmp_one"] += int((soak & (tmp == C1)).sum())
                pinfo["tmp_zero_hsn_reduced"] += int((soak & (tmp == C0) & (hs_new < hs)).sum())
                hs = np.where(soak, hs_new, hs)
                hp = np.where(hide, C0, np.where(soak, hpi * tmp, hp))
                fp = np.where(hide, C0, np.where(soak, fp * tmp, fp))
                shallow = hp < HPMIN
                pinfo["hpn_lt_hpmin"] += int((shallow & (fp > C0)).sum())
                fp = np.where(shallow, C0, fp)
                pinfo["fsn_cut"] += int((C1 - fp < fs).sum())
                fs = npdedd._min(fs, C1 - fp)
                y["apeffn"][b, n][jj, ii] = fp
                y["snowfracn"][b, n][jj, ii] = fs
                npdedd.shortwave_dEdd(p, io, y, b, n, jj, ii, fs, hs, rsnw, fp, hp, exp, info)
            # coupling_prep (CICE_RunMod.F90:503-548), as npdedd.step_radiation_dedd: every cell of the block arrays
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
    return infos, pinfos
