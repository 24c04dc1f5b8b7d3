// evpk_therm1s.hip -- the rest of step_therm1 (source/ice_step_mod.F90:154-733) around thermo_vertical: two kernels, one in front of
// k_thermo_vertical (evpk_therm1.hip, which stays as it is) and one behind it.  Included by evpk_api.hip behind evpk_therm1.hip.
//   k_therm1_open    aice_init / aicen_init / vicen_init (:272-285, every cell of the block arrays); frzmlt_bottom_lateral
//                    (source/ice_therm_vertical.F90:611-834, AusCOM branch: cpchr = -cp_ocn rhow chio) -- rside, Tbot, fbot on every cell;
//                    per listed cell and category atmo_boundary_layer (source/ice_atmo.F90:82-483; sfctype 'ice', highfreq and formdrag
//                    .false.), the AusCOM strairxn = strairyn = 0 without calc_strair (:458-464), increment_age (source/ice_age.F90:45-75),
//                    update_FYarea (source/ice_firstyear.F90:57-105).  atmo_boundary_layer of category n reads only Tsfc(n) of entry and
//                    frzmlt_bottom_lateral only the state of entry, so running all of it before the first thermo_vertical call is the
//                    reference's result, not a reordering.
//   k_therm1_merge   per category in order: fswabsn (:565-571), compute_ponds_cesm (source/ice_meltpond_cesm.F90:61-197) on its own list
//                    (aicen > puny AFTER the vertical thermodynamics), merge_fluxes (source/ice_flux.F90:681-831) weighted with aicen_init
//                    over the list of entry.  One thread per cell: the category order gives the sums the reference's bits.
//                    Its LVL instantiations (evpk_step_therm1_lvl) run compute_ponds_lvl (source/ice_meltpond_lvl.F90:79-404) in the place
//                    of compute_ponds_cesm, on that routine's own list: physical cells with aicen alvl > puny**2, and tmask.
// The eight per-category results of atmo_boundary_layer (shcoef, lhcoef, strairxn, strairyn, Cdn_atm_ratio_n, Trefn, Qrefn, Urefn) are locals
// of step_therm1; here they are per-category planes, ZERO wherever the cell is not listed.  (The Fortran's block-wide `icells > 0` test only
// decides whether locals nobody reads -- merge_fluxes and thermo_vertical run over the same list -- hold zeros or the previous category's
// values.)  Cdn_atm_ratio_n without calc_strair is not set by the reference at all; here it is zero.
// Cell list: physical cells with tmask and aicen > puny, as k_thermo_vertical (its stated departure), so that the three kernels list the
// same cells; compute_ponds_cesm's list requires tmask too.  frzmlt_bottom_lateral's list is the reference's (physical cells with
// aice > puny and frzmlt < 0; land carries aice = 0).
// Operation order: the Fortran's, -ffp-contract=off.  min / max are a comparison and a select; sign(a, b) is copysign (b = -0 gives -|a|);
// x**2 is x*x; exp is dev_exp; log, atan and the real power deltaT**m2 are the fixed algorithms of evpk_fmath2.h; sqrt is the IEEE one.
// rdn = vonkar / log(zref / iceruf) and al2 = log(zref / zTrf) are computed as written.
// k_therm1_open runs one thread per cell of the block arrays that walks the categories, as the other column kernels do.  Measured against
// one thread per (cell, category) for the boundary-layer part (which has no cross-category dependence), the 2-D work on the threads of
// category 1: at 3600 x 2700, 5 categories the one call took 13.42 ms against 13.79 ms (medians of 6; profiles/step_therm1/), so that
// variant is not kept.
#pragma once

#define EVPK_HD __host__ __device__ __forceinline__
#include "evpk_fmath2.h"

namespace evpk {

// compiled-in constants (include/evpk.h cites the lines)
namespace th1s {
constexpr double vonkar = 0.4, zref = 10.0, iceruf = 0.0005, zvir = 0.606, cp_air = 1005.0, cp_wv = 1.81e3, gravit = 9.80616, Lsub = 2.835e6,
                 pi = 3.14159265358979323846, pih = 0.5 * pi, secday = 86400.0, rhofresh = 1000.0, Timelt = 0.0, m1 = 1.6e-6, m2 = 1.36,
                 floediam = 300.0, floeshape = 0.66, zTrf = 2.0, cpvir = cp_wv / cp_air - 1.0, Td = 2.0, rexp = 0.01, dpthhi = 0.9;
}  // namespace th1s

constexpr int T1S_NMERGE = 22;

struct Therm1sArgs {
    const double *aice, *frzmlt, *sst, *Tf, *strocnxT, *strocnyT, *uatm, *vatm, *wind, *zlvl, *potT, *Qa, *rhoa, *flw, *frain;       // (nb, ny, nx)
    const double *fswthrun;                                             // (nb, ncat, ny, nx)
    const int32_t *lmask_n, *lmask_s;                                   // (nb, ny, nx)
    double *aicen, *vicen, *vsnon, *trcrn;                              // the state: read by both kernels; iage / FY, apnd / hpnd written
    double *Cdn_atm, *rside, *fbot, *Tbot, *aice_init, *aicen_init, *vicen_init;
    double *shcoef, *lhcoef, *strairxn, *strairyn, *Cdn_atm_ratio_n, *Trefn, *Qrefn, *Urefn;       // (nb, ncat, ny, nx), written on every cell
    // what k_thermo_vertical left, per category
    const double *fswsfcn, *fswintn, *flwoutn, *evapn, *freshn, *fsaltn, *fhocnn, *fsensn, *flatn, *fsurfn, *fcondtopn, *melttn, *meltsn, *meltbn,
                 *congeln, *snoicen;
    // merge_fluxes' cumulative planes in its argument order: strairxT, strairyT, Cdn_atm_ratio, fsurf, fcondtop, fsens, flat, fswabs, flwout, evap,
    // Tref, Qref, Uref, fresh, fsalt, fhocn, fswthru, meltt, meltb, melts, congel, snoice
    double *m[T1S_NMERGE];
    int ncat, ntrcr_dim, nxb, nyb, nilyr, nslyr, nt_Tsfc, nt_qice, nt_qsno, nt_apnd, nt_hpnd, nt_iage, nt_FY, tr_iage, tr_FY, tr_pond_cesm,
        calc_strair, natmiter;
    double dt, yday, puny, rhoi, rhos, rhow, chio, ustar_min, hi_min, pndaspect, rfracmin, rfracmax;
    // tr_pond_lvl (the LVL instantiations of k_therm1_merge only; behind the members above so that theirs keep their places)
    const double *dhsn, *Tair;                                          // (nb, ncat, ny, nx), (nb, ny, nx)
    double *ffracn;                                                     // (nb, ncat, ny, nx), written on every cell
    int nt_alvl, nt_ipnd, nt_sice, frzpnd;                              // frzpnd: 0 'cesm', 1 'hlid'
    double dpscale, Lfresh, cp_ice;
};

// the unstable parts of the stability functions (ice_atmo.F90:208-212)
__device__ __forceinline__ double t1s_psimhu(double xd) {
    const double c1 = 1.0, c2 = 2.0, c8 = 8.0;
    return (evpk_log(((c1 + xd * (c2 + xd)) * (c1 + xd * xd)) / c8) - c2 * evpk_atan(xd)) + th1s::pih;
}
__device__ __forceinline__ double t1s_psixhu(double xd) {
    const double c1 = 1.0, c2 = 2.0;
    return c2 * evpk_log((c1 + xd * xd) / c2);
}

// the 2-D forcing atmo_boundary_layer reads, loaded once per cell
struct T1sAtm { double potT, Qa, rhoa, uatm, vatm, wind, zlvl; };

// atmo_boundary_layer on one listed cell and category; bc: its place in the per-category planes
__device__ __forceinline__ void t1s_boundary_layer(const Therm1sArgs &A, const T1sAtm &F, double Tsf, size_t ci, size_t bc) {
    using namespace th1s;
    const double c0 = 0.0, c1 = 1.0, c5 = 5.0, c10 = 10.0, c16 = 16.0, p5 = 0.5, p01 = 0.01;
    const double al2 = evpk_log(zref / zTrf);
    const double vmag = litd_max(c1, F.wind);                                            // :276 (umin = 1)
    const double rdn = vonkar / evpk_log(zref / iceruf);                                 // :282
    A.Cdn_atm[ci] = rdn * rdn;
    const double TsfK = Tsf + th1::Tffresh;                                              // :314-322
    const double qsat = th1::qqqice * dev_exp(-th1::TTTice / TsfK);
    const double ssq = qsat / F.rhoa;
    const double thva = F.potT * (c1 + zvir * F.Qa);
    const double delt = F.potT - TsfK;
    const double delq = F.Qa - ssq;
    const double alz = evpk_log(F.zlvl / zref);
    const double cp = cp_air * (c1 + cpvir * ssq);
    const double rhn = rdn, ren = rdn;                                                   // :329-335
    double ustar = rdn * vmag, tstar = rhn * delt, qstar = ren * delq;
    double hol = c0, stable = c0, psixh = c0, rd = c0, rh = c0, re = c0;
    _Pragma("unroll 1")
    for (int k = 0; k < A.natmiter; k++) {                                               // :343-379
        hol = (((vonkar * gravit) * F.zlvl) * (tstar / thva + qstar / (c1 / zvir + F.Qa))) / (ustar * ustar);
        hol = copysign(litd_min(fabs(hol), c10), hol);
        stable = p5 + copysign(p5, hol);
        double xqq = litd_max(sqrt(fabs(c1 - c16 * hol)), c1);
        xqq = sqrt(xqq);
        const double psimhs = -((0.7 * hol + (0.75 * (hol - 14.3)) * dev_exp(-0.35 * hol)) + 10.7);
        const double psimh = psimhs * stable + (c1 - stable) * t1s_psimhu(xqq);
        psixh = psimhs * stable + (c1 - stable) * t1s_psixhu(xqq);
        rd = rdn / (c1 + (rdn / vonkar) * (alz - psimh));
        rh = rhn / (c1 + (rhn / vonkar) * (alz - psixh));
        re = ren / (c1 + (ren / vonkar) * (alz - psixh));
        ustar = rd * vmag;
        tstar = rh * delt;
        qstar = re * delq;
    }
    double strx = c0, stry = c0, ratio = c0;
    if (A.calc_strair) {                                                                 // :428-434
        const double tau = (F.rhoa * ustar) * rd;
        strx = tau * F.uatm;
        stry = tau * F.vatm;
        ratio = ((rd * rd) / rdn) / rdn;
    }
    A.strairxn[bc] = strx; A.strairyn[bc] = stry; A.Cdn_atm_ratio_n[bc] = ratio;
    A.shcoef[bc] = (((F.rhoa * ustar) * cp) * rh) + c1;                                  // :454-455
    A.lhcoef[bc] = ((F.rhoa * ustar) * Lsub) * re;
    hol = (hol * zTrf) / F.zlvl;                                                         // :461-479
    double xqq = litd_max(c1, sqrt(fabs(c1 - c16 * hol)));
    xqq = sqrt(xqq);
    const double psix2 = ((-c5 * hol) * stable) + (c1 - stable) * t1s_psixhu(xqq);
    double fac = (rh / vonkar) * (((alz + al2) - psixh) + psix2);
    double Tref = F.potT - delt * fac;
    Tref = Tref - p01 * zTrf;
    fac = (re / vonkar) * (((alz + al2) - psixh) + psix2);
    A.Trefn[bc] = Tref;
    A.Qrefn[bc] = F.Qa - delq * fac;
    A.Urefn[bc] = (vmag * rd) / rdn;
}

template <int NC>
__global__ void __launch_bounds__(64) k_therm1_open(Slab s, const BlockDesc *bd, Therm1sArgs A) {
    using namespace th1s;
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    if (i > A.nxb) return;
    const int ncat = NC ? NC : A.ncat;
    const int b = blockIdx.z;
    const double c0 = 0.0, c1 = 1.0, puny = A.puny;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const BlockDesc d = bd[b];
    const bool ocean = itd_ocean(s, d, i, j);
    {
        const bool phys = i >= d.ilo && i <= d.ihi && j >= d.jlo && j <= d.jhi;
        const double aice = A.aice[ci];
        A.aice_init[ci] = aice;                                                          // ice_step_mod.F90:272-276
        // frzmlt_bottom_lateral (ice_therm_vertical.F90:698-829)
        double rside = c0, fbot = c0;
        const double Tbot = A.Tf[ci];
        const double frzmlt = A.frzmlt[ci];
        if (phys && aice > puny && frzmlt < c0) {
            const double cpchr = -((th1::cp_ocn * A.rhow) * A.chio);
            const double deltaT = litd_max(A.sst[ci] - Tbot, c0);
            const double sx = A.strocnxT[ci], sy = A.strocnyT[ci];
            double ustar = sqrt(sqrt(sx * sx + sy * sy) / A.rhow);
            ustar = litd_max(ustar, A.ustar_min);
            fbot = (cpchr * deltaT) * ustar;
            fbot = litd_max(fbot, frzmlt);
            const double wlat = m1 * evpk_pow_pos(deltaT, m2);
            rside = ((wlat * A.dt) * pi) / (floeshape * floediam);
            rside = litd_max(c0, litd_min(rside, c1));
            double fside = c0;
            const double rnslyr = (double)A.nslyr, rnilyr = (double)A.nilyr;
            for (int n = 1; n <= ncat; n++) {
                const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
                const double *t = A.trcrn + lo * A.ntrcr_dim * nn + o;
                const double vs = A.vsnon[bc], vi = A.vicen[bc];
                double etot = c0;
                for (int k = 0; k < A.nslyr; k++) etot = etot + (t[(size_t)(A.nt_qsno - 1 + k) * nn] * vs) / rnslyr;
                for (int k = 0; k < A.nilyr; k++) etot = etot + (t[(size_t)(A.nt_qice - 1 + k) * nn] * vi) / rnilyr;
                fside = fside + (rside * etot) / A.dt;
            }
            double xtmp = frzmlt / ((fbot + fside) + puny);
            xtmp = litd_min(xtmp, c1);
            fbot = fbot * xtmp;
            rside = rside * xtmp;
        }
        A.rside[ci] = rside; A.Tbot[ci] = Tbot; A.fbot[ci] = fbot;
    }
    T1sAtm F{};
    bool fy_n = false, fy_s = false;
    if (ocean) {
        F.potT = A.potT[ci]; F.Qa = A.Qa[ci]; F.rhoa = A.rhoa[ci]; F.uatm = A.uatm[ci]; F.vatm = A.vatm[ci]; F.wind = A.wind[ci]; F.zlvl = A.zlvl[ci];
        if (A.tr_FY) {                                                                   // ice_firstyear.F90:87-103
            fy_n = A.yday >= 259.0 && A.yday < 259.0 + A.dt / secday && A.lmask_n[ci] != 0;
            fy_s = A.yday >= 75.0 && A.yday < 75.0 + A.dt / secday && A.lmask_s[ci] != 0;
        }
    }
    _Pragma("unroll 1")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        const double aicen = A.aicen[bc];
        A.aicen_init[bc] = aicen;                                                        // ice_step_mod.F90:278-285
        A.vicen_init[bc] = A.vicen[bc];
        if (ocean && aicen > puny) {
            double *t = A.trcrn + lo * A.ntrcr_dim * nn + o;
            t1s_boundary_layer(A, F, t[(size_t)(A.nt_Tsfc - 1) * nn], ci, bc);
            if (A.tr_iage) { double *q = t + (size_t)(A.nt_iage - 1) * nn; *q = *q + A.dt; }
            if (A.tr_FY && (fy_n || fy_s)) t[(size_t)(A.nt_FY - 1) * nn] = c0;
        } else {
            A.shcoef[bc] = c0; A.lhcoef[bc] = c0; A.strairxn[bc] = c0; A.strairyn[bc] = c0; A.Cdn_atm_ratio_n[bc] = c0;
            A.Trefn[bc] = c0; A.Qrefn[bc] = c0; A.Urefn[bc] = c0;
        }
    }
}
template __global__ void __launch_bounds__(64) k_therm1_open<0>(Slab, const BlockDesc *, Therm1sArgs);
template __global__ void __launch_bounds__(64) k_therm1_open<5>(Slab, const BlockDesc *, Therm1sArgs);

// compute_ponds_lvl (source/ice_meltpond_lvl.F90:79-345) with brine_permeability (:351-404) and calculate_Tin_from_qin under l_brine
// (source/ice_therm_shared.F90:62-90) on one physical ocean cell and category, on the state thermo_vertical left; t: the category's tracer
// planes at this cell.  ffracn is written by the caller's zero and, under 'hlid', here.  ktherm is 1 (evpk_thermo_vertical refuses
// anything else), so the drainage runs whenever hpondn > 0 and dpscale > puny; the nilyr enthalpy and salinity planes are read only then.
__device__ __forceinline__ void t1s_ponds_lvl(const Therm1sArgs &A, double *t, size_t nn, size_t bc, size_t ci, double aicen) {
    using namespace th1s;
    const double c0 = 0.0, c1 = 1.0, c2 = 2.0, c4 = 4.0, c10 = 10.0, p5 = 0.5, puny = A.puny;
    const double viscosity_dyn = 1.79e-3;                                                // drivers/cice/ice_constants.F90:42
    double *apnd = t + (size_t)(A.nt_apnd - 1) * nn, *hpnd = t + (size_t)(A.nt_hpnd - 1) * nn, *ipnd = t + (size_t)(A.nt_ipnd - 1) * nn;
    const double alvl = t[(size_t)(A.nt_alvl - 1) * nn];
    if (!(aicen * alvl > puny * puny)) return;                                           // :187-196
    const double hpnd0 = *hpnd, apnd0 = *apnd;
    double volpn = ((hpnd0 * aicen) * alvl) * apnd0;                                     // :177-178
    const double hi = A.vicen[bc] / aicen, hs = A.vsnon[bc] / aicen;
    double apondn, hpondn, hlid = c0;
    if (hi < A.hi_min) {                                                                 // :206-215
        apondn = c0; hpondn = c0; volpn = c0; hlid = c0;
    } else {
        apondn = apnd0 * alvl;
        const double rfrac = A.rfracmin + (A.rfracmax - A.rfracmin) * aicen;             // ice_step_mod.F90:624
        double dvn = ((rfrac / rhofresh) * ((A.melttn[bc] * A.rhoi + A.meltsn[bc] * A.rhos) + A.frain[ci] * A.dt)) * aicen;       // :228-230
        if (A.frzpnd == 0) {                                                             // 'cesm' (:233-236)
            const double Tp = Timelt - Td;
            const double dTs = litd_max(Tp - t[(size_t)(A.nt_Tsfc - 1) * nn], c0);
            dvn = dvn - volpn * (c1 - dev_exp((rexp * dTs) / Tp));
        } else {                                                                         // 'hlid' (:238-267)
            hlid = *ipnd;
            double dhlid;
            if (dvn == c0) {
                const double Ts = A.Tair[ci] - th1::Tffresh;
                if (Ts < c0) {
                    const double bdt = ((((-c2) * Ts) * th1::kice) * A.dt) / (A.rhoi * A.Lfresh);
                    dhlid = p5 * sqrt(bdt);
                    if (hlid > dhlid) dhlid = (p5 * bdt) / hlid;
                    dhlid = litd_min(dhlid, (hpnd0 * rhofresh) / A.rhoi);
                    hlid = hlid + dhlid;
                } else {
                    dhlid = c0;
                }
            } else {
                const double fsurfn = A.fsurfn[bc];
                dhlid = litd_max((fsurfn * A.dt) / (A.rhoi * A.Lfresh), c0);
                dhlid = -litd_min(dhlid, hlid);
                hlid = litd_max(hlid + dhlid, c0);
                if (hs - A.dhsn[bc] < puny) {
                    double ffrac = c1;
                    if (fsurfn > puny) ffrac = litd_min((((-dhlid) * A.rhoi) * A.Lfresh) / (A.dt * fsurfn), c1);
                    A.ffracn[bc] = ffrac;
                }
            }
            const double alid = apondn * aicen;
            dvn = dvn - ((dhlid * alid) * A.rhoi) / rhofresh;
        }
        volpn = volpn + dvn;
        if (volpn <= c0) { volpn = c0; apondn = c0; }                                    // :274-277
        if (apondn * aicen > puny) {                                                     // existing ponds (:279-284)
            apondn = litd_max(c0, litd_min(alvl, apondn + (0.5 * dvn) / ((A.pndaspect * apondn) * aicen)));
            hpondn = c0;
            if (apondn > puny) hpondn = volpn / (apondn * aicen);
        } else if (alvl * aicen > c10 * puny) {                                          // new ponds (:286-288)
            apondn = litd_min(sqrt(volpn / (A.pndaspect * aicen)), alvl);
            hpondn = A.pndaspect * apondn;
        } else {                                                                         // melt water runs off deformed ice (:290-293)
            apondn = c0; hpondn = c0;
        }
        apondn = litd_max(apondn, c0);
        hpondn = litd_min(hpondn, ((A.rhow - A.rhoi) * hi - A.rhos * hs) / rhofresh);    // :297
        apondn = apondn * aicen;
        volpn = hpondn * apondn;
        if (volpn <= c0) { volpn = c0; apondn = c0; hpondn = c0; hlid = c0; }            // :303-308
        if (hpondn > c0 && A.dpscale > puny) {                                           // :316-331 (ktherm = 1)
            const double draft = (A.rhos * hs + A.rhoi * hi) / A.rhow + hpondn;
            double deltah = (hpondn + hi) - draft;
            const double pressure_head = (gravit * A.rhow) * litd_max(deltah, c0);
            double phimin = c0;
            _Pragma("unroll 1")
            for (int k = 0; k < A.nilyr; k++) {                                          // brine_permeability (:384-402)
                const double qin = t[(size_t)(A.nt_qice - 1 + k) * nn], salin = t[(size_t)(A.nt_sice - 1 + k) * nn];
                const double Tmlt = (-salin) * th1::depressT;
                const double aa1 = A.cp_ice;                                             // ice_therm_shared.F90:80-84
                const double bb1 = (((th1::cp_ocn - A.cp_ice) * Tmlt) - qin / A.rhoi) - A.Lfresh;
                const double cc1 = A.Lfresh * Tmlt;
                const double Tin = litd_min((-bb1 - sqrt(bb1 * bb1 - (c4 * aa1) * cc1)) / (c2 * aa1), Tmlt);
                const double Sbr = c1 / (1.0e-3 - th1::depressT / Tin);
                double phi = salin / Sbr;
                if (phi < 0.05) phi = c0;
                if (k == 0 || phi < phimin) phimin = phi;
            }
            const double perm = 3.0e-8 * ((phimin * phimin) * phimin);
            const double drain = (((perm * pressure_head) * A.dt) / (viscosity_dyn * hi)) * A.dpscale;
            deltah = litd_min(drain, hpondn);
            const double dvd = (-deltah) * apondn;
            volpn = volpn + dvd;
            apondn = litd_max(c0, litd_min(apondn + (0.5 * dvd) / (A.pndaspect * apondn), alvl * aicen));
            hpondn = c0;
            if (apondn > puny) hpondn = volpn / apondn;
        }
    }
    *hpnd = hpondn;                                                                      // :339-341
    *apnd = apondn / (aicen * alvl);
    if (A.frzpnd == 1) *ipnd = hlid;
}

// LVL = 1: tr_pond_lvl -- compute_ponds_lvl at the reference's call site (ice_step_mod.F90:623-642) in place of compute_ponds_cesm, and
// ffracn = 0 on every cell of the block arrays (ice_meltpond_lvl.F90:175-181).  LVL = 0 is the kernel as it was.
template <int NC, int LVL>
__global__ void __launch_bounds__(64) k_therm1_merge(Slab s, const BlockDesc *bd, Therm1sArgs A) {
    using namespace th1s;
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if constexpr (LVL) {
        const int nc = NC ? NC : A.ncat;
        const size_t pn = (size_t)A.nyb * A.nxb, po = (size_t)(j - 1) * A.nxb + (i - 1);
        for (int n = 0; n < nc; n++) A.ffracn[((size_t)b * nc + n) * pn + po] = 0.0;
    }
    if (!itd_ocean(s, bd[b], i, j)) return;
    const int ncat = NC ? NC : A.ncat;
    const double c0 = 0.0, c1 = 1.0, puny = A.puny;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    double m[T1S_NMERGE];
    bool any = false;
    _Pragma("unroll 1")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        const double aicen = A.aicen[bc];
        if constexpr (LVL) {
            t1s_ponds_lvl(A, A.trcrn + lo * A.ntrcr_dim * nn + o, nn, bc, ci, aicen);
        } else if (A.tr_pond_cesm && aicen > puny) {                                     // ice_meltpond_cesm.F90:124-193
            double *t = A.trcrn + lo * A.ntrcr_dim * nn + o;
            double *apnd = t + (size_t)(A.nt_apnd - 1) * nn, *hpnd = t + (size_t)(A.nt_hpnd - 1) * nn;
            const double rfrac = A.rfracmin + (A.rfracmax - A.rfracmin) * aicen;         // ice_step_mod.F90:610
            double volpn = ((*hpnd) * (*apnd)) * aicen;
            const double hi = A.vicen[bc] / aicen;
            double apondn = c0, hpondn = c0;
            if (!(hi < A.hi_min)) {
                volpn = volpn + ((rfrac / rhofresh) * ((A.melttn[bc] * A.rhoi + A.meltsn[bc] * A.rhos) + A.frain[ci] * A.dt)) * aicen;
                const double Tp = Timelt - Td;
                const double dTs = litd_max(Tp - t[(size_t)(A.nt_Tsfc - 1) * nn], c0);
                volpn = volpn * dev_exp((rexp * dTs) / Tp);
                volpn = litd_max(volpn, c0);
                apondn = litd_min(sqrt(volpn / (A.pndaspect * aicen)), c1);
                hpondn = A.pndaspect * apondn;
                apondn = apondn * aicen;
                hpondn = litd_min(hpondn, dpthhi * hi);
            }
            *apnd = apondn / aicen;
            *hpnd = hpondn;
        }
        const double w = A.aicen_init[bc];
        if (w > puny) {                                                                  // ice_flux.F90:790-829 over the list of entry
            if (!any) {
                _Pragma("unroll")
                for (int q = 0; q < T1S_NMERGE; q++) m[q] = A.m[q][ci];
                any = true;
            }
            const double fswthrun = A.fswthrun[bc];
            const double fswabsn = (A.fswsfcn[bc] + A.fswintn[bc]) + fswthrun;           // ice_step_mod.F90:567-569
            m[0] = m[0] + A.strairxn[bc] * w;
            m[1] = m[1] + A.strairyn[bc] * w;
            m[2] = m[2] + A.Cdn_atm_ratio_n[bc] * w;
            m[3] = m[3] + A.fsurfn[bc] * w;
            m[4] = m[4] + A.fcondtopn[bc] * w;
            m[5] = m[5] + A.fsensn[bc] * w;
            m[6] = m[6] + A.flatn[bc] * w;
            m[7] = m[7] + fswabsn * w;
            m[8] = m[8] + (A.flwoutn[bc] - (c1 - th1::emissivity) * A.flw[ci]) * w;
            m[9] = m[9] + A.evapn[bc] * w;
            m[10] = m[10] + A.Trefn[bc] * w;
            m[11] = m[11] + A.Qrefn[bc] * w;
            m[12] = m[12] + A.Urefn[bc] * w;
            m[13] = m[13] + A.freshn[bc] * w;
            m[14] = m[14] + A.fsaltn[bc] * w;
            m[15] = m[15] + A.fhocnn[bc] * w;
            m[16] = m[16] + fswthrun * w;
            m[17] = m[17] + A.melttn[bc] * w;
            m[18] = m[18] + A.meltbn[bc] * w;
            m[19] = m[19] + A.meltsn[bc] * w;
            m[20] = m[20] + A.congeln[bc] * w;
            m[21] = m[21] + A.snoicen[bc] * w;
        }
    }
    if (any) {
        _Pragma("unroll")
        for (int q = 0; q < T1S_NMERGE; q++) A.m[q][ci] = m[q];
    }
}
template __global__ void __launch_bounds__(64) k_therm1_merge<0, 0>(Slab, const BlockDesc *, Therm1sArgs);
template __global__ void __launch_bounds__(64) k_therm1_merge<5, 0>(Slab, const BlockDesc *, Therm1sArgs);
template __global__ void __launch_bounds__(64) k_therm1_merge<0, 1>(Slab, const BlockDesc *, Therm1sArgs);
template __global__ void __launch_bounds__(64) k_therm1_merge<5, 1>(Slab, const BlockDesc *, Therm1sArgs);

}  // namespace evpk
