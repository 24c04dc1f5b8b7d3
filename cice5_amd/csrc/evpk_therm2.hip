// evpk_therm2.hip -- what step_therm2 (source/ice_step_mod.F90:741-995) does between linear_itd and cleanup_itd, on the device and on the
// caller's block arrays as they are: add_new_ice (source/ice_therm_itd.F90:1239-1850, l_conservation_check = .false.) with
// update_vertical_tracers (:967-1033) and the mushy liquidus (ice_therm_mushy.F90:43-123, :3687-3756, :3903-3918), lateral_melt (:1043-1217)
// and, for ncat = 1, reduce_area (ice_itd.F90:743-806).  Included by evpk_api.hip (one translation unit) behind evpk_itd.hip.
//
// Neither routine looks beyond its own cell: add_new_ice's jcells / kcells lists are compressions of the ocean cells, lateral_melt's list is
// rside > 0.  Hence two kernels, one thread per cell of the block arrays:
//   k_therm2_open    every cell, ghost cells included: the frain line (ice_step_mod.F90:804-809) on the aice of entry, then aggregate_area
//   k_therm2_leads   physical ocean cells: add_new_ice, lateral_melt for n = 1 .. ncat (n outer, layers inner), reduce_area.  A cell with
//                    frzmlt <= 0 and rside <= 0 writes frazil and leaves (ncat = 1: after reduce_area); it touches no tracer
// <NC, NL>: NC = 5, NL = 4 keeps the layer profiles of update_vertical_tracers in registers (unrolled loops, selects); <0, 0> is generic.
// Only + - * /, comparisons and selects, in the Fortran's operation order; -ffp-contract=off.
#pragma once

namespace evpk {

constexpr int T2_MAXL = 8;          // nilyr, nslyr at most

struct Therm2Args {
    const double *aicen_init, *vicen_init;                      // (nb, ncat, ny, nx); read for ncat = 1 only (reduce_area)
    const double *frain, *frzmlt, *Tf, *sss, *rside;            // (nb, ny, nx); frain may be null
    const double *salinz;                                       // (nb, nilyr + 1, ny, nx)
    double *frazil, *frz_onset, *meltl;                         // (nb, ny, nx); frz_onset may be null
    int ktherm, update_ocn_f, nt_sice, nt_iage, nt_FY, nt_vlvl, tr_pond_cesm, tr_pond_lvl;
    double yday, hfrazilmin, phi_init, dSin0_frazil, cp_ocn, rhow, hi0max;
};

// the liquidus parameters of ice_therm_mushy.F90:43-123, in that file's expression order (bz1 = 0.0: J1 = -0.0, O1 = +0.0)
namespace liq {
constexpr double c1 = 1.0, c1000 = 1000.0;
constexpr double az1 = -18.48, bz1 = 0.0, az2 = -10.3085, bz2 = 62.4;
constexpr double Tb = -7.6362968855167352, Sb = 123.66702800276086;
constexpr double az1p = az1 / c1000, bz1p = bz1 / c1000, az2p = az2 / c1000, bz2p = bz2 / c1000;
constexpr double J1 = bz1 / az1, K1 = c1 / c1000, L1 = (c1 + bz1p) / az1, J2 = bz2 / az2, K2 = c1 / c1000, L2 = (c1 + bz2p) / az2;
constexpr double M1 = az1, N1 = -az1p, O1 = -bz1 / az1, M2 = az2, N2 = -az2p, O2 = -bz2 / az2;
}  // namespace liq

// liquidus_brine_salinity_mush (:3687-3710): the merge(c1, c0, ...) masks stay multiplications
__device__ __forceinline__ double t2_liquidus_brine_salinity(double T) {
    const double c0 = 0.0, c1 = 1.0;
    const double t_high = T > liq::Tb ? c1 : c0, lsubzero = T <= c0 ? c1 : c0;
    double Sbr = ((T + liq::J1) / (liq::K1 * T + liq::L1)) * t_high + ((T + liq::J2) / (liq::K2 * T + liq::L2)) * (c1 - t_high);
    Sbr = Sbr * lsubzero;
    return Sbr;
}
// liquidus_temperature_mush (:3714-3733)
__device__ __forceinline__ double t2_liquidus_temperature(double Sbr) {
    const double c0 = 0.0, c1 = 1.0;
    const double t_high = Sbr <= liq::Sb ? c1 : c0;
    return ((Sbr / (liq::M1 + liq::N1 * Sbr)) + liq::O1) * t_high + ((Sbr / (liq::M2 + liq::N2 * Sbr)) + liq::O2) * (c1 - t_high);
}
// enthalpy_mush (:3737-3756) through liquid_fraction (:3903-3918)
__device__ __forceinline__ double t2_enthalpy_mush(double T, double S, double cp_ocn, double rhow, double cp_ice, double rhoi, double Lfresh,
                                                   double puny) {
    const double c1 = 1.0;
    const double Sbr = litd_max(t2_liquidus_brine_salinity(T), puny);
    const double phi = S / litd_max(Sbr, S);
    return phi * (cp_ocn * rhow - cp_ice * rhoi) * T + rhoi * cp_ice * T - (c1 - phi) * rhoi * Lfresh;
}

// update_vertical_tracers (:967-1033) on the nilyr layers of one tracer group of one category, t: layer 1 of the cell, layers nn apart
template <int NL>
__device__ __forceinline__ void t2_update_vertical(double *t, size_t nn, int nilyr_rt, double h1, double h2, double trc0) {
    const int nilyr = NL ? NL : nilyr_rt;
    constexpr int NA = NL ? NL : T2_MAXL;
    const double c0 = 0.0, rnilyr = (double)nilyr;
    double trc[NA], trc2[NA];
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) trc[k] = t[(size_t)k * nn];
    _Pragma("unroll")
    for (int k2 = 1; k2 <= nilyr; k2++) {
        double x = c0;
        const double z2a = ((double)(k2 - 1) * h2) / rnilyr, z2b = ((double)k2 * h2) / rnilyr;
        _Pragma("unroll")
        for (int k1 = 1; k1 <= nilyr; k1++) {
            const double z1a = ((double)(k1 - 1) * h1) / rnilyr, z1b = ((double)k1 * h1) / rnilyr;
            const double overlap = litd_max(litd_min(z1b, z2b) - litd_max(z1a, z2a), c0);
            x = x + overlap * trc[k1 - 1];
        }
        const double overlap = litd_max(litd_min(h2, z2b) - litd_max(h1, z2a), c0);
        x = x + overlap * trc0;
        trc2[k2 - 1] = (rnilyr * x) / h2;
    }
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) t[(size_t)k * nn] = trc2[k];
}

// the frain line on the aice of entry, then aggregate_area (ice_itd.F90:468-506), on every cell of every block
template <int NC>
__global__ void __launch_bounds__(64) k_therm2_open(ItdArgs A, const double *frain) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    const double c0 = 0.0, c1 = 1.0;
    const int ncat = NC ? NC : A.ncat;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    if (frain) A.fresh[ci] = A.fresh[ci] + frain[ci] * A.aice[ci];
    double aice = c0;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) aice = aice + A.aicen[((size_t)b * ncat + (n - 1)) * nn + o];
    A.aice[ci] = aice;
    A.aice0[ci] = fmax(c1 - aice, c0);
}
template __global__ void __launch_bounds__(64) k_therm2_open<0>(ItdArgs, const double *);
template __global__ void __launch_bounds__(64) k_therm2_open<5>(ItdArgs, const double *);

template <int NC, int NL>
__global__ void __launch_bounds__(64) k_therm2_leads(Slab s, const BlockDesc *bd, ItdArgs A, Therm2Args T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if (!itd_ocean(s, bd[b], i, j)) return;
    const double puny = A.puny, c0 = 0.0, c1 = 1.0, c2 = 2.0, c4 = 4.0, p1 = 0.1, p001 = 0.001;
    const int ncat = NC ? NC : A.ncat;
    const int nilyr = NL ? NL : A.nilyr;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const size_t cs = (size_t)A.ntrcr_dim * nn;
    double *t0 = A.trcrn + (size_t)b * ncat * cs + o;     // tracer 1 of category 1 of the cell
    const double dt = A.dt, rhoi = A.rhoi, rhos = A.rhos;
    const bool trc = A.ntrcr > 0;
    const bool tr_iage = T.nt_iage > 0, tr_FY = T.nt_FY > 0, tr_lvl = A.nt_alvl > 0 && T.nt_vlvl > 0, mushy = T.ktherm == 2;

    // ---- add_new_ice: the enthalpy and salinity of new ice (:1461-1493) ----
    const double frzmlt = T.frzmlt[ci], rside = T.rside[ci];
    double qi0new = -rhoi * A.Lfresh, Si0new = c0;
    if (mushy) {
        const double sss = T.sss[ci];
        Si0new = sss > c2 * T.dSin0_frazil ? sss - T.dSin0_frazil : sss * sss / (c4 * T.dSin0_frazil);
        const double Ti = litd_min(t2_liquidus_temperature(Si0new / T.phi_init), -p1);
        qi0new = t2_enthalpy_mush(Ti, Si0new, T.cp_ocn, T.rhow, A.cp_ice, rhoi, A.Lfresh, puny);
    }
    // volume, the diagnostics and the ocean fluxes (:1506-1545)
    const double fnew = litd_max(frzmlt, c0);
    double vi0new = -fnew * dt / qi0new;
    T.frazil[ci] = vi0new;
    if (T.frz_onset && vi0new > puny && T.frz_onset[ci] < puny) T.frz_onset[ci] = T.yday;
    const bool grows = vi0new > c0, melts = rside > c0;
    if (!grows && !melts && ncat != 1) return;            // (the flux increments of vi0new = 0 are -0: they change no bit)
    // fresh, fsalt: lateral_melt's increments, and add_new_ice's under update_ocn_f or ktherm = 2 -- else they keep every bit
    const bool fluxes = melts || (grows && (T.update_ocn_f || mushy));
    double fresh = fluxes ? A.fresh[ci] : c0, fsalt = fluxes ? A.fsalt[ci] : c0;
    if (T.update_ocn_f) {
        const double dfresh = -rhoi * vi0new / dt, dfsalt = A.salinity * p001 * dfresh;
        fresh = fresh + dfresh; fsalt = fsalt + dfsalt;
    } else if (mushy) {
        const double vi0tmp = fnew * dt / (rhoi * A.Lfresh);
        const double dfresh = -rhoi * (vi0new - vi0tmp) / dt, dfsalt = A.salinity * p001 * dfresh;
        fresh = fresh + dfresh; fsalt = fsalt + dfsalt;
    }
    // the distribution decision (:1551-1575)
    double hsurp = c0, ai0new = c0;
    double aice0 = c0;
    if (grows) {
        aice0 = A.aice0[ci];
        const double aice = A.aice[ci];
        if (aice0 > puny) {
            double hi0new = litd_max(vi0new / aice0, T.hfrazilmin);
            if (hi0new > T.hi0max && aice0 + puny < c1) {
                hi0new = T.hi0max;
                ai0new = aice0;
                const double vsurp = vi0new - ai0new * hi0new;
                hsurp = vsurp / aice;
                vi0new = ai0new * hi0new;
            } else {
                ai0new = vi0new / hi0new;
            }
        } else {
            hsurp = vi0new / aice;
            vi0new = c0;
        }
    }
    const bool jcell = vi0new > c0, kcell = hsurp > c0;
    // the state: category 1 for a jcell, every category for a kcell, lateral melt or reduce_area
    const bool all = kcell || melts || ncat == 1;
    double a[NA + 1], v[NA + 1];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        a[n] = c0; v[n] = c0;
        if (all || (jcell && n == 1)) {
            const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
            a[n] = A.aicen[bc]; v[n] = A.vicen[bc];
        }
    }
    // ---- the surplus over all categories (:1613-1698) ----
    if (kcell) {
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            double *t = t0 + (size_t)(n - 1) * cs;
            const double vsurp = hsurp * a[n];
            double vtmp = v[n] + vsurp;
            if (trc && tr_iage && vtmp > puny) {
                double *p = t + (size_t)(T.nt_iage - 1) * nn;
                *p = (*p * v[n] + dt * vsurp) / vtmp;
            }
            if (trc && tr_lvl && v[n] > puny) {
                double *p = t + (size_t)(T.nt_vlvl - 1) * nn;
                *p = (*p * v[n] + t[(size_t)(A.nt_alvl - 1) * nn] * vsurp) / vtmp;
            }
            v[n] = vtmp;
            vtmp = v[n] - vsurp;                                                                            // (v[n] is the new volume)
            if (trc && v[n] > c0) {
                double *q = t + (size_t)(A.nt_qice - 1) * nn, *sl = t + (size_t)(T.nt_sice - 1) * nn;
                if (mushy) {
                    t2_update_vertical<NL>(q, nn, nilyr, vtmp, v[n], qi0new);
                    t2_update_vertical<NL>(sl, nn, nilyr, vtmp, v[n], Si0new);
                } else {
                    _Pragma("unroll")
                    for (int k = 0; k < nilyr; k++) {
                        const double Sp = T.salinz[((size_t)b * (nilyr + 1) + k) * nn + o];
                        q[(size_t)k * nn] = (q[(size_t)k * nn] * vtmp + qi0new * vsurp) / v[n];
                        sl[(size_t)k * nn] = (sl[(size_t)k * nn] * vtmp + Sp * vsurp) / v[n];
                    }
                }
            }
        }
    }
    // ---- new ice into category 1 (:1710-1788) ----
    if (jcell) {
        const double area1 = a[1], vice1 = v[1];
        a[1] = a[1] + ai0new;
        aice0 = aice0 - ai0new;
        v[1] = v[1] + vi0new;
        A.aice0[ci] = aice0;
        if (trc) {
            double *t = t0;
            {
                double *p = t + (size_t)(A.nt_Tsfc - 1) * nn;
                const double x = (*p * area1 + T.Tf[ci] * ai0new) / a[1];
                *p = litd_min(x, c0);
            }
            if (tr_FY) {
                double *p = t + (size_t)(T.nt_FY - 1) * nn;
                const double x = (*p * area1 + ai0new) / a[1];
                *p = litd_min(x, c1);
            }
            if (v[1] > puny) {
                if (tr_iage) {
                    double *p = t + (size_t)(T.nt_iage - 1) * nn;
                    *p = (*p * vice1 + dt * vi0new) / v[1];
                }
                double alvl = c0, alvl1 = c0;
                if (tr_lvl) {
                    double *pa = t + (size_t)(A.nt_alvl - 1) * nn, *pv = t + (size_t)(T.nt_vlvl - 1) * nn;
                    alvl = *pa;
                    alvl1 = (alvl * area1 + ai0new) / a[1];
                    *pa = alvl1;
                    *pv = (*pv * vice1 + vi0new) / v[1];
                }
                if ((T.tr_pond_cesm || A.tr_pond_topo) && A.nt_apnd > 0) {
                    double *p = t + (size_t)(A.nt_apnd - 1) * nn;
                    *p = *p * area1 / a[1];
                } else if (T.tr_pond_lvl && A.nt_apnd > 0) {
                    if (alvl1 > puny) {
                        double *p = t + (size_t)(A.nt_apnd - 1) * nn;
                        *p = *p * alvl * area1 / (alvl1 * a[1]);
                    }
                }
            }
            if (v[1] > c0) {
                double *q = t + (size_t)(A.nt_qice - 1) * nn, *sl = t + (size_t)(T.nt_sice - 1) * nn;
                _Pragma("unroll")
                for (int k = 0; k < nilyr; k++) {
                    const double Sp = mushy ? Si0new : T.salinz[((size_t)b * (nilyr + 1) + k) * nn + o];
                    q[(size_t)k * nn] = (q[(size_t)k * nn] * vice1 + qi0new * vi0new) / v[1];
                    sl[(size_t)k * nn] = (sl[(size_t)k * nn] * vice1 + Sp * vi0new) / v[1];
                }
            }
        }
    }
    // ---- lateral_melt (:1108-1215): n outer, the layers inner ----
    double sn[NA + 1];
    if (melts) {
        double fpond = A.tr_pond_topo ? A.fpond[ci] : c0, fhocn = A.fhocn[ci], meltl = T.meltl[ci];
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
            const double *t = t0 + (size_t)(n - 1) * cs;
            sn[n] = A.vsnon[bc];
            const double dfresh = (rhos * sn[n] + rhoi * v[n]) * rside / dt;
            const double dfsalt = rhoi * v[n] * A.salinity * p001 * rside / dt;
            fresh = fresh + dfresh;
            fsalt = fsalt + dfsalt;
            if (A.tr_pond_topo) {
                const double dfpond = a[n] * t[(size_t)(A.nt_apnd - 1) * nn] * t[(size_t)(A.nt_hpnd - 1) * nn] * rside;
                fpond = fpond - dfpond;
            }
            meltl = meltl + v[n] * rside;
            a[n] = a[n] * (c1 - rside);
            v[n] = v[n] * (c1 - rside);
            sn[n] = sn[n] * (c1 - rside);
            A.vsnon[bc] = sn[n];
            if (trc) {
                for (int k = 0; k < nilyr; k++) {
                    const double dfhocn = t[(size_t)(A.nt_qice - 1 + k) * nn] * rside / dt * v[n] / (double)nilyr;
                    fhocn = fhocn + dfhocn;
                }
                for (int k = 0; k < A.nslyr; k++) {
                    const double dfhocn = t[(size_t)(A.nt_qsno - 1 + k) * nn] * rside / dt * sn[n] / (double)A.nslyr;
                    fhocn = fhocn + dfhocn;
                }
            }
        }
        if (A.tr_pond_topo) A.fpond[ci] = fpond;
        A.fhocn[ci] = fhocn;
        T.meltl[ci] = meltl;
    }
    // ---- reduce_area (ice_itd.F90:776-804), ncat = 1 ----
    bool reduced = false;
    if (ncat == 1) {
        const size_t bc = (size_t)b * nn + o;
        const double ai = T.aicen_init[bc], vi = T.vicen_init[bc];
        const double hi0 = ai > c0 ? vi / ai : c0;
        double hi1 = a[1] > c0 ? v[1] / a[1] : c0;
        if (hi1 <= A.hin_max[0] && A.hin_max[0] > c0) { a[1] = v[1] / A.hin_max[0]; hi1 = A.hin_max[0]; reduced = true; }
        if (a[1] > c0) {
            const double dhi = hi1 - hi0;
            if (dhi < c0) {
                hi1 = v[1] / a[1];
                a[1] = c2 * v[1] / (hi1 + hi0);
                reduced = true;
            }
        }
    }
    if (fluxes) { A.fresh[ci] = fresh; A.fsalt[ci] = fsalt; }
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (!(kcell || melts || ((jcell || reduced) && n == 1))) continue;
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        A.aicen[bc] = a[n]; A.vicen[bc] = v[n];
    }
}
template __global__ void __launch_bounds__(64) k_therm2_leads<0, 0>(Slab, const BlockDesc *, ItdArgs, Therm2Args);
template __global__ void __launch_bounds__(64) k_therm2_leads<5, 4>(Slab, const BlockDesc *, ItdArgs, Therm2Args);

}  // namespace evpk
