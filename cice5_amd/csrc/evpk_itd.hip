// evpk_itd.hip -- cleanup_itd (source/ice_itd.F90:1514-1769: aggregate_area, the area check, rebin with shift_ice and compute_tracers,
// zap_small_areas I / II with zap_snow, zap_snow_temperature, the flux increments) and aggregate (:246-458) with the tendency lines of
// step_dynamics (ice_step_mod.F90:1183-1189) on the device, on the caller's block arrays as they are; at the end of the file linear_itd
// (source/ice_therm_itd.F90:69-958), which ends in the same shift_ice / compute_tracers.  Included by evpk_api.hip (one translation unit).
//
// One thread per cell of the block arrays.  rebin's shiftflag is one flag per BLOCK and per category boundary -- 2 (ncat - 1) boundaries,
// first upward, then downward: when any listed cell of a block (physical, aice > puny) shifts at a boundary, shift_ice runs for every
// listed cell of the block, which rewrites all its tracers as (aicen * trcrn) / aicen and resets categories with aicen <= puny, and
// compute_tracers zeroes the tracers of every other cell of the block (:1401).  A cell's own donor decisions depend on its own aicen /
// vicen / hicen only, and a pass of shift_ice in which it is no donor leaves those unchanged (hicen is recomputed from the same operands;
// the one exception, hicen(1) = hin_max(0) after the category-1 adjustment, is read at the very first boundary only).  Hence three kernels:
//   k_itd_scan   every cell: aggregate_area (aice, aice0); listed cells with tmask: the area check and a replay of rebin's area / volume part,
//                which ORs the boundaries at which the cell shifts into bmask[block] and records the reference's l_stop cases
//   k_itd_shift  physical ocean cells of the blocks with bmask != 0 (the others leave at once): the boundaries of bmask[block] with the
//                tracers -- the kernel that needs the registers (old and new state, parents, one tracer of every category)
//   k_itd_zap    physical ocean cells: zap I / II, the snow-temperature zap and the flux increments on the state rebin left; a cell that
//                zaps nothing writes nothing -- the common case reads aicen, vicen, vsnon, aice, aice0 and the snow enthalpies
// A stop is one 64-bit key, the smallest wins: block | stage (0 the area check, 1 + q boundary q in rebin's order, then zap I, zap II) |
// sub (shift_ice's four checks in their order; zap I: the category) | cell -- where the reference's loop does not exit (:1648-1655,
// :1040-1126) the cell field counts down so that the LAST failing cell wins, in zap_small_areas (which returns) it counts up.
// Same operation order as the Fortran, -ffp-contract=off: bit-comparable with the reference (tests/golden/ref_itd_*.npz).
#pragma once

namespace evpk {

enum { ITD_STOP_BOUNDS = 1, ITD_STOP_NEG_DAICE = 2, ITD_STOP_NEG_DVICE = 3, ITD_STOP_DAICE = 4, ITD_STOP_DVICE = 5, ITD_STOP_NEG_AICEN = 6,
       ITD_STOP_EXCESS = 7 };

struct ItdArgs {
    double *aicen, *vicen, *vsnon, *trcrn, *aice0, *aice;       // (nb, ncat, ny, nx) x 3, (nb, ncat, ntrcr_dim, ny, nx), (nb, ny, nx) x 2
    double *fpond, *fresh, *fsalt, *fhocn;                      // (nb, ny, nx) or nullptr
    int32_t *first_ice;                                         // (nb, ncat, ny, nx) or nullptr
    // aggregate only
    double *vice, *vsno, *trcr, *daidtd, *dvidtd, *dagedtd;
    int ncat, ntrcr, ntrcr_dim, nxb, nyb;
    int nt_Tsfc, nt_qice, nilyr, nt_qsno, nslyr, nt_alvl, nt_apnd, nt_hpnd, nt_fbri, nt_iage, tr_pond_topo, tr_brine;
    double dt, Tocnfrz, salinity, hs_min, cp_ice, Lfresh, Tmin, puny, rhoi, rhos;
    double hin_max[MAXCAT + 1];
    // per tracer (0-based), as RidgeArgs: acc how aicen * trcrn is built (0 area, 1 ice volume, 2 snow volume, 3 aicen * alvl, 4 aicen * apnd,
    // 5 aicen * alvl * apnd, 6 vicen * fbri, -1 no rule); rule, d1, d2: compute_tracer's rule (0: nt_Tsfc) and the parent slots + 1 (slot 0
    // alvl, 1 apnd, 2 fbri); slot: the slot this tracer fills + 1
    signed char acc[RG_MAXT], rule[RG_MAXT], d1[RG_MAXT], d2[RG_MAXT], slot[RG_MAXT];
};

__device__ __forceinline__ unsigned long long itd_key(int b, int stage, int sub, unsigned cellcode) {
    return ((unsigned long long)b << 48) | ((unsigned long long)stage << 40) | ((unsigned long long)sub << 32) | (unsigned long long)cellcode;
}

// boundary q of rebin's sequence (0 .. 2 (ncat - 1) - 1): the Fortran boundary n, the donor and the receiver category (1-based)
__device__ __forceinline__ void itd_boundary(int ncat, int q, bool &up, int &n, int &nd, int &nr) {
    up = q < ncat - 1;
    n = up ? q + 1 : 2 * (ncat - 1) - q;
    nd = up ? n : n + 1;
    nr = up ? n + 1 : n;
}

// shift_ice's range checks of one donor cell (:994-1033): may reset daice / dvice; returns -1 or the first failing check 0 .. 3 in the order
// of the error loops (:1040-1126)
__device__ __forceinline__ int itd_check(double &daice, double &dvice, double a, double v, double puny) {
    const double c0 = 0.0, c1 = 1.0;
    bool na = false, nv = false, ga = false, gv = false;
    if (daice < c0) { if (daice > -puny * a) { daice = c0; dvice = c0; } else na = true; }
    if (dvice < c0) { if (dvice > -puny * v) { daice = c0; dvice = c0; } else nv = true; }
    if (daice > a * (c1 - puny)) { if (daice < a * (c1 + puny)) { daice = a; dvice = v; } else ga = true; }
    if (dvice > v * (c1 - puny)) { if (dvice < v * (c1 + puny)) { daice = a; dvice = v; } else gv = true; }
    return na ? 0 : nv ? 1 : ga ? 2 : gv ? 3 : -1;
}

__device__ __forceinline__ bool itd_ocean(const Slab &s, const BlockDesc &d, int i, int j) {
    int si, sj;
    return ridge_listed(s, d, i, j, si, sj);
}

template <int NC>
__global__ void __launch_bounds__(64) k_itd_scan(Slab s, const BlockDesc *bd, ItdArgs A, unsigned *bmask, unsigned long long *key) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    const double puny = A.puny, c0 = 0.0, c1 = 1.0;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    double a[NA + 2], v[NA + 2], h[NA + 2];
    double aice = c0;                                                                                       // aggregate_area (:489-506)
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        a[n] = A.aicen[bc];
        aice = aice + a[n];
    }
    A.aice[ci] = aice;
    A.aice0[ci] = fmax(c1 - aice, c0);
    if (!itd_ocean(s, bd[b], i, j)) return;
    if (aice > c1 + puny || aice < -puny) { atomicMin(key, itd_key(b, 0, 0, 0xffffffffu - (unsigned)o)); return; }      // :1650
    if (!(aice > puny)) return;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        v[n] = A.vicen[((size_t)b * ncat + (n - 1)) * nn + o];
        h[n] = a[n] > puny ? v[n] / a[n] : c0;                                                              // :590-594
    }
    if (a[1] > puny && h[1] <= A.hin_max[0] && A.hin_max[0] > c0) { a[1] = v[1] / A.hin_max[0]; h[1] = A.hin_max[0]; }      // :605-610
    unsigned bits = 0;
    _Pragma("unroll")
    for (int q = 0; q < 2 * (ncat - 1); q++) {
        bool up; int n, nd, nr;
        itd_boundary(ncat, q, up, n, nd, nr);
        if (!(a[nd] > puny && (up ? h[nd] > A.hin_max[n] : h[nd] <= A.hin_max[n]))) continue;               // :632-633, :687-688
        bits |= 1u << q;
        double daice = a[nd], dvice = v[nd];
        const int bad = itd_check(daice, dvice, a[nd], v[nd], puny);
        if (bad >= 0) { atomicMin(key, itd_key(b, 1 + q, bad, 0xffffffffu - (unsigned)o)); break; }
        if (daice > c0) {                                                                                   // :1162-1166
            a[nd] = a[nd] - daice; a[nr] = a[nr] + daice;
            v[nd] = v[nd] - dvice; v[nr] = v[nr] + dvice;
        }
        _Pragma("unroll")
        for (int m = 1; m <= ncat; m++) h[m] = a[m] > puny ? v[m] / a[m] : c0;                              // :1227-1231
    }
    if (bits) atomicOr(&bmask[b], bits);
}
template __global__ void __launch_bounds__(64) k_itd_scan<0>(Slab, const BlockDesc *, ItdArgs, unsigned *, unsigned long long *);
template __global__ void __launch_bounds__(64) k_itd_scan<5>(Slab, const BlockDesc *, ItdArgs, unsigned *, unsigned long long *);

// aicen * trcrn with shift_ice's association (:919-975, :1191-1208): the base, then alvl, apnd / fbri, then the tracer
__device__ __forceinline__ double itd_product(int acc, double a, double v, double sn, double alvl, double apnd, double fbri, double t) {
    switch (acc) {
    case 0: return a * t;
    case 1: return v * t;
    case 2: return sn * t;
    case 3: return a * alvl * t;
    case 4: return a * apnd * t;
    case 5: return a * alvl * apnd * t;
    case 6: return v * fbri * t;
    default: return 0.0;
    }
}

// one call of shift_ice as a listed cell sees it: atrcrn from the old state, the transfer nd -> nr if the cell is a donor (nd > 0),
// compute_tracers on the new state -- one tracer at a time, the old and new values of the tracers that others hang on in registers
template <int NC>
__device__ __forceinline__ void itd_shift_tracers(const ItdArgs &A, int ncat, double *t0 /* trcrn of (b, category 1, tracer 1, cell) */, size_t nn,
                                                  const double *ao, const double *vo, const double *so, const double *an, const double *vn,
                                                  const double *sn, int nd, int nr, double daice, double dvice, double dvsnow) {
    constexpr int NA = NC ? NC : MAXCAT;
    double oldP[3][NA + 1], newP[3][NA + 1];
    const size_t cs = (size_t)A.ntrcr_dim * nn;                 // category stride
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const double *t = t0 + (size_t)(n - 1) * cs;
        oldP[0][n] = A.nt_alvl ? t[(size_t)(A.nt_alvl - 1) * nn] : 0.0;
        oldP[1][n] = A.nt_apnd ? t[(size_t)(A.nt_apnd - 1) * nn] : 0.0;
        oldP[2][n] = A.nt_fbri ? t[(size_t)(A.nt_fbri - 1) * nn] : 0.0;
        newP[0][n] = 0.0; newP[1][n] = 0.0; newP[2][n] = 0.0;          // (a parent that comes later in the table is still 0, :1401)
    }
    for (int it = 0; it < A.ntrcr; it++) {
        const int acc = A.acc[it], rule = A.rule[it], d1 = A.d1[it], d2 = A.d2[it], sl = A.slot[it];
        double told[NA + 1], atr[NA + 1];
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            told[n] = t0[(size_t)(n - 1) * cs + (size_t)it * nn];
            atr[n] = itd_product(acc, ao[n], vo[n], so[n], oldP[0][n], oldP[1][n], oldP[2][n], told[n]);
        }
        if (nd > 0) {
            double dat = 0.0;
            _Pragma("unroll")
            for (int n = 1; n <= ncat; n++)
                if (n == nd) dat = itd_product(acc, daice, dvice, dvsnow, oldP[0][n], oldP[1][n], oldP[2][n], told[n]);
            if (acc >= 0) {
                _Pragma("unroll")
                for (int n = 1; n <= ncat; n++) {
                    if (n == nd) atr[n] = atr[n] - dat;
                    if (n == nr) atr[n] = atr[n] + dat;
                }
            }
        }
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            const double p1 = d1 == 1 ? newP[0][n] : d1 == 2 ? newP[1][n] : d1 == 3 ? newP[2][n] : 0.0;
            const double p2 = d2 == 1 ? newP[0][n] : d2 == 2 ? newP[1][n] : d2 == 3 ? newP[2][n] : 0.0;
            const double r = compute_tracer(rule, atr[n], an[n], vn[n], sn[n], p1, p2, it + 1 == A.nt_fbri, A.Tocnfrz);
            if (sl == 1) newP[0][n] = r;
            else if (sl == 2) newP[1][n] = r;
            else if (sl == 3) newP[2][n] = r;
            t0[(size_t)(n - 1) * cs + (size_t)it * nn] = r;
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(64) k_itd_shift(Slab s, const BlockDesc *bd, ItdArgs A, const unsigned *bmask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    const unsigned bm = bmask[b];
    if (!bm) return;                                      // the common case: no cell of the block shifts
    if (!itd_ocean(s, bd[b], i, j)) return;
    const double puny = A.puny, c0 = 0.0;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const size_t cs = (size_t)A.ntrcr_dim * nn;
    double *t0 = A.trcrn + (size_t)b * ncat * cs + o;
    double a[NA + 2], v[NA + 2], sn[NA + 2], h[NA + 2];
    const double aice = A.aice[ci];                       // (k_itd_scan's)
    if (!(aice > puny)) {                                 // an unlisted cell of a block that shifts: trcrn(:,:,:) = c0 (:1401)
        for (int n = 0; n < ncat; n++)
            for (int it = 0; it < A.ntrcr; it++) t0[(size_t)n * cs + (size_t)it * nn] = c0;
        return;
    }
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        a[n] = A.aicen[bc]; v[n] = A.vicen[bc]; sn[n] = A.vsnon[bc];
    }
    unsigned dirty = 0;                                   // bit n - 1: aicen / vicen / vsnon of category n changed
    {                                                     // a listed cell: rebin (:578-726)
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) h[n] = a[n] > puny ? v[n] / a[n] : c0;
        if (a[1] > puny && h[1] <= A.hin_max[0] && A.hin_max[0] > c0) { a[1] = v[1] / A.hin_max[0]; h[1] = A.hin_max[0]; dirty |= 1u; }
        {
            _Pragma("unroll")
            for (int q = 0; q < 2 * (ncat - 1); q++) {
                if (!(bm & (1u << q))) continue;
                bool up; int n, nd, nr;
                itd_boundary(ncat, q, up, n, nd, nr);
                double ao[NA + 2], vo[NA + 2], so[NA + 2];
                _Pragma("unroll")
                for (int m = 1; m <= ncat; m++) { ao[m] = a[m]; vo[m] = v[m]; so[m] = sn[m]; }
                double daice = c0, dvice = c0, dvsnow = c0;
                bool donor = a[nd] > puny && (up ? h[nd] > A.hin_max[n] : h[nd] <= A.hin_max[n]);
                if (donor) {
                    daice = a[nd]; dvice = v[nd];
                    if (itd_check(daice, dvice, a[nd], v[nd], puny) >= 0) return;       // a stop (k_itd_scan has recorded it): the state is undefined
                    donor = daice > c0;                                                // :1137
                }
                if (donor) {                                                           // :1153-1171
                    const double worka = daice / a[nd];
                    a[nd] = a[nd] - daice; a[nr] = a[nr] + daice;
                    v[nd] = v[nd] - dvice; v[nr] = v[nr] + dvice;
                    dvsnow = sn[nd] * worka;
                    sn[nd] = sn[nd] - dvsnow; sn[nr] = sn[nr] + dvsnow;
                    dirty |= (1u << (nd - 1)) | (1u << (nr - 1));
                }
                if (A.ntrcr > 0) itd_shift_tracers<NC>(A, ncat, t0, nn, ao, vo, so, a, v, sn, donor ? nd : 0, nr, daice, dvice, dvsnow);
                _Pragma("unroll")
                for (int m = 1; m <= ncat; m++) h[m] = a[m] > puny ? v[m] / a[m] : c0;
            }
        }
    }
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (!(dirty & (1u << (n - 1)))) continue;
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        A.aicen[bc] = a[n]; A.vicen[bc] = v[n]; A.vsnon[bc] = sn[n];
    }
}
template __global__ void __launch_bounds__(64) k_itd_shift<0>(Slab, const BlockDesc *, ItdArgs, const unsigned *);
template __global__ void __launch_bounds__(64) k_itd_shift<5>(Slab, const BlockDesc *, ItdArgs, const unsigned *);

// zap_small_areas I / II, zap_snow_temperature and the flux increments of a physical ocean cell, on the state rebin left
template <int NC>
__global__ void __launch_bounds__(64) k_itd_zap(Slab s, const BlockDesc *bd, ItdArgs A, const unsigned *bmask, unsigned long long *key) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if (!itd_ocean(s, bd[b], i, j)) return;
    const double puny = A.puny, c0 = 0.0, c1 = 1.0, p001 = 0.001;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const size_t cs = (size_t)A.ntrcr_dim * nn;
    double *t0 = A.trcrn + (size_t)b * ncat * cs + o;
    double a[NA + 2], v[NA + 2], sn[NA + 2];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        a[n] = A.aicen[bc]; v[n] = A.vicen[bc]; sn[n] = A.vsnon[bc];
    }
    double aice = A.aice[ci], aice0 = A.aice0[ci];        // (k_itd_scan's: the sums over the state before rebin)
    unsigned dirty = 0;                                   // bit n - 1: aicen / vicen / vsnon of category n changed
    // the category-1 adjustment of rebin (:605-610) in a block that does not shift (k_itd_shift has made it in the others)
    if (!bmask[b] && aice > puny && a[1] > puny && v[1] / a[1] <= A.hin_max[0] && A.hin_max[0] > c0) { a[1] = v[1] / A.hin_max[0]; dirty |= 1u; }
    double dfpond = c0, dfresh = c0, dfsalt = c0, dfhocn = c0;
    bool zapped = false;
    const double dt = A.dt;
    // zap_small_areas I (:1872-2015)
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (a[n] < -puny) { atomicMin(key, itd_key(b, 2 * ncat, n, (unsigned)o)); return; }                   // :1881 (returns: the first one)
        if (!(fabs(a[n]) != c0 && fabs(a[n]) <= puny)) continue;
        zapped = true;
        double *t = t0 + (size_t)(n - 1) * cs;
        if (A.tr_pond_topo) { const double x = a[n] * t[(size_t)(A.nt_apnd - 1) * nn] * t[(size_t)(A.nt_hpnd - 1) * nn]; dfpond = dfpond - x; }
        for (int k = 0; k < A.nilyr; k++) {
            const double x = t[(size_t)(A.nt_qice - 1 + k) * nn] / dt * v[n] / (double)A.nilyr;
            dfhocn = dfhocn + x;
        }
        double x = (A.rhoi * v[n]) / dt;
        dfresh = dfresh + x;
        x = A.rhoi * v[n] * A.salinity * p001 / dt;
        dfsalt = dfsalt + x;
        aice0 = aice0 + a[n];
        a[n] = c0; v[n] = c0;
        for (int k = 0; k < A.nslyr; k++) {                                                                  // zap_snow (:2240-2268)
            x = t[(size_t)(A.nt_qsno - 1 + k) * nn] / dt * sn[n] / (double)A.nslyr;
            dfhocn = dfhocn + x;
        }
        x = (A.rhos * sn[n]) / dt;
        dfresh = dfresh + x;
        sn[n] = c0;
        dirty |= 1u << (n - 1);
        // :1947 qice = 0, :1972 Tsfc = Tocnfrz, :2251 qsno = 0, then tracers 2 .. ntrcr: 0, fbri 1 (:1991-2007) -- tracer 1 is not in that loop
        if (A.nt_Tsfc == 1) t[0] = A.Tocnfrz;
        else if ((A.nilyr > 0 && A.nt_qice == 1) || (A.nslyr > 0 && A.nt_qsno == 1)) t[0] = c0;
        for (int it = 1; it < A.ntrcr; it++) t[(size_t)it * nn] = (A.tr_brine && it + 1 == A.nt_fbri) ? c1 : c0;
        if (A.first_ice) A.first_ice[((size_t)b * ncat + (n - 1)) * nn + o] = 1;
    }
    // II (:2022-2164)
    if (aice > c1 + puny) { atomicMin(key, itd_key(b, 2 * ncat + 1, 0, (unsigned)o)); return; }
    if (aice > c1 && aice < c1 + puny) {
        zapped = true;
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            const double *t = t0 + (size_t)(n - 1) * cs;
            double x;
            if (A.tr_pond_topo) {
                x = a[n] * t[(size_t)(A.nt_apnd - 1) * nn] * t[(size_t)(A.nt_hpnd - 1) * nn] * (aice - c1) / aice;
                dfpond = dfpond - x;
            }
            for (int k = 0; k < A.nilyr; k++) {
                x = t[(size_t)(A.nt_qice - 1 + k) * nn] * v[n] / (double)A.nilyr * (aice - c1) / aice / dt;
                dfhocn = dfhocn + x;
            }
            for (int k = 0; k < A.nslyr; k++) {
                x = t[(size_t)(A.nt_qsno - 1 + k) * nn] * sn[n] / (double)A.nslyr * (aice - c1) / aice / dt;
                dfhocn = dfhocn + x;
            }
            x = (A.rhoi * v[n] + A.rhos * sn[n]) * (aice - c1) / aice / dt;
            dfresh = dfresh + x;
            x = A.rhoi * v[n] * A.salinity * p001 * (aice - c1) / aice / dt;
            dfsalt = dfsalt + x;
            a[n] = a[n] * (c1 / aice); v[n] = v[n] * (c1 / aice); sn[n] = sn[n] * (c1 / aice);
        }
        dirty = ~0u;
        aice = c1; aice0 = c0;
        A.aice[ci] = aice;
    }
    // zap_snow_temperature (:2341-2413)
    const double rnslyr = (double)A.nslyr;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (!(a[n] > puny)) continue;
        double *t = t0 + (size_t)(n - 1) * cs;
        const double hsn = sn[n] / a[n];
        bool l_zap = false;
        for (int k = 0; k < A.nslyr; k++) {
            double zqsn, Tmax;
            if (hsn > A.hs_min) {
                zqsn = t[(size_t)(A.nt_qsno - 1 + k) * nn];
                Tmax = -zqsn * puny * rnslyr / (A.rhos * A.cp_ice * sn[n]);
            } else {
                zqsn = -A.rhos * A.Lfresh;
                Tmax = puny;
            }
            const double zTsn = (A.Lfresh + zqsn / A.rhos) / A.cp_ice;
            if (zTsn < A.Tmin || zTsn > Tmax) l_zap = true;
        }
        if (!l_zap) continue;
        zapped = true;
        for (int k = 0; k < A.nslyr; k++) {
            const double x = t[(size_t)(A.nt_qsno - 1 + k) * nn] / dt * sn[n] / (double)A.nslyr;
            dfhocn = dfhocn + x;
            t[(size_t)(A.nt_qsno - 1 + k) * nn] = c0;
        }
        const double x = (A.rhos * sn[n]) / dt;
        dfresh = dfresh + x;
        sn[n] = c0;
        dirty |= 1u << (n - 1);
    }
    if (zapped) A.aice0[ci] = aice0;
    if (dirty) {
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            if (!(dirty & (1u << (n - 1)))) continue;
            const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
            A.aicen[bc] = a[n]; A.vicen[bc] = v[n]; A.vsnon[bc] = sn[n];
        }
    }
    if (zapped) {                                           // :1741-1748 (adding the zero of a cell that zaps nothing changes nothing)
        if (A.fpond) A.fpond[ci] = A.fpond[ci] + dfpond;
        if (A.fresh) A.fresh[ci] = A.fresh[ci] + dfresh;
        if (A.fsalt) A.fsalt[ci] = A.fsalt[ci] + dfsalt;
        if (A.fhocn) A.fhocn[ci] = A.fhocn[ci] + dfhocn;
    }
}
template __global__ void __launch_bounds__(64) k_itd_zap<0>(Slab, const BlockDesc *, ItdArgs, const unsigned *, unsigned long long *);
template __global__ void __launch_bounds__(64) k_itd_zap<5>(Slab, const BlockDesc *, ItdArgs, const unsigned *, unsigned long long *);

// aggregate (:246-458) on every cell of every block, then the tendencies of step_dynamics on the physical cells
template <int NC>
__global__ void __launch_bounds__(64) k_itd_aggregate(Slab s, const BlockDesc *bd, ItdArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    const double c0 = 0.0, c1 = 1.0;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const BlockDesc d = bd[b];
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const size_t cs = (size_t)A.ntrcr_dim * nn;
    const int si = d.iglob_lo + (i - d.ilo) - s.i0 + 1, sj = d.jglob_lo + (j - d.jlo) - s.j0 + 1;
    const bool inslab = si >= 0 && si <= s.nxl + 1 && sj >= 0 && sj <= s.nyl + 1;
    const bool tm = inslab && s.tmask[mcell(s, si, sj)] != 0;
    double *tr = A.trcr + (size_t)b * cs + o;
    double aice = c0, vice = c0, vsno = c0, aice0 = c1;
    if (tm) {
        const double *t0 = A.trcrn + (size_t)b * ncat * cs + o;
        double a[NA + 1], v[NA + 1], sn[NA + 1], P[3][NA + 1], newP[3] = {c0, c0, c0};
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
            a[n] = A.aicen[bc]; v[n] = A.vicen[bc]; sn[n] = A.vsnon[bc];
            aice = aice + a[n]; vice = vice + v[n]; vsno = vsno + sn[n];
            const double *t = t0 + (size_t)(n - 1) * cs;
            P[0][n] = A.nt_alvl ? t[(size_t)(A.nt_alvl - 1) * nn] : c0;
            P[1][n] = A.nt_apnd ? t[(size_t)(A.nt_apnd - 1) * nn] : c0;
            P[2][n] = A.nt_fbri ? t[(size_t)(A.nt_fbri - 1) * nn] : c0;
        }
        aice0 = fmax(c1 - aice, c0);
        for (int it = 0; it < A.ntrcr; it++) {
            const int acc = A.acc[it], d1 = A.d1[it], d2 = A.d2[it], sl = A.slot[it];
            double atr = c0;
            _Pragma("unroll")
            for (int n = 1; n <= ncat; n++) {                                                               // :356-431: the tracer first
                const double t = t0[(size_t)(n - 1) * cs + (size_t)it * nn];
                double p;
                switch (acc) {
                case 0: p = t * a[n]; break;
                case 1: p = t * v[n]; break;
                case 2: p = t * sn[n]; break;
                case 3: p = t * P[0][n] * a[n]; break;
                case 4: p = t * P[1][n] * a[n]; break;
                case 5: p = t * P[1][n] * P[0][n] * a[n]; break;
                case 6: p = t * P[2][n] * v[n]; break;
                default: p = c0;
                }
                if (acc >= 0) atr = atr + p;
            }
            const double p1 = d1 == 1 ? newP[0] : d1 == 2 ? newP[1] : d1 == 3 ? newP[2] : c0;
            const double p2 = d2 == 1 ? newP[0] : d2 == 2 ? newP[1] : d2 == 3 ? newP[2] : c0;
            const double r = compute_tracer(A.rule[it], atr, aice, vice, vsno, p1, p2, it + 1 == A.nt_fbri, A.Tocnfrz);
            if (sl == 1) newP[0] = r;
            else if (sl == 2) newP[1] = r;
            else if (sl == 3) newP[2] = r;
            tr[(size_t)it * nn] = r;
        }
    } else {
        for (int it = 0; it < A.ntrcr; it++) tr[(size_t)it * nn] = c0;                                      // trcrn(:,:,:) = c0 (:1401)
    }
    A.aice[ci] = aice; A.vice[ci] = vice; A.vsno[ci] = vsno; A.aice0[ci] = aice0;
    if (i >= d.ilo && i <= d.ihi && j >= d.jlo && j <= d.jhi) {                                             // ice_step_mod.F90:1183-1189
        if (A.dvidtd) A.dvidtd[ci] = (vice - A.dvidtd[ci]) / A.dt;
        if (A.daidtd) A.daidtd[ci] = (aice - A.daidtd[ci]) / A.dt;
        if (A.dagedtd && A.nt_iage > 0) A.dagedtd[ci] = (tr[(size_t)(A.nt_iage - 1) * nn] - A.dagedtd[ci]) / A.dt;
    }
}
template __global__ void __launch_bounds__(64) k_itd_aggregate<0>(Slab, const BlockDesc *, ItdArgs);
template __global__ void __launch_bounds__(64) k_itd_aggregate<5>(Slab, const BlockDesc *, ItdArgs);

// ---- bound_state (ice_state.F90:173-238) in one launch, block array to block array ----
// What k_gather_fs -> halo(centre, scalar, fill 0) -> k_scatter_halo leave in the caller's aicen, trcrn(1:ntrcr), vicen, vsnon, without
// the slab in between.  Only the non-physical cells of a block can change, and of those only the ring around the physical cells and the
// outermost row / column of the array: a thread takes one such cell of one block, classifies it once -- keep, fill, or copy from a
// physical cell of another (or the same) block, found through the E-W wrap resp. the fold onto row ny_global and the block table -- and
// then moves a group of BS_PG planes, loads ahead of stores.
// In place in a single launch: a source is always a PHYSICAL cell and a destination never is, so no thread reads what another writes.
// One rank only (the slab is the whole domain, global index = slab index); blocks are uniform (create_blocks), which the host verifies.
constexpr int BS_PG = 8;            // planes per thread: 75 planes of a 5 x 12 state make 10 groups
constexpr int BS_TX = 128;
struct BsArr { double *base; size_t bstride; };          // blocks `bstride` doubles apart
struct BsArgs {
    BsArr aicen, trcrn, vicen, vsnon;                    // planes per block: ncat, ncat * ntrcr_dim, ncat, ncat
    int ncat, ntrcr, ntrcr_dim, nxb, nyb, nplanes;       // nplanes = ncat * (3 + ntrcr)
    int nxg, nyg, bsx, bsy, nbx;                         // bmap[((gj - 1) / bsy) * nbx + (gi - 1) / bsx]: the block of a global cell, -1 eliminated
    int cyclic, tripole;
};

__global__ void __launch_bounds__(BS_TX) k_bound_state(const BlockDesc *bd, const int *bmap, BsArgs A) {
    const int t = blockIdx.x * BS_TX + threadIdx.x, b = blockIdx.y;
    const int nxb = A.nxb, nyb = A.nyb;
    const BlockDesc d = bd[b];
    // the candidate cells: four rows (array bottom, array top, above and below the physical cells) over all columns, then four columns
    // over the rows those four have not taken; a row / column that coincides with the array's edge is listed once
    int i, j;
    if (t < 4 * nxb) {
        const int r = t / nxb;
        i = t - r * nxb + 1;
        j = r == 0 ? 1 : r == 1 ? nyb : r == 2 ? d.jhi + 1 : d.jlo - 1;
        if (r >= 2 && (j <= 1 || j >= nyb)) return;
    } else {
        const int u = t - 4 * nxb;
        if (u >= 4 * nyb) return;
        const int r = u / nyb;
        j = u - r * nyb + 1;
        i = r == 0 ? 1 : r == 1 ? nxb : r == 2 ? d.ihi + 1 : d.ilo - 1;
        if (r >= 2 && (i <= 1 || i >= nxb)) return;
        if (j == 1 || j == nyb || j == d.jhi + 1 || j == d.jlo - 1) return;
    }
    if (i >= d.ilo && i <= d.ihi && j >= d.jlo && j <= d.jhi) return;          // physical cells are never written
    // k_scatter_halo's classification (top_row_too = 0, stress = 0)
    const bool edge = (i == 1 || i == nxb || j == 1 || j == nyb);
    const bool padding = (i > d.ihi + 1 || j > d.jhi + 1);
    const int gi = d.iglob_lo + (i - d.ilo), gj = d.jglob_lo + (j - d.jlo);
    const bool has_src = !padding && ((gi >= 1 && gi <= A.nxg) || A.cyclic) && ((gj >= 1 && gj <= A.nyg) || (A.tripole && gj == A.nyg + 1));
    if (!has_src && !edge) return;                                              // keeps the caller's value
    const size_t nn = (size_t)nyb * nxb;
    const size_t dcell = (size_t)(j - 1) * nxb + (i - 1);
    int sb = -1;
    size_t scell = 0;
    if (has_src) {
        int si = gi, sj = gj;
        if (si < 1) si += A.nxg;
        if (si > A.nxg) si -= A.nxg;
        if (sj == A.nyg + 1) { si = A.nxg - si + 1; sj = A.nyg; }              // centre fold: ghost(g, ny + 1) = top(nx - g + 1, ny)
        sb = bmap[((sj - 1) / A.bsy) * A.nbx + (si - 1) / A.bsx];
        if (sb >= 0) {
            const BlockDesc e = bd[sb];
            scell = (size_t)(e.jlo + (sj - e.jglob_lo) - 1) * nxb + (e.ilo + (si - e.iglob_lo) - 1);
        }
    }
    const int p0 = blockIdx.z * BS_PG;
    const int c1 = A.ncat, c2 = c1 + A.ncat * A.ntrcr, c3 = c2 + A.ncat;
    double v[BS_PG];
    double *dst[BS_PG];
#pragma unroll
    for (int q = 0; q < BS_PG; q++) {
        const int p = p0 + q;
        v[q] = 0.0; dst[q] = nullptr;
        if (p < A.nplanes) {
            const BsArr a = p < c1 ? A.aicen : p < c2 ? A.trcrn : p < c3 ? A.vicen : A.vsnon;
            int pp;
            if (p < c1) pp = p;
            else if (p < c2) { const int r = p - c1, n = r / A.ntrcr; pp = n * A.ntrcr_dim + (r - n * A.ntrcr); }
            else pp = p < c3 ? p - c2 : p - c3;
            dst[q] = a.base + (size_t)b * a.bstride + (size_t)pp * nn + dcell;
            if (sb >= 0) v[q] = a.base[(size_t)sb * a.bstride + (size_t)pp * nn + scell];
        }
    }
#pragma unroll
    for (int q = 0; q < BS_PG; q++) if (dst[q]) *dst[q] = v[q];
}

// ---- bound_state across x-slab ranks in one exchange round ----
// The same fact carries further: the source of every ghost cell is a PHYSICAL cell of some rank, so every rank packs physical cells
// only, the messages cross once, and every rank then fills all its ghost cells in one launch -- no N-S-then-E-W ordering.
// A rank's message to a partner, for the `np` planes of a round (plane list of k_bound_state):
//     [ W: np x nyg, its westmost physical column, rows 1 .. ny_global ]      if the partner is its west neighbour
//     [ E: np x nyg, its eastmost physical column ]                            if the partner is its east neighbour
//     [ T: np x nxl, its top physical row (ny_global) over its own columns ]   if the partner is a tripole fold partner
// (two ranks on a cyclic ring: one message holds W and E).  A cell of an eliminated land block packs 0: the sender knows its block table,
// the receiver does not need it.  The block table bmap covers the GLOBAL block columns; "not mine" is told from "eliminated" by the
// rank's own column range i0 .. i1.
constexpr int BR_MAXT = 5;          // fold partners (evpk_connect refuses more)
struct BrArgs {
    int i0, i1;                     // the rank's global columns
    int p0, np;                     // the planes of this round
    // pack: where the sections go (the neighbour's mapped slot, or a local send buffer); null: no such partner
    double *toW, *toE;
    double *toT[BR_MAXT];
    int nT;
    // fill: the west neighbour's E section, the east neighbour's W section, the fold partners' T sections with their columns
    const double *fromW, *fromE;
    const double *fromT[BR_MAXT];
    int t_i0[BR_MAXT], t_w[BR_MAXT];
    int nS;
};

// plane p of the list aicen(1:ncat), trcrn(1:ntrcr, 1:ncat), vicen, vsnon: its array and its plane inside a block of that array
__device__ inline BsArr bs_plane(const BsArgs &A, int p, int &pp) {
    const int c1 = A.ncat, c2 = c1 + A.ncat * A.ntrcr, c3 = c2 + A.ncat;
    if (p < c1) { pp = p; return A.aicen; }
    if (p < c2) { const int r = p - c1, n = r / A.ntrcr; pp = n * A.ntrcr_dim + (r - n * A.ntrcr); return A.trcrn; }
    if (p < c3) { pp = p - c2; return A.vicen; }
    pp = p - c3;
    return A.vsnon;
}

// blockIdx.y: 0 the W section, 1 the E section, 2 the T sections; a thread takes one physical cell and a group of BS_PG planes, loads
// ahead of stores (the column sections read one cell per block row; the stores of every section are consecutive along the message)
__global__ void __launch_bounds__(BS_TX) k_bound_pack(const BlockDesc *bd, const int *bmap, BsArgs A, BrArgs R) {
    const int t = blockIdx.x * BS_TX + threadIdx.x, sec = blockIdx.y;
    const int nxl = R.i1 - R.i0 + 1;
    int si, sj;
    if (sec < 2) {
        if ((sec == 0 ? R.toW : R.toE) == nullptr || t >= A.nyg) return;
        si = sec == 0 ? R.i0 : R.i1; sj = t + 1;
    } else {
        if (R.nT == 0 || t >= nxl) return;
        si = R.i0 + t; sj = A.nyg;
    }
    const int sb = bmap[((sj - 1) / A.bsy) * A.nbx + (si - 1) / A.bsx];
    const size_t nn = (size_t)A.nyb * A.nxb;
    size_t scell = 0;
    if (sb >= 0) {
        const BlockDesc e = bd[sb];
        scell = (size_t)(e.jlo + (sj - e.jglob_lo) - 1) * A.nxb + (e.ilo + (si - e.iglob_lo) - 1);
    }
    const int q0 = blockIdx.z * BS_PG;
    double v[BS_PG];
#pragma unroll
    for (int q = 0; q < BS_PG; q++) {
        v[q] = 0.0;
        if (q0 + q < R.np && sb >= 0) {
            int pp;
            const BsArr a = bs_plane(A, R.p0 + q0 + q, pp);
            v[q] = a.base[(size_t)sb * a.bstride + (size_t)pp * nn + scell];
        }
    }
    if (sec < 2) {
        double *to = sec == 0 ? R.toW : R.toE;
#pragma unroll
        for (int q = 0; q < BS_PG; q++) if (q0 + q < R.np) to[(size_t)(q0 + q) * A.nyg + t] = v[q];
    } else {
        for (int k = 0; k < R.nT; k++) {
            double *to = R.toT[k];
#pragma unroll
            for (int q = 0; q < BS_PG; q++) if (q0 + q < R.np) to[(size_t)(q0 + q) * nxl + t] = v[q];
        }
    }
}

// k_bound_state's classification per ghost cell on a slab that starts at i0 > 1: keep, fill, copy from a physical cell of the rank's own
// blocks, or take the value a partner packed
__global__ void __launch_bounds__(BS_TX) k_bound_fill(const BlockDesc *bd, const int *bmap, BsArgs A, BrArgs R) {
    const int t = blockIdx.x * BS_TX + threadIdx.x, b = blockIdx.y;
    const int nxb = A.nxb, nyb = A.nyb;
    const BlockDesc d = bd[b];
    int i, j;
    if (t < 4 * nxb) {
        const int r = t / nxb;
        i = t - r * nxb + 1;
        j = r == 0 ? 1 : r == 1 ? nyb : r == 2 ? d.jhi + 1 : d.jlo - 1;
        if (r >= 2 && (j <= 1 || j >= nyb)) return;
    } else {
        const int u = t - 4 * nxb;
        if (u >= 4 * nyb) return;
        const int r = u / nyb;
        j = u - r * nyb + 1;
        i = r == 0 ? 1 : r == 1 ? nxb : r == 2 ? d.ihi + 1 : d.ilo - 1;
        if (r >= 2 && (i <= 1 || i >= nxb)) return;
        if (j == 1 || j == nyb || j == d.jhi + 1 || j == d.jlo - 1) return;
    }
    if (i >= d.ilo && i <= d.ihi && j >= d.jlo && j <= d.jhi) return;          // physical cells are never written
    const bool edge = (i == 1 || i == nxb || j == 1 || j == nyb);
    const bool padding = (i > d.ihi + 1 || j > d.jhi + 1);
    const int gi = d.iglob_lo + (i - d.ilo), gj = d.jglob_lo + (j - d.jlo);
    const bool has_src = !padding && ((gi >= 1 && gi <= A.nxg) || A.cyclic) && ((gj >= 1 && gj <= A.nyg) || (A.tripole && gj == A.nyg + 1));
    if (!has_src && !edge) return;                                              // keeps the caller's value
    const size_t nn = (size_t)nyb * nxb;
    const size_t dcell = (size_t)(j - 1) * nxb + (i - 1);
    int sb = -1;                    // own block of the source, -1: none
    size_t scell = 0;
    const double *msg = nullptr;    // or the source's place in a received section (plane 0 of the round), planes mstride apart
    size_t mstride = 0;
    if (has_src) {
        int si = gi, sj = gj;
        if (si < 1) si += A.nxg;
        if (si > A.nxg) si -= A.nxg;
        const bool folded = sj == A.nyg + 1;
        if (folded) { si = A.nxg - si + 1; sj = A.nyg; }                        // centre fold: ghost(g, ny + 1) = top(nx - g + 1, ny)
        if (folded ? (si >= R.i0 && si <= R.i1) : (gi >= R.i0 && gi <= R.i1)) {
            sb = bmap[((sj - 1) / A.bsy) * A.nbx + (si - 1) / A.bsx];
            if (sb >= 0) {
                const BlockDesc e = bd[sb];
                scell = (size_t)(e.jlo + (sj - e.jglob_lo) - 1) * nxb + (e.ilo + (si - e.iglob_lo) - 1);
            }
        } else if (!folded) {
            const double *from = gi < R.i0 ? R.fromW : R.fromE;
            if (from) { msg = from + (sj - 1); mstride = (size_t)A.nyg; }
        } else {
            for (int k = 0; k < R.nS; k++)
                if (si >= R.t_i0[k] && si < R.t_i0[k] + R.t_w[k]) { msg = R.fromT[k] + (si - R.t_i0[k]); mstride = (size_t)R.t_w[k]; }
        }
    }
    const int q0 = blockIdx.z * BS_PG;
    double v[BS_PG];
    double *dst[BS_PG];
#pragma unroll
    for (int q = 0; q < BS_PG; q++) {
        v[q] = 0.0; dst[q] = nullptr;
        if (q0 + q < R.np) {
            int pp;
            const BsArr a = bs_plane(A, R.p0 + q0 + q, pp);
            dst[q] = a.base + (size_t)b * a.bstride + (size_t)pp * nn + dcell;
            if (sb >= 0) v[q] = a.base[(size_t)sb * a.bstride + (size_t)pp * nn + scell];
            else if (msg) v[q] = msg[(size_t)(q0 + q) * mstride];
        }
    }
#pragma unroll
    for (int q = 0; q < BS_PG; q++) if (dst[q]) *dst[q] = v[q];
}

// ---- linear_itd (source/ice_therm_itd.F90:69-859 with fit_line :871-958) as step_therm2 calls it (ice_step_mod.F90:821-871) ----
// Two launches, no host synchronisation between them:
//   k_litd_scan   every cell: aggregate_area (aice, aice0); a physical ocean cell with aice > puny is listed and sets its block's flag
//   k_litd_remap  physical ocean cells of the flagged blocks: an unlisted cell zeroes its tracers (compute_tracers, ice_itd.F90:1401); a
//                 listed cell computes hbnew, remap_flag, fit_line, the category-1 melt, donor / daice / dvice of every boundary, then
//                 shift_ice with all ncat - 1 boundaries at once and compute_tracers, the hi_min clamp and aggregate_area
// A boundary's donor is the category below or above it, known at run time only: it is kept as a direction (LITD_UP / LITD_DOWN) and every
// access is a select between the two neighbours of an unrolled loop, never an index into a per-thread array.
// The stop key is cleanup_itd's: block | boundary n | shift_ice's check 0 .. 3 | cell counting down (the error loops do not exit).
struct LitdArgs {
    const double *aicen_init, *vicen_init;                      // (nb, ncat, ny, nx)
    double hi_min;
};
enum { LITD_NONE = 0, LITD_UP = 1, LITD_DOWN = 2 };             // donor(n) = 0, n, n + 1

template <int NC>
__global__ void __launch_bounds__(64) k_litd_scan(Slab s, const BlockDesc *bd, ItdArgs A, unsigned *bflag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    const double c0 = 0.0, c1 = 1.0;
    const int ncat = NC ? NC : A.ncat;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    double aice = c0;                                                                                       // aggregate_area (ice_itd.F90:489-506)
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) aice = aice + A.aicen[((size_t)b * ncat + (n - 1)) * nn + o];
    A.aice[ci] = aice;
    A.aice0[ci] = fmax(c1 - aice, c0);
    // ice_step_mod.F90:830-839; the flag only ever goes from 0 to 1, so a cell that sees it set has nothing to add
    if (itd_ocean(s, bd[b], i, j) && aice > A.puny && __atomic_load_n(&bflag[b], __ATOMIC_RELAXED) == 0u) atomicOr(&bflag[b], 1u);
}
template __global__ void __launch_bounds__(64) k_litd_scan<0>(Slab, const BlockDesc *, ItdArgs, unsigned *);
template __global__ void __launch_bounds__(64) k_litd_scan<5>(Slab, const BlockDesc *, ItdArgs, unsigned *);

// (min / max as a comparison and a select: no NaN rule to differ on)
__device__ __forceinline__ double litd_min(double x, double y) { return y < x ? y : x; }
__device__ __forceinline__ double litd_max(double x, double y) { return y > x ? y : x; }

// fit_line (:917-956) of one cell and category
__device__ __forceinline__ void litd_fit_line(double a, double hice, double hbL, double hbR, double puny, double &g0, double &g1, double &hL, double &hR) {
    const double c0 = 0.0, c1 = 1.0, c2 = 2.0, c3 = 3.0, c6 = 6.0, p5 = 0.5, p333 = c1 / c3, p666 = c2 / c3;
    if (a > puny && hbR - hbL > puny) {
        hL = hbL; hR = hbR;
        const double h13 = p333 * (c2 * hL + hR), h23 = p333 * (hL + c2 * hR);
        if (hice < h13) hR = c3 * hice - c2 * hL;
        else if (hice > h23) hL = c3 * hice - c2 * hR;
        const double dhr = c1 / (hR - hL), wk1 = c6 * a * dhr, wk2 = (hice - hL) * dhr;
        g0 = wk1 * (p666 - wk2);
        g1 = c2 * dhr * wk1 * (wk2 - p5);
    } else {
        g0 = c0; g1 = c0; hL = c0; hR = c0;
    }
}

// shift_ice's tracer part for all boundaries of one call (ice_itd.F90:919-975, :1175-1214, :1234-1239), the extension of
// itd_shift_tracers: atrcrn once from the old state, the transfers of boundaries 1 .. ncat - 1 in order, each with the donor's untouched
// trcrn, compute_tracers once.  qoff != 0: the snow enthalpies carry + rhos * Lfresh through the call (ice_therm_itd.F90:659-690).
// apnd1 / hpnd1: the new pond tracers of category 1, for the hi_min clamp.
template <int NC>
__device__ __forceinline__ void litd_shift_tracers(const ItdArgs &A, int ncat, double *t0, size_t nn, const double *ao, const double *vo,
                                                   const double *so, const double *an, const double *vn, const double *sn, const int *dn,
                                                   const double *dA, const double *dV, const double *dS, double qoff, double &apnd1,
                                                   double &hpnd1) {
    constexpr int NA = NC ? NC : MAXCAT;
    double oldP[3][NA + 2], newP[3][NA + 2];
    const size_t cs = (size_t)A.ntrcr_dim * nn;                 // category stride
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const double *t = t0 + (size_t)(n - 1) * cs;
        oldP[0][n] = A.nt_alvl ? t[(size_t)(A.nt_alvl - 1) * nn] : 0.0;
        oldP[1][n] = A.nt_apnd ? t[(size_t)(A.nt_apnd - 1) * nn] : 0.0;
        oldP[2][n] = A.nt_fbri ? t[(size_t)(A.nt_fbri - 1) * nn] : 0.0;
        newP[0][n] = 0.0; newP[1][n] = 0.0; newP[2][n] = 0.0;
    }
    for (int it = 0; it < A.ntrcr; it++) {
        const int acc = A.acc[it], rule = A.rule[it], d1 = A.d1[it], d2 = A.d2[it], sl = A.slot[it];
        const bool qs = qoff != 0.0 && A.nslyr > 0 && it + 1 >= A.nt_qsno && it + 1 < A.nt_qsno + A.nslyr;
        double told[NA + 2], atr[NA + 2];
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            told[n] = t0[(size_t)(n - 1) * cs + (size_t)it * nn];
            if (qs) told[n] = told[n] + qoff;
            atr[n] = itd_product(acc, ao[n], vo[n], so[n], oldP[0][n], oldP[1][n], oldP[2][n], told[n]);
        }
        if (acc >= 0) {
            _Pragma("unroll")
            for (int n = 1; n < ncat; n++) {
                if (dn[n] == LITD_NONE) continue;
                const bool up = dn[n] == LITD_UP;
                const double dat = itd_product(acc, dA[n], dV[n], dS[n], up ? oldP[0][n] : oldP[0][n + 1], up ? oldP[1][n] : oldP[1][n + 1],
                                               up ? oldP[2][n] : oldP[2][n + 1], up ? told[n] : told[n + 1]);
                const double lo = up ? atr[n] - dat : atr[n] + dat, hi = up ? atr[n + 1] + dat : atr[n + 1] - dat;
                atr[n] = lo; atr[n + 1] = hi;
            }
        }
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            const double p1 = d1 == 1 ? newP[0][n] : d1 == 2 ? newP[1][n] : d1 == 3 ? newP[2][n] : 0.0;
            const double p2 = d2 == 1 ? newP[0][n] : d2 == 2 ? newP[1][n] : d2 == 3 ? newP[2][n] : 0.0;
            const double r = compute_tracer(rule, atr[n], an[n], vn[n], sn[n], p1, p2, it + 1 == A.nt_fbri, A.Tocnfrz);
            if (sl == 1) newP[0][n] = r;
            else if (sl == 2) newP[1][n] = r;
            else if (sl == 3) newP[2][n] = r;
            if (n == 1 && it + 1 == A.nt_apnd) apnd1 = r;
            if (n == 1 && it + 1 == A.nt_hpnd) hpnd1 = r;
            t0[(size_t)(n - 1) * cs + (size_t)it * nn] = qs ? r - qoff : r;
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(64) k_litd_remap(Slab s, const BlockDesc *bd, ItdArgs A, LitdArgs L, const unsigned *bflag, unsigned long long *key) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if (!bflag[b]) return;                                // icells = 0: linear_itd is not called for this block
    if (!itd_ocean(s, bd[b], i, j)) return;
    const double puny = A.puny, c0 = 0.0, c1 = 1.0, c2 = 2.0, c3 = 3.0, p5 = 0.5, p333 = c1 / c3;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const size_t cs = (size_t)A.ntrcr_dim * nn;
    double *t0 = A.trcrn + (size_t)b * ncat * cs + o;
    if (!(A.aice[ci] > puny)) {                           // an unlisted cell of a block that calls shift_ice: trcrn(:,:,:) = c0 (ice_itd.F90:1401)
        for (int n = 0; n < ncat; n++)
            for (int it = 0; it < A.ntrcr; it++) t0[(size_t)n * cs + (size_t)it * nn] = c0;
        return;
    }
    double a[NA + 2], v[NA + 2], sn[NA + 2], h[NA + 2], hi0[NA + 2], dh[NA + 2], hb[NA + 2];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {                                                                       // :308-328
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        a[n] = A.aicen[bc]; v[n] = A.vicen[bc]; sn[n] = A.vsnon[bc];
        const double ai = L.aicen_init[bc], vi = L.vicen_init[bc];
        hi0[n] = ai > puny ? vi / ai : c0;
        if (a[n] > puny) { h[n] = v[n] / a[n]; dh[n] = h[n] - hi0[n]; }
        else { h[n] = c0; dh[n] = c0; }
    }
    bool remap = true;
    hb[0] = A.hin_max[0];
    _Pragma("unroll")
    for (int n = 1; n < ncat; n++) {                                                                        // :339-436
        const double hn = A.hin_max[n];
        if (hi0[n] > puny && hi0[n + 1] > puny) {
            const double slope = (dh[n + 1] - dh[n]) / (hi0[n + 1] - hi0[n]);
            hb[n] = hn + dh[n] + slope * (hn - hi0[n]);
        } else if (hi0[n] > puny) hb[n] = hn + dh[n];
        else if (hi0[n + 1] > puny) hb[n] = hn + dh[n + 1];
        else hb[n] = hn;
        if (a[n] > puny && h[n] >= hb[n]) remap = false;
        else if (a[n + 1] > puny && h[n + 1] <= hb[n]) remap = false;
        if (hb[n] > A.hin_max[n + 1]) remap = false;
        if (hb[n] < A.hin_max[n - 1]) remap = false;
    }
    hb[ncat] = a[ncat] > puny ? c3 * h[ncat] - c2 * hb[ncat - 1] : A.hin_max[ncat];                         // :445-454
    hb[ncat] = litd_max(hb[ncat], A.hin_max[ncat - 1]);

    int dn[NA + 2];
    double dA[NA + 2], dV[NA + 2], dS[NA + 2];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) { dn[n] = LITD_NONE; dA[n] = c0; dV[n] = c0; dS[n] = c0; }
    const bool topo = A.tr_pond_topo != 0;
    double fp = topo ? A.fpond[ci] : c0;
    if (remap) {
        double g0[NA + 2], g1[NA + 2], hL[NA + 2], hR[NA + 2];
        litd_fit_line(a[1], hi0[1], hb[0], A.hin_max[1], puny, g0[1], g1[1], hL[1], hR[1]);                 // :482-492
        if (a[1] > puny) {                                                                                  // :501-548
            double dh0 = dh[1];
            if (dh0 < c0) {
                dh0 = litd_min(-dh0, A.hin_max[1]);
                const double etamax = litd_min(dh0, hR[1]) - hL[1];
                if (etamax > c0) {
                    const double x1 = etamax, x2 = p5 * etamax * etamax;
                    double da0 = g1[1] * x2 + g0[1] * x1;
                    const double damax = a[1] * (c1 - h[1] / hi0[1]);
                    da0 = litd_min(da0, damax);
                    h[1] = h[1] * a[1] / (a[1] - da0);
                    a[1] = a[1] - da0;
                    if (topo) fp = fp - (da0 * t0[(size_t)(A.nt_apnd - 1) * nn] * t0[(size_t)(A.nt_hpnd - 1) * nn]);
                }
            } else {
                hb[0] = litd_min(dh0, A.hin_max[1]);
            }
        }
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) litd_fit_line(a[n], h[n], hb[n - 1], hb[n], puny, g0[n], g1[n], hL[n], hR[n]);      // :554-563
        _Pragma("unroll")
        for (int n = 1; n < ncat; n++) {                                                                    // :577-647
            const double hn = A.hin_max[n];
            const bool up = hb[n] > hn;
            const double G0 = up ? g0[n] : g0[n + 1], G1 = up ? g1[n] : g1[n + 1], HL = up ? hL[n] : hL[n + 1], HR = up ? hR[n] : hR[n + 1];
            const double and_ = up ? a[n] : a[n + 1], vnd = up ? v[n] : v[n + 1];
            const double etamin = up ? litd_max(hn, HL) - HL : c0;
            const double etamax = (up ? litd_min(hb[n], HR) : litd_min(hn, HR)) - HL;
            double da = c0, dv = c0;
            int don = up ? LITD_UP : LITD_DOWN;
            if (etamax > etamin) {
                const double x1 = etamax - etamin;
                double wk1 = etamin * etamin, wk2 = etamax * etamax;
                const double x2 = p5 * (wk2 - wk1);
                wk1 = wk1 * etamin; wk2 = wk2 * etamax;
                const double x3 = p333 * (wk2 - wk1);
                da = G1 * x2 + G0 * x1;
                dv = G1 * x3 + G0 * x2 + da * HL;
            }
            if (da < and_ * puny) { da = c0; dv = c0; don = LITD_NONE; }
            if (dv < vnd * puny) { da = c0; dv = c0; don = LITD_NONE; }
            if (da > and_ * (c1 - puny)) { da = and_; dv = vnd; }
            if (dv > vnd * (c1 - puny)) { da = and_; dv = vnd; }
            // (donor = 0 with daice > 0 needs a negative vicen under aicen > puny; the reference then indexes category 0: nothing moves here)
            if (don == LITD_NONE) { da = c0; dv = c0; }
            dn[n] = don; dA[n] = da; dV[n] = dv;
        }
    }
    // shift_ice (ice_itd.F90:815-1250) with every boundary, for every listed cell
    double ao[NA + 2], vo[NA + 2], so[NA + 2];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) { ao[n] = a[n]; vo[n] = v[n]; so[n] = sn[n]; }
    _Pragma("unroll")
    for (int n = 1; n < ncat; n++) {
        if (dn[n] == LITD_NONE) continue;
        const bool up = dn[n] == LITD_UP;
        const double and_ = up ? a[n] : a[n + 1], vnd = up ? v[n] : v[n + 1], snd = up ? sn[n] : sn[n + 1];
        const int bad = itd_check(dA[n], dV[n], and_, vnd, puny);
        if (bad >= 0) { atomicMin(key, itd_key(b, n, bad, 0xffffffffu - (unsigned)o)); return; }           // a stop: the state is undefined
        if (!(dA[n] > c0)) { dn[n] = LITD_NONE; continue; }                                                // :1137
        const double worka = dA[n] / and_;
        const double dvs = snd * worka;
        dS[n] = dvs;
        const double alo = up ? a[n] - dA[n] : a[n] + dA[n], ahi = up ? a[n + 1] + dA[n] : a[n + 1] - dA[n];
        const double vlo = up ? v[n] - dV[n] : v[n] + dV[n], vhi = up ? v[n + 1] + dV[n] : v[n + 1] - dV[n];
        const double slo = up ? sn[n] - dvs : sn[n] + dvs, shi = up ? sn[n + 1] + dvs : sn[n + 1] - dvs;
        a[n] = alo; a[n + 1] = ahi; v[n] = vlo; v[n + 1] = vhi; sn[n] = slo; sn[n + 1] = shi;
    }
    double apnd1 = c0, hpnd1 = c0;
    if (A.ntrcr > 0)
        litd_shift_tracers<NC>(A, ncat, t0, nn, ao, vo, so, a, v, sn, dn, dA, dV, dS, remap ? A.rhos * A.Lfresh : c0, apnd1, hpnd1);
    if (remap) {                                                                                            // :701-718
        const double h1 = a[1] > puny ? v[1] / a[1] : c0;                                                   // (shift_ice's hicen, ice_itd.F90:1227-1231)
        if (L.hi_min > c0 && a[1] > puny && h1 < L.hi_min) {
            const double da0 = a[1] * (c1 - h1 / L.hi_min);
            a[1] = a[1] - da0;
            if (topo) fp = fp - (da0 * apnd1 * hpnd1);
        }
    }
    double aice = c0;                                                                                       // aggregate_area
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        A.aicen[bc] = a[n]; A.vicen[bc] = v[n]; A.vsnon[bc] = sn[n];
        aice = aice + a[n];
    }
    A.aice[ci] = aice;
    A.aice0[ci] = fmax(c1 - aice, c0);
    if (topo) A.fpond[ci] = fp;
}
template __global__ void __launch_bounds__(64) k_litd_remap<0>(Slab, const BlockDesc *, ItdArgs, LitdArgs, const unsigned *, unsigned long long *);
template __global__ void __launch_bounds__(64) k_litd_remap<5>(Slab, const BlockDesc *, ItdArgs, LitdArgs, const unsigned *, unsigned long long *);

}  // namespace evpk
