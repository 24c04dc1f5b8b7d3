// evpk_ridge.hip -- ridge_ice (source/ice_mechred.F90:101-746) on the device: asum_ridging, ridge_prep, ridge_itd, ridge_shift with
// compute_tracers, ridge_check and the diagnostics, on the caller's block arrays as they are.  SURVEY.md S8 row f-5.  Included by
// evpk_api.hip (one translation unit).
//
// One thread per cell of the block arrays; a cell is LISTED if it is a physical cell with tmask (step_ridge's list,
// ice_step_mod.F90:1272-1281).  The reference keeps atrcrn(icells, ntrcr, ncat) live across the n / nr double loop of ridge_shift;
// here a cell's work is split in two kernels per iteration:
//   k_ridge_weights  ridge_prep (first iteration), ridge_itd, closing_gross with its two reductions, the aice0 update, the per-category
//                    weights ardg1n / ardg2n / virdgn / vsrdgn, the per-(n, nr) fractions farea / fvol, the new aicen / vicen / vsnon,
//                    the scalar accumulators, asum_ridging + ridge_check for the next iteration
//   k_ridge_tracers  one tracer at a time: atrcrn(it, 1..ncat) from the old trcrn and the weights in the reference's accumulation
//                    order (n outer, nr inner, :1752-2017), then compute_tracers; the old and the new values of the tracers that
//                    others hang on (alvl, apnd, fbri) stay in registers.  Last, the new aicen / vicen / vsnon are committed.
// What passes from one kernel (and one iteration) to the next is a pool of planes indexed by the block-array cell.
// Iteration is per BLOCK as in the reference (ridge_check's iterate_ridging is one flag per ridge_ice call): flags[k][b] is set by any
// cell of block b that is not converged after iteration k, and every listed cell of b then runs iteration k + 1.
// Same operation order as the Fortran, -ffp-contract=off, exp() = dev_exp: bit-comparable with the CPU restatement.
#pragma once

namespace evpk {

constexpr int RG_MAXT = 32;
constexpr int RG_NITER = 20;                                  // nitermax (:244)
enum { RG_CLOSING = 0, RG_OPNING, RG_MSNOW, RG_ESNOW, RG_MPOND, RG_ARDG1, RG_ARDG2, RG_VIRDG, RG_AOPEN, RG_ASUM, RG_NSCALAR };
// pool planes after the scalars, each group ncat (or ncat * ncat) planes
struct RidgePool {
    double *base;
    unsigned *mask;         // per cell: bit n - 1 = category n ridged in this iteration
    size_t N;               // cells per plane
    int ncat;
    __host__ __device__ double *sc(int q) const { return base + (size_t)q * N; }
    __host__ __device__ double *ardg1n(int n) const { return base + (size_t)(RG_NSCALAR + n) * N; }                 // n 0-based
    __host__ __device__ double *ardg2n(int n) const { return base + (size_t)(RG_NSCALAR + ncat + n) * N; }
    __host__ __device__ double *virdgn(int n) const { return base + (size_t)(RG_NSCALAR + 2 * ncat + n) * N; }
    __host__ __device__ double *mraftn(int n) const { return base + (size_t)(RG_NSCALAR + 3 * ncat + n) * N; }
    __host__ __device__ double *vsrdgn(int n) const { return base + (size_t)(RG_NSCALAR + 4 * ncat + n) * N; }
    __host__ __device__ double *anew(int q, int n) const { return base + (size_t)(RG_NSCALAR + (5 + q) * ncat + n) * N; }   // q 0 a, 1 v, 2 s
    __host__ __device__ double *farea(int n, int nr) const { return base + (size_t)(RG_NSCALAR + 8 * ncat + n * ncat + nr) * N; }
    __host__ __device__ double *fvol(int n, int nr) const { return base + (size_t)(RG_NSCALAR + 8 * ncat + (ncat + n) * ncat + nr) * N; }
    static size_t planes(int ncat) { return (size_t)RG_NSCALAR + 8 * (size_t)ncat + 2 * (size_t)ncat * ncat; }
};

// control words: the smallest key of a cell that met one of the reference's l_stop conditions, and the per-iteration flags
struct RidgeCtl {
    unsigned long long key;            // ~0: none
    int any[RG_NITER + 1];             // any[k]: some block repeats after iteration k
};
enum { RG_STOP_AICE0 = 1, RG_STOP_ARDG = 2, RG_STOP_NITER = 3, RG_STOP_ASUM = 4 };
// (block, kind, category, cell of the block) in the order the reference would meet them inside one ridge_shift: the aice0 loop over
// the cells, then n outer / cells inner
__device__ __forceinline__ unsigned long long ridge_key(int b, int kind, int n, size_t o) {
    return ((unsigned long long)b << 44) | ((unsigned long long)kind << 40) | ((unsigned long long)n << 32) | (unsigned long long)o;
}

struct RidgeArgs {
    double *aice0, *aicen, *vicen, *vsnon, *trcrn;      // block arrays (nb, ny, nx), (nb, ncat, ny, nx) x 3, (nb, ncat, ntrcr_dim, ny, nx)
    const double *rdg_conv, *rdg_shear;                 // block arrays, or nullptr: planes F_RDGCONV / F_RDGSHEAR of the slab
    double *dardg1dt, *dardg2dt, *dvirdgdt, *opening, *fpond, *fresh, *fhocn;
    double *dardg1ndt, *dardg2ndt, *dvirdgndt, *aparticn, *krdgn, *araftn, *vraftn, *aredistn, *vredistn;
    int ncat, ntrcr, ntrcr_dim, nxb, nyb;
    int nt_qsno, nslyr, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_fbri, tr_pond_topo;
    double dt, dti_thermo;                               // dti_thermo = 1 / (ndtd * dt)  (:691)
    double hin_max[MAXCAT + 1];                          // hin_max(0:ncat), hin_max(ncat) = 1e8 (ridge_prep, :864)
    // per tracer (0-based): acc: how atrcrn is built and moved (0 area, 1 ice volume, 2 snow volume, 3 aicen * alvl, 4 aicen * apnd,
    // 5 aicen * alvl * apnd, 6 vicen * fbri, -1: no rule); rule, d1, d2: compute_tracer's rule and the parent SLOTS + 1 (slot 0 alvl,
    // 1 apnd, 2 fbri; 0 = none); slot: the slot this tracer fills + 1
    signed char acc[RG_MAXT], rule[RG_MAXT], d1[RG_MAXT], d2[RG_MAXT], slot[RG_MAXT];
};

__device__ __forceinline__ bool ridge_listed(const Slab &s, const BlockDesc &d, int i, int j, int &si, int &sj) {
    if (i < d.ilo || i > d.ihi || j < d.jlo || j > d.jhi) return false;
    si = d.iglob_lo + (i - d.ilo) - s.i0 + 1;
    sj = d.jglob_lo + (j - d.jlo) - s.j0 + 1;
    if (si < 1 || si > s.nxl || sj < 1 || sj > s.nyl) return false;
    return s.tmask[mcell(s, si, sj)] != 0;
}

// iter: 1-based.  flags: (RG_NITER + 1) rows of nblocks ints, row k = "block repeats after iteration k"
// (64 threads per block: the register budget of a wave is then the whole file, and the NC = 5 arrays stay out of scratch memory)
template <int NC>
__global__ void __launch_bounds__(64) k_ridge_weights(Slab s, DevParams p, const BlockDesc *bd, RidgeArgs A, RidgePool P, int iter, int *flags, int nblocks,
                                RidgeCtl *ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if (iter > 1 && !flags[(size_t)(iter - 1) * nblocks + b]) return;
    int si, sj;
    if (!ridge_listed(s, bd[b], i, j, si, sj)) return;
    const double puny = 1.0e-11, c0 = 0.0, c1 = 1.0, Cs = 0.25, fsnowrdg = 0.5;                              // :66-69
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const double dt = A.dt;
    double an[NA + 1], vn[NA + 1], sn[NA + 1], ai[NA + 1], vi[NA + 1], sni[NA + 1];
    double a0 = A.aice0[ci];
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        an[n] = A.aicen[bc]; vn[n] = A.vicen[bc]; sn[n] = A.vsnon[bc];
    }
    double closing_net, opning, msnow_mlt = c0, esnow_mlt = c0, mpond = c0, ardg1 = c0, ardg2 = c0, virdg = c0;
    double mraft[NA + 1];
    if (iter == 1) {
        double asum = a0;                                                                                   // asum_ridging (:791-810)
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) asum = asum + an[n];
        double conv, shear;
        if (A.rdg_conv) { conv = A.rdg_conv[ci]; shear = A.rdg_shear[ci]; }
        else { const size_t k = cell(s, si, sj); conv = FD(s, F_RDGCONV, k); shear = FD(s, F_RDGSHEAR, k); }
        closing_net = Cs * shear + conv;                                                                    // ridge_prep (:893-913)
        const double divu_adv = (c1 - asum) / dt;
        if (divu_adv < c0) closing_net = fmax(closing_net, -divu_adv);
        opning = closing_net + divu_adv;
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) {
            mraft[n] = c0;
            P.ardg1n(n - 1)[ci] = c0; P.ardg2n(n - 1)[ci] = c0; P.virdgn(n - 1)[ci] = c0;                   // (:278-281)
        }
    } else {
        closing_net = P.sc(RG_CLOSING)[ci]; opning = P.sc(RG_OPNING)[ci];
        msnow_mlt = P.sc(RG_MSNOW)[ci]; esnow_mlt = P.sc(RG_ESNOW)[ci]; mpond = P.sc(RG_MPOND)[ci];
        ardg1 = P.sc(RG_ARDG1)[ci]; ardg2 = P.sc(RG_ARDG2)[ci]; virdg = P.sc(RG_VIRDG)[ci];
        _Pragma("unroll")
        for (int n = 1; n <= ncat; n++) mraft[n] = P.mraftn(n - 1)[ci];
    }
    double apartic[NA + 1], hrmin[NA + 1], hrmax[NA + 1], hrexp[NA + 1], krdg[NA + 1];
    const double aksum = ridge_itd<NC, true>(p, ncat, a0, [&](int n) { return an[n]; }, [&](int n) { return vn[n]; }, apartic, hrmin, hrmax,
                                             hrexp, krdg, mraft);
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t bc = ((size_t)b * ncat + (n - 1)) * nn + o;
        if (A.aparticn) A.aparticn[bc] = apartic[n];
        if (A.krdgn) A.krdgn[bc] = krdg[n];
        P.mraftn(n - 1)[ci] = mraft[n];
    }
    // ridge_shift: closing_gross and its reductions (:1528-1568)
    double closing_gross = closing_net / aksum;
    if (apartic[0] > c0) {
        const double wk1 = apartic[0] * closing_gross * dt;
        if (wk1 > a0) {
            const double tmpfac = a0 / wk1;
            closing_gross = closing_gross * tmpfac;
            opning = opning * tmpfac;
        }
    }
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (an[n] > puny && apartic[n] > c0) {
            const double wk1 = apartic[n] * closing_gross * dt;
            if (wk1 > an[n]) {
                const double tmpfac = an[n] / wk1;
                closing_gross = closing_gross * tmpfac;
                opning = opning * tmpfac;
            }
        }
    }
    a0 = a0 - apartic[0] * closing_gross * dt + opning * dt;                                                // :1580-1582
    if (a0 < -puny) atomicMin(&ctl->key, ridge_key(b, 0, 0, o));                                            // :1583 (the state is undefined from here)
    else if (a0 < c0) a0 = c0;
    const double aopen = opning * dt;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) { ai[n] = an[n]; vi[n] = vn[n]; sni[n] = sn[n]; }                       // :1605-1613
    unsigned mask = 0;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        if (!(ai[n] > puny && apartic[n] > c0 && closing_gross > c0)) continue;                             // :1631-1632
        mask |= 1u << (n - 1);
        double ardg1n = apartic[n] * closing_gross * dt;                                                    // :1654
        if (ardg1n > ai[n] + puny) atomicMin(&ctl->key, ridge_key(b, 1, n, o));                             // :1656
        else ardg1n = fmin(ai[n], ardg1n);
        const double ardg2n = ardg1n / krdg[n];
        const double afrac = ardg1n / ai[n];
        const double virdgn = vi[n] * afrac, vsrdgn = sni[n] * afrac;
        an[n] = an[n] - ardg1n; vn[n] = vn[n] - virdgn; sn[n] = sn[n] - vsrdgn;
        ardg1 = ardg1 + ardg1n; ardg2 = ardg2 + ardg2n; virdg = virdg + virdgn;
        P.ardg1n(n - 1)[ci] = ardg1n; P.ardg2n(n - 1)[ci] = ardg2n; P.virdgn(n - 1)[ci] = virdgn; P.vsrdgn(n - 1)[ci] = vsrdgn;
        msnow_mlt = msnow_mlt + p.rhos * vsrdgn * (c1 - fsnowrdg);                                          // :1702
        const double *t = A.trcrn + ((size_t)b * ncat + (n - 1)) * A.ntrcr_dim * nn + o;
        if (A.tr_pond_topo) mpond = mpond + ardg1n * t[(size_t)(A.nt_apnd - 1) * nn] * t[(size_t)(A.nt_hpnd - 1) * nn];     // :1713-1717
        for (int k = 1; k <= A.nslyr; k++) {                                                                // :1734-1746
            const double esrdgn = vsrdgn * t[(size_t)(A.nt_qsno + k - 2) * nn] / (double)A.nslyr;
            esnow_mlt = esnow_mlt + esrdgn * (c1 - fsnowrdg);
        }
        const double hi1 = hrmin[n], hexp = hrexp[n];
        _Pragma("unroll")
        for (int nr = 1; nr <= ncat; nr++) {                                                                // krdg_redist = 1 (:1881-1917)
            double farea, fvol;
            if (nr < ncat) {
                if (hi1 >= A.hin_max[nr]) { farea = c0; fvol = c0; }
                else {
                    const double hL = fmax(hi1, A.hin_max[nr - 1]), hR = A.hin_max[nr];
                    const double expL = dev_exp(-(hL - hi1) / hexp), expR = dev_exp(-(hR - hi1) / hexp);
                    farea = expL - expR;
                    fvol = ((hL + hexp) * expL - (hR + hexp) * expR) / (hi1 + hexp);
                }
            } else {
                const double hL = fmax(hi1, A.hin_max[nr - 1]);
                const double expL = dev_exp(-(hL - hi1) / hexp);
                farea = expL;
                fvol = (hL + hexp) * expL / (hi1 + hexp);
            }
            if (n == 1) {                                                                                   // :1920-1935
                const size_t bcr = ((size_t)b * ncat + (nr - 1)) * nn + o;
                if (A.aredistn) A.aredistn[bcr] = farea * ardg2n;
                if (A.vredistn) A.vredistn[bcr] = fvol * virdgn;
            }
            an[nr] = an[nr] + farea * ardg2n;                                                               // :1950-1953
            vn[nr] = vn[nr] + fvol * virdgn;
            sn[nr] = sn[nr] + fvol * vsrdgn * fsnowrdg;
            P.farea(n - 1, nr - 1)[ci] = farea;
            P.fvol(n - 1, nr - 1)[ci] = fvol;
        }
    }
    // asum_ridging + ridge_check (:431-441, :2081-2091): the rates of the next iteration
    double asum = a0;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) asum = asum + an[n];
    if (fabs(asum - c1) < puny) { closing_net = c0; opning = c0; }
    else {
        atomicOr(&flags[(size_t)iter * nblocks + b], 1);
        atomicOr(&ctl->any[iter], 1);
        const double divu_adv = (c1 - asum) / dt;
        closing_net = fmax(c0, -divu_adv);
        opning = fmax(c0, divu_adv);
    }
    A.aice0[ci] = a0;
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) { P.anew(0, n - 1)[ci] = an[n]; P.anew(1, n - 1)[ci] = vn[n]; P.anew(2, n - 1)[ci] = sn[n]; }
    P.sc(RG_CLOSING)[ci] = closing_net; P.sc(RG_OPNING)[ci] = opning; P.sc(RG_MSNOW)[ci] = msnow_mlt; P.sc(RG_ESNOW)[ci] = esnow_mlt;
    P.sc(RG_MPOND)[ci] = mpond; P.sc(RG_ARDG1)[ci] = ardg1; P.sc(RG_ARDG2)[ci] = ardg2; P.sc(RG_VIRDG)[ci] = virdg;
    P.sc(RG_AOPEN)[ci] = aopen; P.sc(RG_ASUM)[ci] = asum;
    P.mask[ci] = mask;
}
template __global__ void __launch_bounds__(64) k_ridge_weights<0>(Slab, DevParams, const BlockDesc *, RidgeArgs, RidgePool, int, int *, int, RidgeCtl *);
template __global__ void __launch_bounds__(64) k_ridge_weights<5>(Slab, DevParams, const BlockDesc *, RidgeArgs, RidgePool, int, int *, int, RidgeCtl *);

// the tracers of the cells that k_ridge_weights has just visited, then the new aicen / vicen / vsnon
template <int NC>
__global__ void __launch_bounds__(64) k_ridge_tracers(Slab s, const BlockDesc *bd, RidgeArgs A, RidgePool P, int iter, const int *flags, int nblocks) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    if (iter > 1 && !flags[(size_t)(iter - 1) * nblocks + b]) return;
    int si, sj;
    if (!ridge_listed(s, bd[b], i, j, si, sj)) return;
    const double fsnowrdg = 0.5;
    const int ncat = NC ? NC : A.ncat;
    constexpr int NA = NC ? NC : MAXCAT;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const unsigned mask = P.mask[ci];
    // in registers across the tracers: the per-category weights and the old / new values of the tracers that others hang on; the old
    // and new aicen / vicen / vsnon are read again per tracer (one of the three each) -- they would cost 60 more registers
    double ardg1n[NA], ardg2n[NA], virdgn[NA], vsrdgn[NA];
    double oldP[3][NA], newP[3][NA];
    _Pragma("unroll")
    for (int n = 0; n < ncat; n++) {
        ardg1n[n] = P.ardg1n(n)[ci]; ardg2n[n] = P.ardg2n(n)[ci]; virdgn[n] = P.virdgn(n)[ci]; vsrdgn[n] = P.vsrdgn(n)[ci];
        const double *t = A.trcrn + ((size_t)b * ncat + n) * A.ntrcr_dim * nn + o;
        oldP[0][n] = A.nt_alvl ? t[(size_t)(A.nt_alvl - 1) * nn] : 0.0;
        oldP[1][n] = A.nt_apnd ? t[(size_t)(A.nt_apnd - 1) * nn] : 0.0;
        oldP[2][n] = A.nt_fbri ? t[(size_t)(A.nt_fbri - 1) * nn] : 0.0;
        newP[0][n] = 0.0; newP[1][n] = 0.0; newP[2][n] = 0.0;          // (a parent that comes later in the table is still 0, ice_itd.F90:1401)
    }
    for (int it = 0; it < A.ntrcr; it++) {
        const int acc = A.acc[it];
        double told[NA], atr[NA];
        _Pragma("unroll")
        for (int n = 0; n < ncat; n++) {
            told[n] = A.trcrn[(((size_t)b * ncat + n) * A.ntrcr_dim + it) * nn + o];
            const size_t bc = ((size_t)b * ncat + n) * nn + o;
            const double base = (acc == 1 || acc == 6) ? A.vicen[bc] : acc == 2 ? A.vsnon[bc] : A.aicen[bc];     // (the old state)
            double w;                                                                                       // :1456-1513
            switch (acc) {
            case 0: case 1: case 2: w = base * told[n]; break;
            case 3: w = base * oldP[0][n] * told[n]; break;
            case 4: w = base * oldP[1][n] * told[n]; break;
            case 5: w = base * oldP[0][n] * oldP[1][n] * told[n]; break;
            case 6: w = base * oldP[2][n] * told[n]; break;
            default: w = 0.0;
            }
            atr[n] = w;
        }
        const bool to_nr = acc == 2 || acc == 6 || (acc == 0 && it + 1 != A.nt_alvl) || (acc == 1 && it + 1 != A.nt_vlvl);      // :1969, :1982
        _Pragma("unroll")
        for (int n = 0; n < ncat; n++) {
            if (!(mask & (1u << n))) continue;
            const double t = told[n];
            switch (acc) {                                                                                  // :1752-1842
            case 0: atr[n] = atr[n] - ardg1n[n] * t; break;
            case 1: atr[n] = atr[n] - virdgn[n] * t; break;
            case 2: atr[n] = atr[n] - vsrdgn[n] * t; break;
            case 3: atr[n] = atr[n] - ardg1n[n] * oldP[0][n] * t; break;
            case 4: atr[n] = atr[n] - ardg1n[n] * oldP[1][n] * t; break;
            case 5: atr[n] = atr[n] - ardg1n[n] * oldP[0][n] * oldP[1][n] * t; break;
            case 6: atr[n] = atr[n] - virdgn[n] * t * oldP[2][n]; break;
            default: break;
            }
            if (!to_nr) continue;
            _Pragma("unroll")
            for (int nr = 0; nr < ncat; nr++) {                                                             // :1967-2017
                if (acc == 0) atr[nr] = atr[nr] + P.farea(n, nr)[ci] * ardg2n[n] * t;
                else {
                    const double fvol = P.fvol(n, nr)[ci];
                    if (acc == 1) atr[nr] = atr[nr] + fvol * virdgn[n] * t;
                    else if (acc == 2) atr[nr] = atr[nr] + fvol * vsrdgn[n] * fsnowrdg * t;
                    else atr[nr] = atr[nr] + fvol * virdgn[n] * oldP[2][n] * t;
                }
            }
        }
        const int d1 = A.d1[it], d2 = A.d2[it], sl = A.slot[it];
        _Pragma("unroll")
        for (int n = 0; n < ncat; n++) {                                                                    // compute_tracers (:2026-2033)
            // (selects, not newP[d1 - 1]: an index known only at run time would put the array in scratch memory)
            const double p1 = d1 == 1 ? newP[0][n] : d1 == 2 ? newP[1][n] : d1 == 3 ? newP[2][n] : 0.0;
            const double p2 = d2 == 1 ? newP[0][n] : d2 == 2 ? newP[1][n] : d2 == 3 ? newP[2][n] : 0.0;
            const int rule = A.rule[it];
            const double a_ = (rule == 1 || rule == 4 || rule == 5) ? P.anew(0, n)[ci] : 0.0;               // (the new state)
            const double v_ = (rule == 2 || rule == 6) ? P.anew(1, n)[ci] : 0.0, s_ = rule == 3 ? P.anew(2, n)[ci] : 0.0;
            const double r = compute_tracer(rule, atr[n], a_, v_, s_, p1, p2, it + 1 == A.nt_fbri, 0.0);
            if (sl == 1) newP[0][n] = r;
            else if (sl == 2) newP[1][n] = r;
            else if (sl == 3) newP[2][n] = r;
            A.trcrn[(((size_t)b * ncat + n) * A.ntrcr_dim + it) * nn + o] = r;
        }
    }
    _Pragma("unroll")
    for (int n = 0; n < ncat; n++) {
        const size_t bc = ((size_t)b * ncat + n) * nn + o;
        A.aicen[bc] = P.anew(0, n)[ci]; A.vicen[bc] = P.anew(1, n)[ci]; A.vsnon[bc] = P.anew(2, n)[ci];
    }
}
template __global__ void __launch_bounds__(64) k_ridge_tracers<0>(Slab, const BlockDesc *, RidgeArgs, RidgePool, int, const int *, int);
template __global__ void __launch_bounds__(64) k_ridge_tracers<5>(Slab, const BlockDesc *, RidgeArgs, RidgePool, int, const int *, int);

// the diagnostics (:609-720) and the final area check (:726-744) of every listed cell
__global__ void k_ridge_diag(Slab s, const BlockDesc *bd, RidgeArgs A, RidgePool P, RidgeCtl *ctl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > A.nxb) return;
    int si, sj;
    if (!ridge_listed(s, bd[b], i, j, si, sj)) return;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const double dti = 1.0 / A.dt;
    if (A.dardg1dt) A.dardg1dt[ci] = P.sc(RG_ARDG1)[ci] * dti;
    if (A.dardg2dt) A.dardg2dt[ci] = P.sc(RG_ARDG2)[ci] * dti;
    if (A.dvirdgdt) A.dvirdgdt[ci] = P.sc(RG_VIRDG)[ci] * dti;
    if (A.opening) A.opening[ci] = P.sc(RG_AOPEN)[ci] * dti;
    for (int n = 0; n < A.ncat; n++) {
        const size_t bc = ((size_t)b * A.ncat + n) * nn + o;
        const double a1 = P.ardg1n(n)[ci], a2 = P.ardg2n(n)[ci], vr = P.virdgn(n)[ci], m = P.mraftn(n)[ci];
        if (A.dardg1ndt) A.dardg1ndt[bc] = a1 * dti;
        if (A.dardg2ndt) A.dardg2ndt[bc] = a2 * dti;
        if (A.dvirdgndt) A.dvirdgndt[bc] = vr * dti;
        if (A.araftn) A.araftn[bc] = m * a2;
        if (A.vraftn) A.vraftn[bc] = m * vr;
    }
    if (A.fresh) A.fresh[ci] = A.fresh[ci] + P.sc(RG_MSNOW)[ci] * A.dti_thermo;
    if (A.fhocn) A.fhocn[ci] = A.fhocn[ci] + P.sc(RG_ESNOW)[ci] * A.dti_thermo;
    if (A.fpond) A.fpond[ci] = A.fpond[ci] - P.sc(RG_MPOND)[ci];
    if (fabs(P.sc(RG_ASUM)[ci] - 1.0) > 1.0e-11) atomicMin(&ctl->key, ridge_key(b, 2, 0, o));
}

}  // namespace evpk
