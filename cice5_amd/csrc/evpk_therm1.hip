// evpk_therm1.hip -- thermo_vertical (source/ice_therm_vertical.F90:79-531) as step_therm1 calls it per category and block
// (source/ice_step_mod.F90:364-540), BL99 path: ktherm = 1, heat_capacity, calc_Tsfc and l_brine all .true. -- on the device and on the
// caller's block arrays as they are.  Included by evpk_api.hip (one translation unit) behind evpk_therm2.hip.
//   init_vertical_profile (:845-1273) with calculate_Tin_from_qin (ice_therm_shared.F90:62-90) and its five stop checks
//   temperature_changes (ice_therm_bl99.F90:51-928): conductivity (:940-1062, MU71 and bubbly), the move of excess Iswabs / Sswabs into
//       fswsfc (non-CCSM: frac = 0.9, dTemp = 0.02), the iteration up to nitermax = 500 with surface_heat_flux / dsurface_heat_flux_dTsf
//       (ice_therm_shared.F90:98-226), get_matrix_elements_calc_Tsfc (:1172-1480), tridiag_solver (:1763-1840), conditions 1 - 5
//   thickness_changes (:1283-2020) with freeboard (:2031-2170) and adjust_enthalpy (:2177-2280); einter is not built (it is only printed)
//   conservation_check_vthermo (:2283-2406), the freshn / fsaltn / fhocnn / fpond lines (:482-503), update_state_vthermo (:2417-2540)
// thermo_vertical looks at no neighbour.  One thread per cell of the block arrays walks the categories n = 1 .. ncat in order: frz_onset,
// mlt_onset and the fpond sum get the reference's category order, the 2-D forcing is loaded once, and the lanes' iteration counts add up
// over ncat solves.  <NC, NL, NS> = <5, 4, 1> keeps the matrix (6 rows) and every layer profile in registers: every loop over layers is
// unrolled, and where the Fortran indexes with a computed row (the Tsf row, adjust_enthalpy's k1 / k2) the row is resolved by selects.
// <0, 0, 0> is generic (ncat <= 16, nilyr, nslyr <= 8).  <5, 4, 1> is built for two waves per SIMD (__launch_bounds__(64, 2)): 255 VGPRs
// and 76 bytes of scratch per lane (24 VGPRs spilled), against 254 VGPRs + 8 AGPRs without scratch at one wave per SIMD, which took
// 1.45 times as long at 3600 x 2700, 5 categories.
// Departure: the cell list is physical cells with tmask and aicen > puny (the reference: every physical cell with aicen > puny; land
// carries no ice).  Land and ghost cells of the in / out arrays keep the caller's values; the fifteen output planes are written on every
// cell, zero where the cell is not listed (:251-280, ice_step_mod.F90:366-371).
// Operation order: the Fortran's, -ffp-contract=off.  min / max are a comparison and a select (litd_min / litd_max); exp is dev_exp;
// x**2, x**3, x**4 are x*x, x*x*x, (x*x)*(x*x); sqrt is the IEEE one.  ktherm = 1 makes qmlt, emlt_atm, emlt_ocn and fadvocn zero: the
// statements that only feed them are left out, the additions of those zeros are kept.
// A stop is one 64-bit key, the smallest wins (itd_key): block | category - 1 | the position in the reference's check sequence | cell
// (counting up: every check returns at its first cell).  The sequence: zTsn > Tmax layer 1 .. nslyr, zTsn < Tmin layer 1 .. nslyr, then per
// ice layer zSin < min_salin - puny, zTin > Tmlts, zTin < Tmin, then no convergence, then ferr > ferrmax.
#pragma once

namespace evpk {

constexpr int T1_MAXL = 8;          // nilyr, nslyr at most
enum { T1_STOP_TSN_HIGH = 1, T1_STOP_TSN_LOW = 2, T1_STOP_SALIN = 3, T1_STOP_TIN_HIGH = 4, T1_STOP_TIN_LOW = 5, T1_STOP_NITER = 6,
       T1_STOP_ENERGY = 7 };

// the constants that are neither in evpk_itd_constants nor in evpk_params (include/evpk.h cites the lines)
namespace th1 {
constexpr double cp_ocn = 4218.0, Lvap = 2.501e6, Tffresh = 273.15, TTTice = 5897.8, qqqice = 11637800.0, emissivity = 0.95,
                 stefan_boltzmann = 567.0e-10, depressT = 0.054, ksno = 0.30, kice = 2.03, betak = 0.13, kimin = 0.10, Tsf_errmax = 5.0e-4,
                 ferrmax = 1.0e-3, frac_sw = 0.9, dTemp = 0.02;
constexpr int nitermax = 500;
}  // namespace th1

struct ThermoArgs {
    double *aicen, *vicen, *vsnon, *trcrn;                              // (nb, ncat, ny, nx) x 3, (nb, ncat, ntrcr_dim, ny, nx)
    const double *flw, *potT, *Qa, *rhoa, *fsnow, *fbot, *Tbot;         // (nb, ny, nx)
    const double *shcoef, *lhcoef;                                      // (nb, ncat, ny, nx)
    double *fswsfcn, *fswintn, *Sswabsn, *Iswabsn;                      // (nb, ncat, ny, nx) x 2, (nb, ncat, nslyr | nilyr, ny, nx)
    double *fpond, *mlt_onset, *frz_onset;                              // (nb, ny, nx); fpond nullptr unless topo ponds
    double *flwoutn, *evapn, *freshn, *fsaltn, *fhocnn, *fsensn, *flatn, *fsurfn, *fcondtopn, *melttn, *meltsn, *meltbn, *congeln, *snoicen,
           *dsnown;                                                     // (nb, ncat, ny, nx), written on every cell
    int ncat, ntrcr_dim, nxb, nyb, nilyr, nslyr, nt_Tsfc, nt_qice, nt_qsno, nt_sice, nt_apnd, nt_hpnd, tr_pond_topo, conduct;
    double dt, yday, min_salin, puny, rhoi, rhos, rhow, cp_ice, Lfresh, hs_min, Tmin, salinity;
};

// adjust_enthalpy (:2177-2280) on the n layers of one profile.  The while loop takes at most 2 n - 1 steps; z1(k1), z1(k1+1), qn(k1),
// z2(k2), z2(k2+1) and hq(k2) are resolved by selects, so that no array is indexed with k1 / k2
template <int N>
__device__ __forceinline__ void t1_adjust_enthalpy(int n_rt, const double *z1, const double *z2, double hlyr, double hn, double *qn, double puny) {
    const int n = N ? N : n_rt;
    constexpr int NA = N ? N : T1_MAXL;
    const double c0 = 0.0, c1 = 1.0;
    double rhlyr = c0;
    if (hn > puny) rhlyr = c1 / hlyr;
    double hq[NA];
    _Pragma("unroll")
    for (int k = 0; k < n; k++) hq[k] = c0;
    int k1 = 0, k2 = 0;
    _Pragma("unroll")
    for (int s = 0; s < 2 * n - 1; s++) {
        if (k1 < n && k2 < n) {
            double a1 = c0, b1 = c0, a2 = c0, b2 = c0, q = c0;
            _Pragma("unroll")
            for (int c = 0; c < n; c++) {
                if (c == k1) { a1 = z1[c]; b1 = z1[c + 1]; q = qn[c]; }
                if (c == k2) { a2 = z2[c]; b2 = z2[c + 1]; }
            }
            double hovlp = litd_min(b1, b2) - litd_max(a1, a2);
            hovlp = litd_max(hovlp, c0);
            _Pragma("unroll")
            for (int c = 0; c < n; c++)
                if (c == k2) hq[c] = hq[c] + hovlp * q;
            if (b1 > b2) k2++; else k1++;
        }
    }
    _Pragma("unroll")
    for (int k = 0; k < n; k++) qn[k] = hq[k] * rhlyr;
}

// the 2-D forcing of one cell, loaded once for all categories
struct T1Forcing { double flw, potT, Qa, rhoa, fsnow, fbot, Tbot; };

// one thermo_vertical call on one listed cell: category plane index bc, t = tracer 1 of the category at the cell.  Returns -1, or the
// position of the first failing check in the reference's sequence
template <int NL, int NS>
__device__ __forceinline__ int t1_category(const ThermoArgs &T, const T1Forcing &F, size_t nn, size_t bc, size_t lo, double *t, double &fpond,
                                           double &mlt_onset, double &frz_onset) {
    using namespace th1;
    const int nilyr = NL ? NL : T.nilyr, nslyr = NS ? NS : T.nslyr;
    constexpr int LA = NL ? NL : T1_MAXL, SA = NS ? NS : T1_MAXL, MA = LA + SA + 1;
    const double c0 = 0.0, c1 = 1.0, c2 = 2.0, c4 = 4.0, p1 = 0.1, p5 = 0.5, p001 = 0.001;
    const double puny = T.puny, dt = T.dt, rhoi = T.rhoi, rhos = T.rhos, cp_ice = T.cp_ice, Lfresh = T.Lfresh, Tmin = T.Tmin;
    const double rnilyr = (double)nilyr, rnslyr = (double)nslyr;
    const size_t o = bc - lo * nn;                      // the cell inside its plane
    const double aicen = T.aicen[bc], vicen = T.vicen[bc], vsnon = T.vsnon[bc];
    int seq = 1 << 20;

    // ---- init_vertical_profile (:954-1271) ----
    double Tsf = t[(size_t)(T.nt_Tsfc - 1) * nn];
    double hin = vicen / aicen, hsn = vsnon / aicen;
    double hilyr = hin / rnilyr, hslyr = hsn / rnslyr;
    double einit = c0;
    double zqsn[SA], zTsn[SA], zqin[LA], zTin[LA], zSin[LA], Tmlts[LA];
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {
        double Tmax;
        if (hslyr > T.hs_min / rnslyr) {
            zqsn[k] = t[(size_t)(T.nt_qsno - 1 + k) * nn];
            Tmax = -zqsn[k] * puny * rnslyr / (rhos * cp_ice * vsnon);
        } else {
            zqsn[k] = -rhos * Lfresh;
            Tmax = puny;
        }
        zTsn[k] = (Lfresh + zqsn[k] / rhos) / cp_ice;
        if (zTsn[k] > Tmax) seq = min(seq, k);
        else if (zTsn[k] < Tmin) seq = min(seq, nslyr + k);
    }
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {
        if (zTsn[k] > c0) { zTsn[k] = c0; zqsn[k] = -rhos * Lfresh; }
        einit = einit + hslyr * zqsn[k];
    }
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) {
        zSin[k] = t[(size_t)(T.nt_sice - 1 + k) * nn];
        if (zSin[k] < T.min_salin - puny) seq = min(seq, 2 * nslyr + 3 * k);
        Tmlts[k] = -zSin[k] * depressT;
        zqin[k] = t[(size_t)(T.nt_qice - 1 + k) * nn];
        {       // calculate_Tin_from_qin, l_brine
            const double aa1 = cp_ice, bb1 = (cp_ocn - cp_ice) * Tmlts[k] - zqin[k] / rhoi - Lfresh, cc1 = Lfresh * Tmlts[k];
            zTin[k] = litd_min((-bb1 - __dsqrt_rn(bb1 * bb1 - c4 * aa1 * cc1)) / (c2 * aa1), Tmlts[k]);
        }
        if (zTin[k] > Tmlts[k]) seq = min(seq, 2 * nslyr + 3 * k + 1);
        else if (zTin[k] < Tmin) seq = min(seq, 2 * nslyr + 3 * k + 2);
        if (zTin[k] > c0) { zTin[k] = c0; zqin[k] = -rhoi * Lfresh; }
        einit = einit + hilyr * zqin[k];
    }
    if (seq != 1 << 20) return seq;
    const double worki = hin, works = hsn;

    // ---- temperature_changes (ice_therm_bl99.F90:239-362) ----
    const bool l_snow = hslyr > T.hs_min / rnslyr;
    bool l_cold = true;
    double fcondbot = c0, dTsf_prev = c0, dfsens_dT = c0, dflat_dT = c0, dflwout_dT = c0, einex = c0;
    const double dt_rhoi_hlyr = dt / (rhoi * hilyr);
    double Tsn_init[SA], Tsn_start[SA], etas[SA], Tin_init[LA], Tin_start[LA], kh[MA], Iswabs[LA], Sswabs[SA];
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {
        Tsn_init[k] = zTsn[k]; Tsn_start[k] = zTsn[k];
        etas[k] = l_snow ? dt / (rhos * cp_ice * hslyr) : c0;
    }
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) { Tin_init[k] = zTin[k]; Tin_start[k] = zTin[k]; }
    {       // conductivity (:988-1060)
        double kilyr[LA];
        _Pragma("unroll")
        for (int k = 0; k < nilyr; k++) {
            if (T.conduct == 0) kilyr[k] = kice + betak * zSin[k] / litd_min(-puny, zTin[k]);
            else kilyr[k] = (2.11 - 0.011 * zTin[k] + 0.09 * zSin[k] / litd_min(-puny, zTin[k])) * rhoi / 917.0;
            kilyr[k] = litd_max(kilyr[k], kimin);
        }
        if (l_snow) {
            kh[0] = c2 * ksno / hslyr;
            kh[nslyr] = c2 * ksno * kilyr[0] / (ksno * hilyr + kilyr[0] * hslyr);
        } else {
            kh[0] = c0;
            kh[nslyr] = c2 * kilyr[0] / hilyr;
        }
        kh[nslyr + nilyr] = c2 * kilyr[nilyr - 1] / hilyr;
        _Pragma("unroll")
        for (int k = 2; k <= nslyr; k++) kh[k - 1] = l_snow ? c2 * ksno * ksno / ((ksno + ksno) * hslyr) : c0;
        _Pragma("unroll")
        for (int k = 2; k <= nilyr; k++) kh[k - 1 + nslyr] = c2 * kilyr[k - 2] * kilyr[k - 1] / ((kilyr[k - 2] + kilyr[k - 1]) * hilyr);
    }
    double fswsfc = T.fswsfcn[bc], fswint = T.fswintn[bc];
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) {       // excess Iswabs into the surface (:309-336)
        Iswabs[k] = T.Iswabsn[(lo * nilyr + k) * nn + o];
        double Iswabs_tmp = c0;
        if (Tin_init[k] <= Tmlts[k] - dTemp) {
            const double ci = cp_ice - Lfresh * Tmlts[k] / (Tin_init[k] * Tin_init[k]);
            Iswabs_tmp = litd_min(Iswabs[k], frac_sw * (Tmlts[k] - Tin_init[k]) * ci / dt_rhoi_hlyr);
        }
        if (Iswabs_tmp < puny) Iswabs_tmp = c0;
        const double dswabs = litd_min(Iswabs[k] - Iswabs_tmp, fswint);
        fswsfc = fswsfc + dswabs;
        fswint = fswint - dswabs;
        Iswabs[k] = Iswabs_tmp;
    }
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {       // (:341-362)
        Sswabs[k] = T.Sswabsn[(lo * nslyr + k) * nn + o];
        if (l_snow) {
            double Sswabs_tmp = c0;
            if (Tsn_init[k] <= -dTemp) Sswabs_tmp = litd_min(Sswabs[k], -frac_sw * Tsn_init[k] / etas[k]);
            if (Sswabs_tmp < puny) Sswabs_tmp = c0;
            const double dswabs = litd_min(Sswabs[k] - Sswabs_tmp, fswint);
            fswsfc = fswsfc + dswabs;
            fswint = fswint - dswabs;
            Sswabs[k] = Sswabs_tmp;
        }
    }

    // ---- the iteration (:369-853): this cell leaves it when its `converged` stays true ----
    const double shcoef = T.shcoef[bc], lhcoef = T.lhcoef[bc];
    double flwoutn = c0, fsensn = c0, flatn = c0, fsurfn = c0, fcondtopn = c0;
    bool converged = false;
    for (int niter = 1; niter <= nitermax && !converged; niter++) {
        converged = true;
        double dfsurf_dT = c0, avg_Tsi = c0, enew = c0;
        einex = c0;
        double etai[LA];
        _Pragma("unroll")
        for (int k = 0; k < nilyr; k++) {
            const double ci = cp_ice - Lfresh * Tmlts[k] / (zTin[k] * Tin_init[k]);
            etai[k] = dt_rhoi_hlyr / ci;
        }
        {       // surface_heat_flux, dsurface_heat_flux_dTsf (ice_therm_shared.F90:138-155, :203-218)
            const double TsfK = Tsf + Tffresh, tmpvar = c1 / TsfK;
            const double qsat = qqqice * dev_exp(-TTTice * tmpvar), Qsfc = qsat / F.rhoa;
            const double flwdabs = emissivity * F.flw;
            flwoutn = -emissivity * stefan_boltzmann * ((TsfK * TsfK) * (TsfK * TsfK));
            fsensn = shcoef * (F.potT - TsfK);
            flatn = lhcoef * (F.Qa - Qsfc);
            fsurfn = fswsfc + flwdabs + flwoutn + fsensn + flatn;
            const double dQsfc_dTsf = TTTice * tmpvar * tmpvar * (qsat / F.rhoa);
            dflwout_dT = -emissivity * stefan_boltzmann * c4 * (TsfK * TsfK * TsfK);
            dfsens_dT = -shcoef;
            dflat_dT = -lhcoef * dQsfc_dTsf;
            dfsurf_dT = dflwout_dT + dfsens_dT + dflat_dT;
        }
        fcondtopn = l_snow ? kh[0] * (Tsf - zTsn[0]) : kh[nslyr] * (Tsf - zTin[0]);
        if (Tsf >= c0 && fsurfn < fcondtopn) Tsf = -puny;
        const double Tsf_start = Tsf;
        l_cold = Tsf < c0;
        // get_matrix_elements_calc_Tsfc (:1261-1468); row r is the Fortran's row r + 1
        double sb[MA], dg[MA], sp[MA], rh[MA], Tmat[MA], wgamma[MA];
        _Pragma("unroll")
        for (int k = 0; k <= nslyr; k++) { sb[k] = c0; dg[k] = c1; sp[k] = c0; rh[k] = c0; }
        if (l_cold) {
            if (l_snow) { sb[0] = c0; dg[0] = dfsurf_dT - kh[0]; sp[0] = kh[0]; rh[0] = dfsurf_dT * Tsf - fsurfn; }
            else { sb[nslyr] = c0; dg[nslyr] = dfsurf_dT - kh[nslyr]; sp[nslyr] = kh[nslyr]; rh[nslyr] = dfsurf_dT * Tsf - fsurfn; }
        }
        if (l_snow) {
            if (l_cold) {
                sb[1] = -etas[0] * kh[0];
                sp[1] = -etas[0] * kh[1];
                dg[1] = c1 + etas[0] * (kh[0] + kh[1]);
                rh[1] = Tsn_init[0] + etas[0] * Sswabs[0];
            } else {
                sb[1] = c0;
                sp[1] = -etas[0] * kh[1];
                dg[1] = c1 + etas[0] * (kh[0] + kh[1]);
                rh[1] = Tsn_init[0] + etas[0] * kh[0] * Tsf + etas[0] * Sswabs[0];
            }
            _Pragma("unroll")
            for (int k = 2; k <= nslyr; k++) {
                sb[k] = -etas[k - 1] * kh[k - 1];
                sp[k] = -etas[k - 1] * kh[k];
                dg[k] = c1 + etas[k - 1] * (kh[k - 1] + kh[k]);
                rh[k] = Tsn_init[k - 1] + etas[k - 1] * Sswabs[k - 1];
            }
        }
        if (nilyr > 1) {
            {       // top ice layer
                const int k = nslyr, kr = nslyr + 1;
                if (l_snow || l_cold) {
                    sb[kr] = -etai[0] * kh[k];
                    sp[kr] = -etai[0] * kh[k + 1];
                    dg[kr] = c1 + etai[0] * (kh[k] + kh[k + 1]);
                    rh[kr] = Tin_init[0] + etai[0] * Iswabs[0];
                } else {
                    sb[kr] = c0;
                    sp[kr] = -etai[0] * kh[k + 1];
                    dg[kr] = c1 + etai[0] * (kh[k] + kh[k + 1]);
                    rh[kr] = Tin_init[0] + etai[0] * Iswabs[0] + etai[0] * kh[k] * Tsf;
                }
            }
            {       // bottom ice layer
                const int ki = nilyr - 1, k = nilyr - 1 + nslyr, kr = nilyr + nslyr;
                sb[kr] = -etai[ki] * kh[k];
                sp[kr] = c0;
                dg[kr] = c1 + etai[ki] * (kh[k] + kh[k + 1]);
                rh[kr] = Tin_init[ki] + etai[ki] * Iswabs[ki] + etai[ki] * kh[k + 1] * F.Tbot;
            }
        } else {    // a single ice layer
            const int k = nslyr, kr = nslyr + 1;
            if (l_snow || l_cold) {
                sb[kr] = -etai[0] * kh[k];
                sp[kr] = c0;
                dg[kr] = c1 + etai[0] * (kh[k] + kh[k + 1]);
                rh[kr] = Tin_init[0] + etai[0] * Iswabs[0] + etai[0] * kh[k + 1] * F.Tbot;
            } else {
                sb[kr] = c0;
                sp[kr] = c0;
                dg[kr] = c1 + etai[0] * (kh[k] + kh[k + 1]);
                rh[kr] = Tin_init[0] + etai[0] * Iswabs[0] + etai[0] * kh[k] * Tsf + etai[0] * kh[k + 1] * F.Tbot;
            }
        }
        _Pragma("unroll")
        for (int ki = 2; ki <= nilyr - 1; ki++) {
            const int k = ki - 1 + nslyr, kr = ki + nslyr;
            sb[kr] = -etai[ki - 1] * kh[k];
            sp[kr] = -etai[ki - 1] * kh[k + 1];
            dg[kr] = c1 + etai[ki - 1] * (kh[k] + kh[k + 1]);
            rh[kr] = Tin_init[ki - 1] + etai[ki - 1] * Iswabs[ki - 1];
        }
        {       // tridiag_solver (:1808-1832)
            const int nmat = nilyr + nslyr + 1;
            double wbeta = dg[0];
            Tmat[0] = rh[0] / wbeta;
            _Pragma("unroll")
            for (int k = 1; k < nmat; k++) {
                wgamma[k] = sp[k - 1] / wbeta;
                wbeta = dg[k] - sb[k] * wgamma[k];
                Tmat[k] = (rh[k] - sb[k] * Tmat[k - 1]) / wbeta;
            }
            _Pragma("unroll")
            for (int k = nmat - 2; k >= 0; k--) Tmat[k] = Tmat[k] - wgamma[k + 1] * Tmat[k + 1];
        }
        // conditions 1 and 2 (:587-647)
        if (l_cold) Tsf = l_snow ? Tmat[0] : Tmat[nslyr];
        else Tsf = c0;
        double dTsf = Tsf - Tsf_start, avg_Tsf = c0;
        if (Tsf > puny) {
            Tsf = c0;
            dTsf = -Tsf_start;
            avg_Tsi = c1;
            converged = false;
        } else if (niter > 1 && Tsf_start <= -puny && fabs(dTsf) > puny && fabs(dTsf_prev) > puny &&
                   -dTsf / (dTsf_prev + puny * puny) > p5) {
            avg_Tsf = c1;
            avg_Tsi = c1;
            dTsf = p5 * dTsf;
            converged = false;
        }
        Tsf = Tsf + avg_Tsf * p5 * (Tsf_start - Tsf);
        _Pragma("unroll")
        for (int k = 0; k < nslyr; k++) {       // (:653-687)
            zTsn[k] = l_snow ? Tmat[k + 1] : c0;
            zTsn[k] = litd_min(zTsn[k], c0);
            zTsn[k] = zTsn[k] + avg_Tsi * p5 * (Tsn_start[k] - zTsn[k]);
            zqsn[k] = -rhos * (Lfresh - cp_ice * zTsn[k]);
            enew = enew + hslyr * zqsn[k];
            Tsn_start[k] = zTsn[k];
        }
        double dqmat[LA];
        bool reduce_kh[LA];
        _Pragma("unroll")
        for (int k = 0; k < nilyr; k++) {       // (:692-760)
            dqmat[k] = c0;
            reduce_kh[k] = false;
            zTin[k] = Tmat[k + 1 + nslyr];
            if (zTin[k] > Tmlts[k] - puny) {
                const double dTmat = zTin[k] - Tmlts[k];
                dqmat[k] = rhoi * dTmat * (cp_ice - Lfresh * Tmlts[k] / (zTin[k] * zTin[k]));
                zTin[k] = Tmlts[k];
                reduce_kh[k] = true;
            }
            zTin[k] = zTin[k] + avg_Tsi * p5 * (Tin_start[k] - zTin[k]);
            zqin[k] = -rhoi * (cp_ice * (Tmlts[k] - zTin[k]) + Lfresh * (c1 - Tmlts[k] / zTin[k]) - cp_ocn * Tmlts[k]);
            enew = enew + hilyr * zqin[k];
            einex = einex + hilyr * dqmat[k];
            Tin_start[k] = zTin[k];
        }
        // conditions 3 and 4 (:776-797)
        if (fabs(dTsf) > Tsf_errmax) converged = false;
        fsurfn = fsurfn + dTsf * dfsurf_dT;
        fcondtopn = l_snow ? kh[0] * (Tsf - zTsn[0]) : kh[nslyr] * (Tsf - zTin[0]);
        if (Tsf >= c0 && fsurfn < fcondtopn) converged = false;
        dTsf_prev = dTsf;
        // condition 5 (:807-838)
        fcondbot = kh[nslyr + nilyr] * (zTin[nilyr - 1] - F.Tbot);
        fcondbot = fcondbot + einex / dt;
        const double ferr = fabs((enew - einit) / dt - (fcondtopn - fcondbot + fswint));
        if (ferr > 0.9 * ferrmax) {
            converged = false;
            _Pragma("unroll")
            for (int k = 0; k < nilyr; k++) {
                if (reduce_kh[k] && dqmat[k] > c0) {
                    const double frac = litd_max(0.5 * (c1 - ferr / fabs(fcondtopn - fcondbot)), p1);
                    kh[k + nslyr + 1] = kh[k + nslyr + 1] * frac;
                    kh[k + nslyr] = kh[k + nslyr + 1];
                }
            }
        }
    }
    if (!converged) return 2 * nslyr + 3 * nilyr;
    flwoutn = flwoutn + dTsf_prev * dflwout_dT;       // (:921-923)
    fsensn = fsensn + dTsf_prev * dfsens_dT;
    flatn = flatn + dTsf_prev * dflat_dT;

    // ---- thickness_changes (ice_therm_vertical.F90:1439-2018), ktherm = 1, l_brine ----
    double hsn_new = c0, dzi[LA], dzs[SA], qm[LA];
    double meltt = c0, melts = c0, meltb = c0, congel = c0, snoice = c0, dsnow = c0;
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) { dzi[k] = hilyr; qm[k] = zqin[k] - c0; }
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) dzs[k] = hslyr;
    double wk1 = -flatn * dt;
    double esub = litd_max(wk1, c0);
    const double econ = litd_min(wk1, c0);
    wk1 = (fsurfn - fcondtopn) * dt;
    double etop_mlt = litd_max(wk1, c0);
    wk1 = (fcondbot - F.fbot) * dt;
    double ebot_mlt = litd_max(wk1, c0);
    const double ebot_gro = litd_min(wk1, c0);
    double evapn = c0;
    if (hsn > puny) {           // condensation onto snow, else onto ice
        const double dhs = econ / (zqsn[0] - rhos * Lvap);
        dzs[0] = dzs[0] + dhs;
        evapn = evapn + dhs * rhos;
    } else {
        const double dhi = econ / (qm[0] - rhoi * Lvap);
        dzi[0] = dzi[0] + dhi;
        evapn = evapn + dhi * rhoi;
    }
    {       // bottom growth (:1563-1605)
        const int L = nilyr - 1;
        const double qbotmax = -p5 * rhoi * Lfresh;
        const double Tmlt = -zSin[L] * depressT;
        double qbot = -rhoi * (cp_ice * (Tmlt - F.Tbot) + Lfresh * (c1 - Tmlt / F.Tbot) - cp_ocn * Tmlt);
        qbot = litd_min(qbot, qbotmax);
        const double dhi = ebot_gro / qbot;
        const double hqtot = dzi[L] * zqin[L] + dhi * qbot;
        dzi[L] = dzi[L] + dhi;
        if (dzi[L] > puny) {
            zqin[L] = hqtot / dzi[L];
            qm[L] = zqin[L] - c0;
        }
        congel = congel + dhi;
        if (dhi > puny && frz_onset < puny) frz_onset = T.yday;
    }
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {       // sublimation and top melt of snow (:1636-1655)
        const double qsub = zqsn[k] - rhos * Lvap;
        double dhs = litd_max(-dzs[k], esub / qsub);
        dzs[k] = dzs[k] + dhs;
        esub = esub - dhs * qsub;
        esub = litd_max(esub, c0);
        evapn = evapn + dhs * rhos;
        dhs = litd_max(-dzs[k], etop_mlt / zqsn[k]);
        dzs[k] = dzs[k] + dhs;
        etop_mlt = etop_mlt - dhs * zqsn[k];
        etop_mlt = litd_max(etop_mlt, c0);
        if (dhs < -puny && mlt_onset < puny) mlt_onset = T.yday;
        melts = melts - dhs;
    }
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) {       // sublimation and top melt of ice (:1672-1698)
        const double qsub = qm[k] - rhoi * Lvap;
        double dhi = litd_max(-dzi[k], esub / qsub);
        dzi[k] = dzi[k] + dhi;
        esub = esub - dhi * qsub;
        esub = litd_max(esub, c0);
        evapn = evapn + dhi * rhoi;
        if (qm[k] < c0) {
            dhi = litd_max(-dzi[k], etop_mlt / qm[k]);
        } else {
            qm[k] = c0;
            dhi = -dzi[k];
        }
        dzi[k] = dzi[k] + dhi;
        etop_mlt = litd_max(etop_mlt - dhi * qm[k], c0);
        if (dhi < -puny && mlt_onset < puny) mlt_onset = T.yday;
        meltt = meltt - dhi;
    }
    _Pragma("unroll")
    for (int k = nilyr - 1; k >= 0; k--) {      // bottom melt of ice (:1715-1727)
        double dhi;
        if (qm[k] < c0) {
            dhi = litd_max(-dzi[k], ebot_mlt / qm[k]);
        } else {
            qm[k] = c0;
            dhi = -dzi[k];
        }
        dzi[k] = dzi[k] + dhi;
        ebot_mlt = litd_max(ebot_mlt - dhi * qm[k], c0);
        meltb = meltb - dhi;
    }
    _Pragma("unroll")
    for (int k = nslyr - 1; k >= 0; k--) {      // ... then of snow (:1742-1745)
        const double dhs = litd_max(-dzs[k], ebot_mlt / zqsn[k]);
        dzs[k] = dzs[k] + dhs;
        ebot_mlt = ebot_mlt - dhs * zqsn[k];
        ebot_mlt = litd_max(ebot_mlt, c0);
    }
    double fhocnn = F.fbot + (esub + etop_mlt + ebot_mlt) / dt;
    if (F.fsnow > c0) {         // snowfall (:1780-1794)
        hsn_new = F.fsnow / rhos * dt;
        const double zqsnew = -rhos * Lfresh;
        const double hstot = dzs[0] + hsn_new;
        if (hstot > c0) {
            zqsn[0] = (dzs[0] * zqsn[0] + hsn_new * zqsnew) / hstot;
            zqsn[0] = litd_min(zqsn[0], -rhos * Lfresh);
            dzs[0] = hstot;
        }
    }
    hin = c0;
    hsn = c0;
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) hin = hin + dzi[k];
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) {
        hsn = hsn + dzs[k];
        dsnow = dsnow + dzs[k] - hslyr;
    }
    {       // freeboard (:2100-2165)
        double dhin = c0, dhsn = c0, hqs = c0;
        const double wk = hsn - hin * (T.rhow - rhoi) / rhos;
        if (wk > puny && hsn > puny) {
            dhsn = litd_min(wk * rhoi / T.rhow, hsn);
            dhin = dhsn * rhos / rhoi;
        }
        if (dhin > puny) {
            _Pragma("unroll")
            for (int k = nslyr - 1; k >= 0; k--) {
                const double dhs = litd_min(dhsn, dzs[k]);
                hsn = hsn - dhs;
                dsnow = dsnow - dhs;
                dzs[k] = dzs[k] - dhs;
                dhsn = dhsn - dhs;
                dhsn = litd_max(dhsn, c0);
                hqs = hqs + dhs * zqsn[k];
            }
            const double w = dzi[0] + dhin;
            hin = hin + dhin;
            zqin[0] = (dzi[0] * zqin[0] + hqs) / w;
            dzi[0] = w;
            snoice = snoice + dhin;
        }
    }
    if (hin > c0) hilyr = hin / rnilyr; else { hin = c0; hilyr = c0; }       // (:1852-1863)
    if (hsn > c0) hslyr = hsn / rnslyr; else { hsn = c0; hslyr = c0; }
    {
        double z1[LA + 1], z2[LA + 1];
        z1[0] = c0; z2[0] = c0;
        _Pragma("unroll")
        for (int k = 0; k < nilyr - 1; k++) { z1[k + 1] = z1[k] + dzi[k]; z2[k + 1] = z2[k] + hilyr; }
        z1[nilyr] = hin; z2[nilyr] = hin;
        t1_adjust_enthalpy<NL>(nilyr, z1, z2, hilyr, hin, zqin, puny);
    }
    if (nslyr > 1) {
        double z1[SA + 1], z2[SA + 1];
        z1[0] = c0; z2[0] = c0;
        _Pragma("unroll")
        for (int k = 0; k < nslyr - 1; k++) { z1[k + 1] = z1[k] + dzs[k]; z2[k + 1] = z2[k] + hslyr; }
        z1[nslyr] = hsn; z2[nslyr] = hsn;
        t1_adjust_enthalpy<NS>(nslyr, z1, z2, hslyr, hsn, zqsn, puny);
    }
    double efinal = -evapn * Lvap;          // (:1980-2018)
    evapn = evapn / dt;
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) efinal = efinal + hslyr * zqsn[k];
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) efinal = efinal + hilyr * zqin[k];
    fhocnn = fhocnn + c0 / dt;
    efinal = efinal + c0;

    // ---- conservation_check_vthermo (:2359-2363) ----
    {
        const double einp = (fsurfn - flatn + fswint - fhocnn - F.fsnow * Lfresh - c0) * dt;
        const double ferr = fabs(efinal - einit - einp) / dt;
        if (ferr > ferrmax) return 2 * nslyr + 3 * nilyr + 1;
    }

    // ---- the fluxes to the ocean (:482-503) ----
    const double dhi = hin - worki, dhs = hsn - works - hsn_new;
    const double freshn = c0 + evapn - (rhoi * dhi + rhos * dhs) / dt;
    const double fsaltn = c0 - rhoi * dhi * T.salinity * p001 / dt;
    fhocnn = fhocnn + c0;
    if (hin == c0 && T.tr_pond_topo)
        fpond = fpond - aicen * t[(size_t)(T.nt_apnd - 1) * nn] * t[(size_t)(T.nt_hpnd - 1) * nn];

    // ---- update_state_vthermo (:2474-2535), Tf = Tbot ----
    const bool ice = hin > c0;
    if (ice) {
        T.vicen[bc] = aicen * hin;
        T.vsnon[bc] = aicen * hsn;
        t[(size_t)(T.nt_Tsfc - 1) * nn] = Tsf;
    } else {
        T.aicen[bc] = c0;
        T.vicen[bc] = c0;
        T.vsnon[bc] = c0;
        t[(size_t)(T.nt_Tsfc - 1) * nn] = F.Tbot;
    }
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) t[(size_t)(T.nt_qice - 1 + k) * nn] = ice ? zqin[k] : c0;
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) t[(size_t)(T.nt_qsno - 1 + k) * nn] = ice ? zqsn[k] : c0;

    T.fswsfcn[bc] = fswsfc; T.fswintn[bc] = fswint;
    _Pragma("unroll")
    for (int k = 0; k < nilyr; k++) T.Iswabsn[(lo * nilyr + k) * nn + o] = Iswabs[k];
    _Pragma("unroll")
    for (int k = 0; k < nslyr; k++) T.Sswabsn[(lo * nslyr + k) * nn + o] = Sswabs[k];
    T.flwoutn[bc] = flwoutn; T.evapn[bc] = evapn; T.freshn[bc] = freshn; T.fsaltn[bc] = fsaltn; T.fhocnn[bc] = fhocnn;
    T.fsensn[bc] = fsensn; T.flatn[bc] = flatn; T.fsurfn[bc] = fsurfn; T.fcondtopn[bc] = fcondtopn;
    T.melttn[bc] = meltt; T.meltsn[bc] = melts; T.meltbn[bc] = meltb; T.congeln[bc] = congel; T.snoicen[bc] = snoice; T.dsnown[bc] = dsnow;
    return -1;
}

template <int NC, int NL, int NS>
__global__ void __launch_bounds__(64, NL ? 2 : 1) k_thermo_vertical(Slab s, const BlockDesc *bd, ThermoArgs T, unsigned long long *key) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    const int b = blockIdx.z;
    if (i > T.nxb) return;
    const int ncat = NC ? NC : T.ncat;
    const double c0 = 0.0;
    const size_t nn = (size_t)T.nyb * T.nxb, o = (size_t)(j - 1) * T.nxb + (i - 1), ci = (size_t)b * nn + o;
    const bool ocean = itd_ocean(s, bd[b], i, j);
    T1Forcing F{};
    double fpond = c0, mlt_onset = c0, frz_onset = c0;
    if (ocean) {
        F.flw = T.flw[ci]; F.potT = T.potT[ci]; F.Qa = T.Qa[ci]; F.rhoa = T.rhoa[ci]; F.fsnow = T.fsnow[ci]; F.fbot = T.fbot[ci]; F.Tbot = T.Tbot[ci];
        mlt_onset = T.mlt_onset[ci]; frz_onset = T.frz_onset[ci];
        if (T.tr_pond_topo) fpond = T.fpond[ci];
    }
    bool any = false;
    _Pragma("unroll 1")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        if (ocean && T.aicen[bc] > T.puny) {
            any = true;
            const int seq = t1_category<NL, NS>(T, F, nn, bc, lo, T.trcrn + lo * T.ntrcr_dim * nn + o, fpond, mlt_onset, frz_onset);
            if (seq >= 0) { atomicMin(key, itd_key(b, n - 1, seq, (unsigned)o)); return; }      // a stop: the arrays are undefined
        } else {
            T.flwoutn[bc] = c0; T.evapn[bc] = c0; T.freshn[bc] = c0; T.fsaltn[bc] = c0; T.fhocnn[bc] = c0;
            T.fsensn[bc] = c0; T.flatn[bc] = c0; T.fsurfn[bc] = c0; T.fcondtopn[bc] = c0;
            T.melttn[bc] = c0; T.meltsn[bc] = c0; T.meltbn[bc] = c0; T.congeln[bc] = c0; T.snoicen[bc] = c0; T.dsnown[bc] = c0;
        }
    }
    if (any) {
        T.mlt_onset[ci] = mlt_onset; T.frz_onset[ci] = frz_onset;
        if (T.tr_pond_topo) T.fpond[ci] = fpond;
    }
}
template __global__ void __launch_bounds__(64, 1) k_thermo_vertical<0, 0, 0>(Slab, const BlockDesc *, ThermoArgs, unsigned long long *);
template __global__ void __launch_bounds__(64, 2) k_thermo_vertical<5, 4, 1>(Slab, const BlockDesc *, ThermoArgs, unsigned long long *);

}  // namespace evpk
