// evpk_dedd.hip -- the Delta-Eddington shortwave of ice_step on the device.  Included by evpk_api.hip behind evpk_rad.hip.
//   k_shortwave_dedd    step_radiation (source/ice_step_mod.F90:1408-1451) on its calc_Tsfc / dEdd branch: run_dEdd
//                       (source/ice_shortwave.F90:1251-1577) with shortwave_dEdd_set_snow (:3782-3883), shortwave_dEdd_set_pond
//                       (:3893-3958), shortwave_dEdd (:1607-2024), compute_dEdd (:2034-3261) and solution_dEdd (:3270-3772), and at once
//                       behind it the albedo lines of coupling_prep (drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586).  One
//                       launch for every category of every block.
// The shape of k_shortwave_ccsm3: one thread per cell of the block arrays, x along the lanes, that walks the categories in order, so the
// 2-D sums carry the reference's bits with no second pass and no atomics, and every plane access is a coalesced 8-byte access along x.
// Per listed, lit (cell, category) up to three surface types (bare ice under fi > 0, snow under fs > 0, pond under fp > puny) times three
// spectral bands, each a column of nslyr + nilyr + 2 layers; a layer costs ten dev_exp: extins, trnlay and eight Gaussian angles.
// Registers: in the <5, 4, 1> instantiation every loop over layers has a compile-time trip count and is unrolled, so the seven layer
// properties (rdir, rdif_a, rdif_b, tdir, tdif_a, tdif_b, trnlay), the four downward interface arrays (trndir, trntdr, trndif, rdndif) and
// the two arrays the upward sweep leaves (dfdir swdr, dfdif swdf; rupdir and rupdif are scalars of the sweep) are registers: no scratch.
// The loops over categories, surface types, bands and Gaussian angles stay rolled (code size).  The generic <0, 0, 0> indexes arrays of
// DEDD_MAXK layers at run time and may use scratch.
// Tables (evpk_dedd_tables.h): the 32-radius snow tables and the Gaussian points are copied to LDS at kernel start -- the radius index
// differs from lane to lane, which the constant cache would serialise.  The lookup (index and delr) is done once per category, the three
// interpolations once per (category, band): every snow layer of a column has the same grain radius (:3873-3880, :2756).
// The adjusted ice and pond optical properties (ki_ssl .. gi_p_int, :2655-2721) are uniform per call: evpk_step_radiation_dedd computes
// them on the host in the Fortran's order (dedd_iops) and passes them by value.
// The LVL instantiations (evpk_step_radiation_dedd_lvl) run the tr_pond_lvl block of run_dEdd (:1450-1514) in the place of the tr_pond_cesm
// lines: dhsn is read and written on the listed cells, ffracn and fsnow are read, and the snow depth the radiation sees is the infiltrated
// one.  The pond scheme is a template parameter so that the instantiations without it keep their registers (no scratch in <5, 4, 1, 0>).
// Operation order: the Fortran's, -ffp-contract=off; x**2 is x*x; min / max are a comparison and a select; sqrt is the IEEE one; exp is
// dev_exp; the statement functions of solution_dEdd (:3500-3508) are evaluated exactly as written.
#pragma once

#include "evpk_dedd_tables.h"

namespace evpk {

constexpr int DEDD_MAXL = 8;                               // nilyr, nslyr <= 8 (T1_MAXL)
constexpr int DEDD_MAXK = 2 * DEDD_MAXL + 2;               // layers 0 .. klev, klev = nslyr + nilyr + 1
constexpr int DEDD_LDS = dedd::NMBRAD + 3 * dedd::NSPINT * dedd::NMBRAD + 2 * dedd::NGMAX;      // doubles of LDS: the tables

struct DeddIop {                                           // [band]
    double ki_ssl[3], wi_ssl[3], gi_ssl[3], ki_dl[3], wi_dl[3], gi_dl[3], ki_int[3], wi_int[3], gi_int[3];
    double ki_p_ssl[3], wi_p_ssl[3], gi_p_ssl[3], ki_p_int[3], wi_p_int[3], gi_p_int[3];
};

// the R_ice / R_pnd adjustment of compute_dEdd (:2655-2721), both signs of each, on the host
inline void dedd_iops(double R_ice, double R_pnd, DeddIop &o) {
    using namespace dedd;
    const double c0 = 0.0, c1 = 1.0;
    auto tune = [&](const double *k_mn, const double *w_mn, const double *g_mn, double R, double fp, double fm, double *k, double *w, double *g) {
        for (int ns = 0; ns < NSPINT; ns++) {
            double sigp;
            if (R >= c0) {
                sigp = k_mn[ns] * w_mn[ns] * (c1 + fp * R);
            } else {
                sigp = k_mn[ns] * w_mn[ns] * (c1 + fm * R);
                sigp = sigp > c0 ? sigp : c0;
            }
            k[ns] = sigp + k_mn[ns] * (c1 - w_mn[ns]);
            w[ns] = sigp / k[ns];
            g[ns] = g_mn[ns];
        }
    };
    tune(ki_ssl_mn, wi_ssl_mn, gi_ssl_mn, R_ice, fp_ice, fm_ice, o.ki_ssl, o.wi_ssl, o.gi_ssl);
    tune(ki_dl_mn, wi_dl_mn, gi_dl_mn, R_ice, fp_ice, fm_ice, o.ki_dl, o.wi_dl, o.gi_dl);
    tune(ki_int_mn, wi_int_mn, gi_int_mn, R_ice, fp_ice, fm_ice, o.ki_int, o.wi_int, o.gi_int);
    tune(ki_p_ssl_mn, wi_p_ssl_mn, gi_p_ssl_mn, R_pnd, fp_pnd, fm_pnd, o.ki_p_ssl, o.wi_p_ssl, o.gi_p_ssl);
    tune(ki_p_int_mn, wi_p_int_mn, gi_p_int_mn, R_pnd, fp_pnd, fm_pnd, o.ki_p_int, o.wi_p_int, o.gi_p_int);
}

struct DeddArgs {
    const double *aicen, *vicen, *vsnon, *trcrn;                        // (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx)
    const double *swvdr, *swvdf, *swidr, *swidf;                        // (nb, ny, nx)
    double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon, *albpndn, *apeffn, *snowfracn, *fswsfcn, *fswintn, *fswthrun;
    double *Sswabsn, *Iswabsn, *fswpenln;                               // fswpenln may be null
    double *coszen, *alvdr, *alidr, *alvdf, *alidf, *albice, *albsno, *albpnd, *apeff_ai, *scale_factor;       // (nb, ny, nx)
    int ncat, ntrcr_dim, nxb, nyb, nilyr, nslyr, nt_Tsfc, nt_apnd, nt_hpnd, tr_pond_cesm;
    double puny, rhos, R_snw, dT_mlt, rsnw_mlt, kalg, hs0, pndaspect, awtvdr, awtidr, awtvdf, awtidf;
    DeddIop iop;
    // tr_pond_lvl (the LVL instantiations only; behind the members above so that theirs keep their places)
    double *dhsn;                                                       // (nb, ncat, ny, nx), in / out on the listed cells
    const double *ffracn, *fsnow;                                       // (nb, ncat, ny, nx), (nb, ny, nx)
    int nt_alvl, nt_ipnd, linitonly;
    double hs1, dt;
};

// the statement functions of solution_dEdd (:3500-3508), as written
__device__ __forceinline__ double dedd_alpha(double w, double uu, double gg, double e) {
    return ((0.75 * w) * uu) * ((1.0 + gg * (1.0 - w)) / (1.0 - ((e * e) * uu) * uu));
}
__device__ __forceinline__ double dedd_agamm(double w, double uu, double gg, double e) {
    return (0.5 * w) * ((1.0 + (((3.0 * gg) * (1.0 - w)) * uu) * uu) / (1.0 - ((e * e) * uu) * uu));
}

// LVL = 1: the tr_pond_lvl block of run_dEdd (:1450-1514) sets the ponds, and the snow depth and fraction the radiation sees; LVL = 0 is
// the kernel as it was (tr_pond_cesm or no pond tracer, chosen at run time).
template <int NC, int NL, int NS, int LVL>
__global__ void __launch_bounds__(64) k_shortwave_dedd(Slab s, const BlockDesc *bd, DeddArgs A) {
    using namespace dedd;
    __shared__ double lds[DEDD_LDS];
    double *const l_rsnw = lds, *const l_Qs = lds + NMBRAD, *const l_ws = l_Qs + NSPINT * NMBRAD, *const l_gs = l_ws + NSPINT * NMBRAD,
                 *const l_gpt = l_gs + NSPINT * NMBRAD, *const l_gwt = l_gpt + NGMAX;
    for (int q = threadIdx.x; q < NMBRAD; q += blockDim.x) l_rsnw[q] = rsnw_tab[q];
    for (int q = threadIdx.x; q < NSPINT * NMBRAD; q += blockDim.x) {
        l_Qs[q] = Qs_tab[q / NMBRAD][q % NMBRAD];
        l_ws[q] = ws_tab[q / NMBRAD][q % NMBRAD];
        l_gs[q] = gs_tab[q / NMBRAD][q % NMBRAD];
    }
    for (int q = threadIdx.x; q < NGMAX; q += blockDim.x) { l_gpt[q] = gauspt[q]; l_gwt[q] = gauswt[q]; }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    if (i > A.nxb) return;
    constexpr int KA = NL ? NS + NL + 2 : DEDD_MAXK;                    // layers 0 .. klev
    constexpr int LA = NL ? NL : DEDD_MAXL, SA = NS ? NS : DEDD_MAXL;
    constexpr int UNR = NL ? KA + 1 : 1;                                // the two sweeps over the layers: unrolled where the count is known
    const int ncat = NC ? NC : A.ncat, nilyr = NL ? NL : A.nilyr, nslyr = NS ? NS : A.nslyr;
    const int klev = nslyr + nilyr + 1, klevp = klev + 1, kii = nslyr + 1;
    const int b = blockIdx.z;
    const double c0 = 0.0, c1 = 1.0, c2 = 2.0, c3 = 3.0, c4 = 4.0, p5 = 0.5, p25 = 0.25, c1p5 = 1.5, p01 = 0.01, puny = A.puny;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const bool ocean = itd_ocean(s, bd[b], i, j);
    const double swvdr = A.swvdr[ci], swvdf = A.swvdf[ci], swidr = A.swidr[ci], swidf = A.swidf[ci];
    const double netsw = ((swvdr + swidr) + swvdf) + swidf;                                  // :1812
    const bool lit = netsw > puny;
    double fnidr = c0;                                                                   // :1762-1765
    if (swidr + swidf > puny) fnidr = swidr / (swidr + swidf);
    // coszen: on a listed cell with netsw > puny max(puny, coszen) is stored back (:1814); coupling_prep reads it after run_dEdd
    double coszen = A.coszen[ci];
    if (ocean && lit) {
        bool any = false;
        for (int n = 1; n <= ncat; n++) any = any || A.aicen[((size_t)b * ncat + (n - 1)) * nn + o] > puny;
        if (any) {
            coszen = litd_max(puny, coszen);
            A.coszen[ci] = coszen;
        }
    }
    // per cell: mu0, the refracted mu0n (:3535-3541) and the Fresnel layer (:3653-3677)
    const double mu0 = litd_max(coszen, p01);
    const double mu0r = sqrt(c1 - ((c1 - mu0 * mu0) / (refindx * refindx)));
    double Rf_dir_a, Tf_dir_a;
    {
        const double R1 = (mu0 - refindx * mu0r) / (mu0 + refindx * mu0r);
        const double R2 = (refindx * mu0 - mu0r) / (refindx * mu0 + mu0r);
        const double T1 = c2 * mu0 / (mu0 + refindx * mu0r);
        const double T2 = c2 * mu0 / (refindx * mu0 + mu0r);
        Rf_dir_a = p5 * (R1 * R1 + R2 * R2);
        Tf_dir_a = p5 * (T1 * T1 + T2 * T2) * refindx * mu0r / mu0;
    }
    const double Rf_dif_a = cp063, Tf_dif_a = c1 - Rf_dif_a, Rf_dif_b = cp455, Tf_dif_b = c1 - Rf_dif_b;
    // band weights and the snow grain adjustment (:2602-2612)
    const double wght2 = cp67 + (cp78 - cp67) * (c1 - fnidr), wght3 = c1 - wght2;
    const double frfac = fr_max * fnidr + fr_min * (c1 - fnidr);
    const double rnilyr = c1 / (double)nilyr, rnslyr = c1 / (double)nslyr;
    const double fsdl = p25 / rnilyr;                                                    // :2862
    double alvdf = c0, alidf = c0, alvdr = c0, alidr = c0, albice = c0, albsno = c0, albpnd = c0, apeff_ai = c0;
    _Pragma("nounroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        const double aicen = A.aicen[bc];
        double alvdrn = c0, alidrn = c0, alvdfn = c0, alidfn = c0, albin = c0, albsn = c0, albpn = c0, apeff = c0, snowfrac = c0;
        double fswsfc = c0, fswint = c0, fswthru = c0;
        double Sswabs[SA], Iswabs[LA], fswpenl[LA + 1];
        _Pragma("unroll")
        for (int k = 0; k < nslyr; k++) Sswabs[k] = c0;
        _Pragma("unroll")
        for (int k = 0; k < nilyr; k++) Iswabs[k] = c0;
        _Pragma("unroll")
        for (int k = 0; k <= nilyr; k++) fswpenl[k] = c0;
        if (ocean && aicen > puny) {                                                     // :1407-1415 and tmask
            const double vsnon = A.vsnon[bc];
            const double Tsfc = A.trcrn[(lo * A.ntrcr_dim + (A.nt_Tsfc - 1)) * nn + o];
            // shortwave_dEdd_set_snow (:3857-3880)
            double hs = vsnon / aicen;
            double fs = c0;
            if (hs >= hs_min) {
                fs = c1;
                if (A.hs0 > puny) fs = litd_min(hs / A.hs0, c1);
            }
            double rsnw;
            {
                const double dTs = Timelt - Tsfc;
                const double fT = -litd_min(dTs / A.dT_mlt - c1, c0);
                double rsnw_nm = rsnw_nonmelt - A.R_snw * rsnw_sig;
                rsnw_nm = litd_max(rsnw_nm, rsnw_fresh);
                rsnw_nm = litd_min(rsnw_nm, A.rsnw_mlt);
                rsnw = rsnw_nm + (A.rsnw_mlt - rsnw_nm) * fT;
                rsnw = litd_max(rsnw, rsnw_fresh);
                rsnw = litd_min(rsnw, A.rsnw_mlt);
            }
            // ponds (:1432-1448 or :1540-1550)
            double fp, hp;
            if constexpr (LVL) {                                                         // :1450-1514
                const double *t = A.trcrn + lo * A.ntrcr_dim * nn + o;
                const double alvl = t[(size_t)(A.nt_alvl - 1) * nn], apnd = t[(size_t)(A.nt_apnd - 1) * nn];
                const double ipn = (alvl * apnd) * t[(size_t)(A.nt_ipnd - 1) * nn];     // the lid thickness averaged over the ice
                double dhs = A.dhsn[bc];
                const double snowfall = A.fsnow[ci] * A.dt;
                if (!A.linitonly && ipn > puny && dhs < puny && snowfall > hs_min) dhs = hs - snowfall;
                const double spn = hs - dhs;                                             // snow depth on the pond ice
                if (!A.linitonly && ipn * spn < puny) dhs = c0;
                A.dhsn[bc] = dhs;
                fp = apnd * alvl;
                hp = t[(size_t)(A.nt_hpnd - 1) * nn];
                fp = (c1 - A.ffracn[bc]) * fp;
                if (dhs > puny && spn >= puny && A.hs1 > puny) {                         // taper with the snow on the pond ice
                    const double asnow = litd_min(spn / A.hs1, c1);
                    fp = (c1 - asnow) * fp;
                }
                double hpi = hp;                                                         // infiltrate the snow
                if (hpi > puny) {
                    const double rhofresh = th1s::rhofresh;
                    const double rp = (rhofresh * hpi) / (rhofresh * hpi + A.rhos * hs);
                    if (rp < 0.15) {
                        fp = c0;
                        hp = c0;
                    } else {
                        const double hmx = (hs * (rhofresh - A.rhos)) / rhofresh;
                        const double tmp = litd_max(c0, copysign(c1, hpi - hmx));
                        hpi = (rhofresh * hpi + (A.rhos * hs) * tmp) / (rhofresh - A.rhos * (c1 - tmp));
                        hs = hs - (hpi * fp) * (c1 - tmp);
                        hp = hpi * tmp;
                        fp = fp * tmp;
                    }
                }
                if (hp < hpmin) fp = c0;
                fs = litd_min(fs, c1 - fp);
                apeff = fp;
            } else if (A.tr_pond_cesm) {
                fp = A.trcrn[(lo * A.ntrcr_dim + (A.nt_apnd - 1)) * nn + o];
                hp = A.trcrn[(lo * A.ntrcr_dim + (A.nt_hpnd - 1)) * nn + o];
                if (hs >= hs_min && A.hs0 > puny) {
                    const double asnow = litd_min(hs / A.hs0, c1);
                    fp = (c1 - asnow) * fp;
                    hp = A.pndaspect * fp;
                }
                apeff = fp;
            } else {
                const double dTs = Timelt - Tsfc;
                const double fT = -litd_min(dTs / dT_pnd - c1, c0);
                apeff = pnd_fac * fT * (c1 - fs);
                fp = c0;
                hp = c0;
            }
            snowfrac = fs;
            if (lit) {                                                                   // shortwave_dEdd (:1812-1962)
                const double hi = A.vicen[bc] / aicen;
                const double fi = c1 - fs - fp;
                // the snow table lookup (:2758-2781): index and delr once per category
                const double frsnw = frfac * rsnw;
                int nr = 0;                                                              // 0: below the table, NMBRAD: at or above its end
                double delr = c0;
                if (!(frsnw < l_rsnw[0])) {
                    nr = NMBRAD;
                    if (!(frsnw >= l_rsnw[NMBRAD - 1])) {
                        for (int q = 1; q < NMBRAD; q++)
                            if (l_rsnw[q - 1] <= frsnw && frsnw < l_rsnw[q]) nr = q;
                        delr = (frsnw - l_rsnw[nr - 1]) / (l_rsnw[nr] - l_rsnw[nr - 1]);
                    }
                }
                // the ice layer thicknesses (:2630-2647)
                const double dzi = hi * rnilyr;
                double dz_ssl = litd_min(hi_ssl, hi / 30.0);
                dz_ssl = litd_min(dz_ssl, dzi / c2);
                const double dzi1 = dzi - dz_ssl;
                _Pragma("nounroll")
                for (int srftyp = 0; srftyp <= 2; srftyp++) {
                    const double f = srftyp == 0 ? fi : srftyp == 1 ? fs : fp;
                    if (!(srftyp == 0 ? fi > c0 : srftyp == 1 ? fs > c0 : fp > puny)) continue;
                    // compute_dEdd
                    const int kfrsnl = srftyp < 2 ? nslyr + 2 : 0;                      // (ksrf, :2724-2730, is taken below)
                    const double hsl = srftyp == 0 ? c0 : hs;                            // (hstmp = 0 for bare ice, :1747, :1835)
                    const double dzs = hsl * rnslyr;                                     // :2618-2627
                    const double dzs0 = litd_min(hs_ssl, dzs / c2), dzs1 = dzs - dzs0;
                    double avdr = c0, avdf = c0, aidr = c0, aidf = c0, fsfc = c0, fint = c0, fthru = c0;
                    double Sabs[SA], Iabs[LA], fthrul[LA + 1];
                    _Pragma("unroll")
                    for (int k = 0; k < nslyr; k++) Sabs[k] = c0;
                    _Pragma("unroll")
                    for (int k = 0; k < nilyr; k++) Iabs[k] = c0;
                    _Pragma("unroll")
                    for (int k = 0; k <= nilyr; k++) fthrul[k] = c0;
                    _Pragma("nounroll")
                    for (int ns = 0; ns < NSPINT; ns++) {
                        // optical properties above the sea ice (:2739-2845): tau differs between layers 0, 1 and the rest
                        double ttop0 = c0, ttop1 = c0, ttopk = c0, wtop = c0, gtop = c0;
                        if (srftyp == 1) {
                            double Qs, ws, gs;
                            const double *tQ = l_Qs + ns * NMBRAD, *tw = l_ws + ns * NMBRAD, *tg = l_gs + ns * NMBRAD;
                            if (nr == 0) {
                                Qs = tQ[0]; ws = tw[0]; gs = tg[0];
                            } else if (nr == NMBRAD) {
                                Qs = tQ[NMBRAD - 1]; ws = tw[NMBRAD - 1]; gs = tg[NMBRAD - 1];
                            } else {
                                Qs = tQ[nr - 1] * (c1 - delr) + tQ[nr] * delr;
                                ws = tw[nr - 1] * (c1 - delr) + tw[nr] * delr;
                                gs = tg[nr - 1] * (c1 - delr) + tg[nr] * delr;
                            }
                            const double ks = Qs * ((A.rhos / rhoi) * 3.0 / (4.0 * frsnw * 1.0e-6));
                            ttop0 = ks * dzs0; ttop1 = ks * dzs1; ttopk = ks * dzs;
                            wtop = ws; gtop = gs;
                        } else if (srftyp == 2) {
                            const double dz = hp / (c1 / rnslyr + c1);
                            ttop0 = ttop1 = ttopk = kw[ns] * dz;
                            wtop = ww[ns]; gtop = gw[ns];
                        }
                        // optical properties of the sea ice (:2850-2988): the surface scattering layer, the layer below it, the
                        // interior, the lowest layer
                        double t_ssl, w_ssl, g_ssl, t_dl, w_dl, g_dl, t_int, w_int, g_int, t_low, w_low, g_low;
                        const DeddIop &P = A.iop;
                        if (srftyp <= 1) {
                            t_ssl = P.ki_ssl[ns] * dz_ssl; w_ssl = P.wi_ssl[ns]; g_ssl = P.gi_ssl[ns];
                            t_dl = P.ki_dl[ns] * dzi1 * fsdl; w_dl = P.wi_dl[ns]; g_dl = P.gi_dl[ns];
                            t_int = P.ki_int[ns] * dzi; w_int = P.wi_int[ns]; g_int = P.gi_int[ns];
                            const double dzl = nilyr == 1 ? dzi1 : dzi;
                            double kabs = P.ki_int[ns] * (c1 - P.wi_int[ns]);
                            if (ns == 0) kabs = kabs + A.kalg * (0.50 / dzl);
                            const double sig = P.ki_int[ns] * P.wi_int[ns];
                            t_low = (kabs + sig) * dzl; w_low = sig / (sig + kabs); g_low = P.gi_int[ns];
                        } else {
                            t_ssl = P.ki_p_ssl[ns] * dz_ssl; w_ssl = P.wi_p_ssl[ns]; g_ssl = P.gi_p_ssl[ns];
                            t_dl = P.ki_p_int[ns] * dzi1; w_dl = P.wi_p_int[ns]; g_dl = P.gi_p_int[ns];
                            t_int = P.ki_p_int[ns] * dzi; w_int = P.wi_p_int[ns]; g_int = P.gi_p_int[ns];
                            if (hpmin <= hp && hp <= hp0) {                              // the transition to bare ice
                                double sig_i = P.ki_ssl[ns] * P.wi_ssl[ns], sig_p = P.ki_p_ssl[ns] * P.wi_p_ssl[ns];
                                double sig = sig_i + (sig_p - sig_i) * (hp / hp0);
                                double kext = sig + P.ki_p_ssl[ns] * (c1 - P.wi_p_ssl[ns]);
                                t_ssl = kext * dz_ssl; w_ssl = sig / kext; g_ssl = P.gi_p_int[ns];
                                sig_i = P.ki_dl[ns] * P.wi_dl[ns] * fsdl; sig_p = P.ki_p_int[ns] * P.wi_p_int[ns];
                                sig = sig_i + (sig_p - sig_i) * (hp / hp0);
                                kext = sig + P.ki_p_int[ns] * (c1 - P.wi_p_int[ns]);
                                t_dl = kext * dzi1; w_dl = sig / kext; g_dl = P.gi_p_int[ns];
                                sig_i = P.ki_int[ns] * P.wi_int[ns];
                                sig = sig_i + (sig_p - sig_i) * (hp / hp0);
                                kext = sig + P.ki_p_int[ns] * (c1 - P.wi_p_int[ns]);
                                t_int = kext * dzi; w_int = sig / kext; g_int = P.gi_p_int[ns];
                            }
                            t_low = nilyr == 1 ? t_dl : t_int; w_low = nilyr == 1 ? w_dl : w_int; g_low = nilyr == 1 ? g_dl : g_int;
                        }
                        const double albod = cp01 * (c1 - litd_min((double)ns, c1));       // :2992-2994
                        const double swdr = ns == 0 ? swvdr : swidr, swdf = ns == 0 ? swvdf : swidf;
                        // solution_dEdd: the downward sweep (:3563-3740)
                        double rdir[KA], rdif_a[KA], rdif_b[KA], tdir[KA], tdif_a[KA], tdif_b[KA], trnlay[KA];
                        double trndir[KA + 1], trntdr[KA + 1], trndif[KA + 1], rdndif[KA + 1];
                        trndir[0] = c1; trntdr[0] = c1; trndif[0] = c1; rdndif[0] = c0;
                        _Pragma("unroll UNR")
                        for (int k = 0; k <= klev; k++) {
                            double r_dir = c0, r_dif_a = c0, r_dif_b = c0, t_dir = c0, t_dif_a = c0, t_dif_b = c0, trn_lay = c0;
                            if (trntdr[k] > trmin) {
                                const int m = k - kii;
                                const double tautot = k == 0 ? ttop0 : k == 1 && m < 0 ? ttop1 : m < 0 ? ttopk
                                                      : m == 0 ? t_ssl : k == klev ? t_low : m == 1 ? t_dl : t_int;
                                const double wtot = m < 0 ? wtop : m == 0 ? w_ssl : k == klev ? w_low : m == 1 ? w_dl : w_int;
                                const double gtot = m < 0 ? gtop : m == 0 ? g_ssl : k == klev ? g_low : m == 1 ? g_dl : g_int;
                                const double ftot = gtot * gtot;
                                const double ts = (c1 - wtot * ftot) * tautot;
                                const double ws = (c1 - ftot) * wtot / (c1 - wtot * ftot);
                                const double gs = (gtot - ftot) / (c1 - ftot);
                                const double lm = sqrt(c3 * (c1 - ws) * (c1 - ws * gs));
                                const double ue = c1p5 * (c1 - ws * gs) / lm;
                                double mu0n = mu0r;
                                if (srftyp < 2 && k < kfrsnl) mu0n = mu0;
                                const double extins = litd_max(exp_min, dev_exp(-lm * ts));
                                const double ne = ((ue + c1) * (ue + c1) / extins) - ((ue - c1) * (ue - c1) * extins);
                                r_dif_a = (ue * ue - c1) * (c1 / extins - extins) / ne;
                                t_dif_a = c4 * ue / ne;
                                trn_lay = litd_max(exp_min, dev_exp(-ts / mu0n));
                                {
                                    const double alp = dedd_alpha(ws, mu0n, gs, lm), gam = dedd_agamm(ws, mu0n, gs, lm);
                                    const double apg = alp + gam, amg = alp - gam;
                                    r_dir = apg * r_dif_a + amg * (t_dif_a * trn_lay - c1);
                                    t_dir = apg * t_dif_a + (amg * r_dif_a - apg + c1) * trn_lay;
                                }
                                const double R1 = r_dif_a, T1 = t_dif_a;
                                double swt = c0, smr = c0, smt = c0;
                                _Pragma("nounroll")
                                for (int ng = 0; ng < NGMAX; ng++) {
                                    const double mu = l_gpt[ng], gwt = l_gwt[ng];
                                    swt = swt + mu * gwt;
                                    const double trn = litd_max(exp_min, dev_exp(-ts / mu));
                                    const double alp = dedd_alpha(ws, mu, gs, lm), gam = dedd_agamm(ws, mu, gs, lm);
                                    const double apg = alp + gam, amg = alp - gam;
                                    const double rdr = apg * R1 + amg * T1 * trn - amg;
                                    const double tdr = apg * T1 + amg * R1 * trn - apg * trn + trn;
                                    smr = smr + mu * rdr * gwt;
                                    smt = smt + mu * tdr * gwt;
                                }
                                r_dif_a = smr / swt;
                                t_dif_a = smt / swt;
                                r_dif_b = r_dif_a;
                                t_dif_b = t_dif_a;
                                if (k == kfrsnl) {                                       // the Fresnel layer on top of layer k (:3683-3700)
                                    const double rintfc = c1 / (c1 - Rf_dif_b * r_dif_a);
                                    const double t_dir0 = t_dir, r_dir0 = r_dir, r_dif_a0 = r_dif_a, t_dif_a0 = t_dif_a;
                                    t_dir = Tf_dir_a * t_dir0 + Tf_dir_a * r_dir0 * Rf_dif_b * rintfc * t_dif_a0;
                                    r_dir = Rf_dir_a + Tf_dir_a * r_dir0 * rintfc * Tf_dif_b;
                                    r_dif_a = Rf_dif_a + Tf_dif_a * r_dif_a0 * rintfc * Tf_dif_b;
                                    r_dif_b = r_dif_b + t_dif_b * Rf_dif_b * rintfc * t_dif_a0;
                                    t_dif_a = t_dif_a0 * rintfc * Tf_dif_a;
                                    t_dif_b = t_dif_b * rintfc * Tf_dif_b;
                                    trn_lay = Tf_dir_a * trn_lay;
                                }
                            }
                            rdir[k] = r_dir; rdif_a[k] = r_dif_a; rdif_b[k] = r_dif_b; tdir[k] = t_dir; tdif_a[k] = t_dif_a; tdif_b[k] = t_dif_b;
                            trnlay[k] = trn_lay;
                            trndir[k + 1] = trndir[k] * trn_lay;                         // :3730-3738
                            const double refkm1 = c1 / (c1 - rdndif[k] * r_dif_a);
                            const double tdrrdir = trndir[k] * r_dir;
                            const double tdndif = trntdr[k] - trndir[k];
                            trntdr[k + 1] = trndir[k] * t_dir + (tdndif + tdrrdir * rdndif[k]) * refkm1 * t_dif_a;
                            rdndif[k + 1] = r_dif_b + (t_dif_b * rdndif[k] * refkm1 * t_dif_a);
                            trndif[k + 1] = trndif[k] * refkm1 * t_dif_a;
                        }
                        // the upward sweep (:3754-3769) with the interface fluxes of compute_dEdd (:3026-3052) as it passes
                        double pdir[KA + 1], pdif[KA + 1];                               // dfdir swdr, dfdif swdf
                        double rupdir = albod, rupdif = albod, rupdir0 = c0, rupdif0 = c0;
                        _Pragma("unroll UNR")
                        for (int k = klevp; k >= 0; k--) {
                            if (k <= klev) {
                                const double refkp1 = c1 / (c1 - rdif_b[k] * rupdif);
                                const double up = rdir[k] + (trnlay[k] * rupdir + (tdir[k] - trnlay[k]) * rupdif) * refkp1 * tdif_b[k];
                                rupdif = rdif_a[k] + tdif_a[k] * rupdif * refkp1 * tdif_b[k];
                                rupdir = up;
                            }
                            const double refk = c1 / (c1 - rdndif[k] * rupdif);
                            double dfdir = trndir[k] + (trntdr[k] - trndir[k]) * (c1 - rupdif) * refk - trndir[k] * rupdir * (c1 - rdndif[k]) * refk;
                            if (dfdir < puny) dfdir = c0;
                            double dfdif = trndif[k] * (c1 - rupdif) * refk;
                            if (dfdif < puny) dfdif = c0;
                            pdir[k] = dfdir * swdr;
                            pdif[k] = dfdif * swdf;
                            if (k == 0) { rupdir0 = rupdir; rupdif0 = rupdif; }
                        }
                        // albedos and fluxes (:3058-3186)
                        const double p_ks = srftyp == 1 ? pdir[1] : pdir[nslyr + 2], q_ks = srftyp == 1 ? pdif[1] : pdif[nslyr + 2];
                        double tmp_0 = pdir[0] + pdif[0], tmp_ks = p_ks + q_ks, tmp_kl = pdir[klevp] + pdif[klevp];
                        if (ns == 0) {
                            avdr = rupdir0;
                            avdf = rupdif0;
                            _Pragma("unroll")
                            for (int k = 0; k <= nilyr; k++) fthrul[k] = pdir[nslyr + 2 + k] + pdif[nslyr + 2 + k];
                            fsfc = fsfc + tmp_0 - tmp_ks;
                            fint = fint + tmp_ks - tmp_kl;
                            fthru = fthru + tmp_kl;
                            if (srftyp == 1) {
                                _Pragma("unroll")
                                for (int k = 1; k <= nslyr; k++)
                                    Sabs[k - 1] = Sabs[k - 1] + pdir[k] + pdif[k] - (pdir[k + 1] + pdif[k + 1]);
                            }
                            _Pragma("unroll")
                            for (int k = 0; k < nilyr; k++) {
                                const int kk = nslyr + 2 + k;
                                const bool up = srftyp == 1 && k == 0;                   // snow over ice: SSL and DL both go to ice layer 1
                                const double pm = up ? pdir[kk - 1] : pdir[kk], qm = up ? pdif[kk - 1] : pdif[kk];
                                Iabs[k] = Iabs[k] + pm + qm - (pdir[kk + 1] + pdif[kk + 1]);
                            }
                        } else {
                            const double wght = ns == 1 ? wght2 : wght3;
                            aidr = aidr + rupdir0 * wght;
                            aidf = aidf + rupdif0 * wght;
                            tmp_0 = tmp_0 * wght;
                            tmp_ks = tmp_ks * wght;
                            tmp_kl = tmp_kl * wght;
                            fsfc = fsfc + tmp_0 - tmp_ks;
                            fint = fint + tmp_ks - tmp_kl;
                            fthru = fthru + tmp_kl;
                            if (srftyp == 1) {
                                _Pragma("unroll")
                                for (int k = 1; k <= nslyr; k++)
                                    Sabs[k - 1] = Sabs[k - 1] + (pdir[k] + pdif[k] - (pdir[k + 1] + pdif[k + 1])) * wght;
                            }
                            _Pragma("unroll")
                            for (int k = 0; k < nilyr; k++) {
                                const int kk = nslyr + 2 + k;
                                const bool up = srftyp == 1 && k == 0;
                                const double pm = up ? pdir[kk - 1] : pdir[kk], qm = up ? pdif[kk - 1] : pdif[kk];
                                Iabs[k] = Iabs[k] + (pm + qm - (pdir[kk + 1] + pdif[kk + 1])) * wght;
                            }
                        }
                    }
                    // back in compute_dEdd (:3201-3231) and shortwave_dEdd (:1848-1855 and its like)
                    fswsfc = fswsfc + fsfc * f;
                    fswint = fswint + fint * f;
                    fswthru = fswthru + fthru * f;
                    _Pragma("unroll")
                    for (int k = 0; k < nslyr; k++) Sswabs[k] = Sswabs[k] + Sabs[k] * f;
                    _Pragma("unroll")
                    for (int k = 0; k < nilyr; k++) Iswabs[k] = Iswabs[k] + Iabs[k] * f;
                    _Pragma("unroll")
                    for (int k = 0; k <= nilyr; k++) fswpenl[k] = fswpenl[k] + fthrul[k] * f;
                    alvdrn = alvdrn + avdr * f;
                    alvdfn = alvdfn + avdf * f;
                    alidrn = alidrn + aidr * f;
                    alidfn = alidfn + aidf * f;
                    const double alb = c0 + A.awtvdr * avdr + A.awtidr * aidr + A.awtvdf * avdf + A.awtidf * aidf;
                    if (srftyp == 0) albin = alb;
                    else if (srftyp == 1) albsn = alb;
                    else albpn = alb;
                }
            }
        }
        A.alvdrn[bc] = alvdrn; A.alidrn[bc] = alidrn; A.alvdfn[bc] = alvdfn; A.alidfn[bc] = alidfn;
        A.albicen[bc] = albin; A.albsnon[bc] = albsn; A.albpndn[bc] = albpn; A.apeffn[bc] = apeff; A.snowfracn[bc] = snowfrac;
        A.fswsfcn[bc] = fswsfc; A.fswintn[bc] = fswint; A.fswthrun[bc] = fswthru;
        _Pragma("unroll")
        for (int k = 0; k < nslyr; k++) A.Sswabsn[(lo * nslyr + k) * nn + o] = Sswabs[k];
        _Pragma("unroll")
        for (int k = 0; k < nilyr; k++) A.Iswabsn[(lo * nilyr + k) * nn + o] = Iswabs[k];
        if (A.fswpenln) {
            _Pragma("unroll")
            for (int k = 0; k <= nilyr; k++) A.fswpenln[(lo * (nilyr + 1) + k) * nn + o] = fswpenl[k];
        }
        // coupling_prep (CICE_RunMod.F90:523-548): every cell of the block arrays
        alvdf = alvdf + alvdfn * aicen;
        alidf = alidf + alidfn * aicen;
        alvdr = alvdr + alvdrn * aicen;
        alidr = alidr + alidrn * aicen;
        if (coszen > puny) {
            albice = albice + albin * aicen;
            albsno = albsno + albsn * aicen;
            albpnd = albpnd + albpn * aicen;
        }
        apeff_ai = apeff_ai + apeff * aicen;
    }
    A.alvdf[ci] = alvdf; A.alidf[ci] = alidf; A.alvdr[ci] = alvdr; A.alidr[ci] = alidr;
    A.albice[ci] = albice; A.albsno[ci] = albsno; A.albpnd[ci] = albpnd; A.apeff_ai[ci] = apeff_ai;
    A.scale_factor[ci] = ((swvdr * (c1 - alvdr) + swvdf * (c1 - alvdf)) + swidr * (c1 - alidr)) + swidf * (c1 - alidf);     // :582-586
}
template __global__ void __launch_bounds__(64) k_shortwave_dedd<0, 0, 0, 0>(Slab, const BlockDesc *, DeddArgs);
template __global__ void __launch_bounds__(64) k_shortwave_dedd<5, 4, 1, 0>(Slab, const BlockDesc *, DeddArgs);
template __global__ void __launch_bounds__(64) k_shortwave_dedd<0, 0, 0, 1>(Slab, const BlockDesc *, DeddArgs);
template __global__ void __launch_bounds__(64) k_shortwave_dedd<5, 4, 1, 1>(Slab, const BlockDesc *, DeddArgs);

}  // namespace evpk
