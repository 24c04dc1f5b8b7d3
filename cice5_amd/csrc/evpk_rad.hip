// evpk_rad.hip -- the shortwave of ice_step on the device.  Included by evpk_api.hip behind evpk_therm1s.hip.
//   k_shortwave_ccsm3   step_radiation (source/ice_step_mod.F90:1364-1524) on its calc_Tsfc / not-dEdd branch: shortwave_ccsm3
//                       (source/ice_shortwave.F90:425-646) with compute_albedos (:652-861) or constant_albedos (:867-1011) and
//                       absorbed_solar (:1020-1238), and at once behind it the albedo lines of coupling_prep
//                       (drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586): the four aggregated albedos, albice, albsno and
//                       scale_factor.  One launch for every category of every block.
//   k_prep_radiation    prep_radiation (source/ice_step_mod.F90:33-145): scale_factor = netsw / scale_factor on the physical cells and
//                       the rescaling of the per-category radiation arrays on the cell list.  drivers/auscom/CICE_RunMod.F90:332-338
//                       compiles the call out: an AusCOM host does not make it.
// One thread per cell of the block arrays, x along the lanes, that walks the categories in order: the 2-D sums carry the reference's
// bits, every input plane is read once, every output plane is written once (the zeros of cells that are not listed included), and every
// access is a coalesced 8-byte access along x.
// Initialisation on EVERY cell of the block arrays, ghost cells included (ice_step_mod.F90:1408-1423, ice_shortwave.F90:523, :538,
// :737-777, :1106-1116): coszen = 0.5, the four category albedos = the ocean albedo of the cell, zero albicen, albsnon, fswsfcn, fswintn,
// fswthrun, Sswabsn, Iswabsn and fswpenln.  The ocean albedo is ocn_albedo2D (AusCOM, :759-772) or, where that is NULL, the scalar albocn.
// Cell list (:527-536): physical cells with aicen > puny AND tmask -- the stated departure of evpk_thermo_vertical, kept so that every
// column kernel lists the same cells.
// Operation order: the Fortran's, -ffp-contract=off.  min / max are a comparison and a select; atan is evpk_atan, exp is dev_exp;
// tranbot = exp(((-kappav) hilyr) k); the sums of albicen, albsnon, swabsv, swabsi and scale_factor run left to right as written.
// Sswabsn stays zero: the CCSM3 scheme absorbs nothing in snow layers.  The aggregation (every cell, ghost cells included, on the
// caller's aicen) needs no second pass and no atomics.  alvdr_ai .. alidf_ai are plain copies of the four sums: the caller aliases them.
#pragma once

#include "evpk_fmath2.h"

namespace evpk {

// compiled-in constants (include/evpk.h cites the lines)
namespace rad {
constexpr double kappav = 1.4, Timelt = 0.0, dT_melt = 1.0, dalb_mlt = -0.075, dalb_mltv = -0.1, dalb_mlti = -0.15, i0vis = 0.70,
                 warmice = 0.68, coldice = 0.70, warmsnow = 0.77, coldsnow = 0.81;
}  // namespace rad

struct RadArgs {
    const double *aicen, *vicen, *vsnon, *trcrn;                        // (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx)
    const double *swvdr, *swvdf, *swidr, *swidf, *ocn_albedo2D;         // (nb, ny, nx); ocn_albedo2D may be null
    double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon, *fswsfcn, *fswintn, *fswthrun;      // (nb, ncat, ny, nx)
    double *Sswabsn, *Iswabsn, *fswpenln;                               // (nb, ncat, nslyr | nilyr | nilyr + 1, ny, nx); fswpenln may be null
    double *coszen, *alvdr, *alidr, *alvdf, *alidf, *albice, *albsno, *scale_factor;                   // (nb, ny, nx)
    int ncat, ntrcr_dim, nxb, nyb, nilyr, nslyr, nt_Tsfc, constant_albedos;
    double puny, albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, albocn, awtvdr, awtidr, awtvdf, awtidf;
};

template <int NC, int NL, int NS>
__global__ void __launch_bounds__(64) k_shortwave_ccsm3(Slab s, const BlockDesc *bd, RadArgs A) {
    using namespace rad;
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    if (i > A.nxb) return;
    const int ncat = NC ? NC : A.ncat, nilyr = NL ? NL : A.nilyr, nslyr = NS ? NS : A.nslyr;
    const int b = blockIdx.z;
    const double c0 = 0.0, c1 = 1.0, c2 = 2.0, c4 = 4.0, p5 = 0.5, puny = A.puny;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    const bool ocean = itd_ocean(s, bd[b], i, j);
    const double ocn = A.ocn_albedo2D ? A.ocn_albedo2D[ci] : A.albocn;
    const double swvdr = A.swvdr[ci], swvdf = A.swvdf[ci], swidr = A.swidr[ci], swidf = A.swidf[ci];
    const double fhtan = evpk_atan(A.ahmax * c4);                                        // ice_shortwave.F90:735
    const double rnilyr = (double)nilyr;
    double alvdf = c0, alidf = c0, alvdr = c0, alidr = c0, albice = c0, albsno = c0;
    const double coszen = p5;                                                            // :523
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        const double aicen = A.aicen[bc];
        double alvdrn = ocn, alidrn = ocn, alvdfn = ocn, alidfn = ocn, albin = c0, albsn = c0;         // :759-775
        double fswsfc = c0, fswint = c0, fswthru = c0, fswpen = c0;                      // :1106-1116
        double hilyr = c0;
        const bool listed = ocean && aicen > puny;                                       // :527-536 and tmask
        if (listed) {
            const double vicen = A.vicen[bc], vsnon = A.vsnon[bc];
            const double Tsfc = A.trcrn[(lo * A.ntrcr_dim + (A.nt_Tsfc - 1)) * nn + o];
            const double hi = vicen / aicen;
            const double hs = vsnon / aicen;
            double alvdfni, alidfni, alvdfns, alidfns;
            if (A.constant_albedos) {                                                    // :964-1009
                if (hs > puny) {
                    alvdfn = Tsfc >= -c2 * puny ? warmsnow : coldsnow;
                } else {
                    alvdfn = Tsfc >= -c2 * puny ? warmice : coldice;
                }
                alidfn = alvdfn;
                alvdrn = alvdfn;
                alidrn = alidfn;
                alvdfni = alvdfn; alidfni = alidfn; alvdfns = alvdfn; alidfns = alidfn;
            } else {                                                                     // :786-859
                const double fh = litd_min(evpk_atan(hi * c4) / fhtan, c1);
                const double albo = ocn * (c1 - fh);
                alvdfni = A.albicev * fh + albo;
                alidfni = A.albicei * fh + albo;
                const double dTs = Timelt - Tsfc;
                const double fT = litd_min(dTs / dT_melt - c1, c0);
                alvdfni = alvdfni - dalb_mlt * fT;
                alidfni = alidfni - dalb_mlt * fT;
                alvdfni = litd_max(alvdfni, ocn);
                alidfni = litd_max(alidfni, ocn);
                alvdfns = ocn; alidfns = ocn;
                double asnow = c0;
                if (hs > puny) {
                    alvdfns = A.albsnowv - dalb_mltv * fT;
                    alidfns = A.albsnowi - dalb_mlti * fT;
                    asnow = hs / (hs + A.snowpatch);
                }
                alvdfn = alvdfni * (c1 - asnow) + alvdfns * asnow;
                alidfn = alidfni * (c1 - asnow) + alidfns * asnow;
                alvdrn = alvdfn;                                                         // (direct = diffuse: the same operands)
                alidrn = alidfn;
            }
            const double alvdrni = alvdfni, alidrni = alidfni, alvdrns = alvdfns, alidrns = alidfns;   // :830-833
            albin = ((A.awtvdr * alvdrni + A.awtidr * alidrni) + A.awtvdf * alvdfni) + A.awtidf * alidfni;
            albsn = ((A.awtvdr * alvdrns + A.awtidr * alidrns) + A.awtvdf * alvdfns) + A.awtidf * alidfns;
            // absorbed_solar (:1118-1166)
            double asnow = c0;
            if (hs > puny) asnow = hs / (hs + A.snowpatch);
            const double swabsv = swvdr * ((c1 - alvdrni) * (c1 - asnow) + (c1 - alvdrns) * asnow) +
                                  swvdf * ((c1 - alvdfni) * (c1 - asnow) + (c1 - alvdfns) * asnow);
            const double swabsi = swidr * ((c1 - alidrni) * (c1 - asnow) + (c1 - alidrns) * asnow) +
                                  swidf * ((c1 - alidfni) * (c1 - asnow) + (c1 - alidfns) * asnow);
            const double swabs = swabsv + swabsi;
            const double fswpenvdr = ((swvdr * (c1 - alvdrni)) * (c1 - asnow)) * i0vis;
            const double fswpenvdf = ((swvdf * (c1 - alvdfni)) * (c1 - asnow)) * i0vis;
            fswpen = fswpenvdr + fswpenvdf;
            fswsfc = swabs - fswpen;
            hilyr = hi / rnilyr;                                                         // :1180-1181
        }
        A.alvdrn[bc] = alvdrn; A.alidrn[bc] = alidrn; A.alvdfn[bc] = alvdfn; A.alidfn[bc] = alidfn;
        A.albicen[bc] = albin; A.albsnon[bc] = albsn;
        // the ice layers (:1172-1211); a cell that is not listed writes its zeros
        double trantop = listed ? c1 : c0, tranbot = c0;
        if (A.fswpenln) A.fswpenln[(lo * (nilyr + 1)) * nn + o] = fswpen;
        _Pragma("unroll")
        for (int k = 1; k <= nilyr; k++) {
            if (listed) tranbot = dev_exp(((-kappav) * hilyr) * (double)k);
            A.Iswabsn[(lo * nilyr + (k - 1)) * nn + o] = fswpen * (trantop - tranbot);
            trantop = tranbot;
            if (A.fswpenln) A.fswpenln[(lo * (nilyr + 1) + k) * nn + o] = fswpen * tranbot;
        }
        if (listed) {
            fswthru = fswpen * tranbot;
            fswint = fswpen - fswthru;
        }
        A.fswsfcn[bc] = fswsfc; A.fswintn[bc] = fswint; A.fswthrun[bc] = fswthru;
        for (int k = 0; k < nslyr; k++) A.Sswabsn[(lo * nslyr + k) * nn + o] = c0;      // :538
        // coupling_prep (CICE_RunMod.F90:523-548): every cell of the block arrays
        alvdf = alvdf + alvdfn * aicen;
        alidf = alidf + alidfn * aicen;
        alvdr = alvdr + alvdrn * aicen;
        alidr = alidr + alidrn * aicen;
        if (coszen > puny) {
            albice = albice + albin * aicen;
            albsno = albsno + albsn * aicen;
        }
    }
    A.coszen[ci] = coszen;
    A.alvdf[ci] = alvdf; A.alidf[ci] = alidf; A.alvdr[ci] = alvdr; A.alidr[ci] = alidr;
    A.albice[ci] = albice; A.albsno[ci] = albsno;
    A.scale_factor[ci] = ((swvdr * (c1 - alvdr) + swvdf * (c1 - alvdf)) + swidr * (c1 - alidr)) + swidf * (c1 - alidf);     // :582-586
}
template __global__ void __launch_bounds__(64) k_shortwave_ccsm3<0, 0, 0>(Slab, const BlockDesc *, RadArgs);
template __global__ void __launch_bounds__(64) k_shortwave_ccsm3<5, 4, 1>(Slab, const BlockDesc *, RadArgs);

struct PrepRadArgs {
    const double *aice, *aicen, *swvdr, *swvdf, *swidr, *swidf, *alvdr_ai, *alvdf_ai, *alidr_ai, *alidf_ai;
    double *scale_factor, *fswfac, *fswsfcn, *fswintn, *fswthrun, *fswpenln, *Sswabsn, *Iswabsn;       // fswpenln may be null
    int ncat, nxb, nyb, nilyr, nslyr;
    double puny;
};

template <int NC, int NL, int NS>
__global__ void __launch_bounds__(64) k_prep_radiation(Slab s, const BlockDesc *bd, PrepRadArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    const int j = blockIdx.y + 1;
    if (i > A.nxb) return;
    const int b = blockIdx.z;
    const BlockDesc d = bd[b];
    if (!(i >= d.ilo && i <= d.ihi && j >= d.jlo && j <= d.jhi)) return;               // ghost cells keep the caller's values
    const int ncat = NC ? NC : A.ncat, nilyr = NL ? NL : A.nilyr, nslyr = NS ? NS : A.nslyr;
    const double c0 = 0.0, c1 = 1.0, puny = A.puny;
    const size_t nn = (size_t)A.nyb * A.nxb, o = (size_t)(j - 1) * A.nxb + (i - 1), ci = (size_t)b * nn + o;
    double sf = A.scale_factor[ci];
    if (A.aice[ci] > c0 && sf > puny) {                                                  // ice_step_mod.F90:86-94
        const double netsw = ((A.swvdr[ci] * (c1 - A.alvdr_ai[ci]) + A.swvdf[ci] * (c1 - A.alvdf_ai[ci])) + A.swidr[ci] * (c1 - A.alidr_ai[ci])) +
                             A.swidf[ci] * (c1 - A.alidf_ai[ci]);
        sf = netsw / sf;
    } else {
        sf = c1;
    }
    A.scale_factor[ci] = sf;
    A.fswfac[ci] = sf;
    if (!itd_ocean(s, d, i, j)) return;                                                  // (the cell list requires tmask)
    _Pragma("unroll")
    for (int n = 1; n <= ncat; n++) {
        const size_t lo = (size_t)b * ncat + (n - 1), bc = lo * nn + o;
        if (!(A.aicen[bc] > puny)) continue;                                             // :108
        A.fswsfcn[bc] = sf * A.fswsfcn[bc];
        A.fswintn[bc] = sf * A.fswintn[bc];
        A.fswthrun[bc] = sf * A.fswthrun[bc];
        if (A.fswpenln)
            for (int k = 0; k <= nilyr; k++) { double *q = A.fswpenln + (lo * (nilyr + 1) + k) * nn + o; *q = sf * (*q); }
        for (int k = 0; k < nslyr; k++) { double *q = A.Sswabsn + (lo * nslyr + k) * nn + o; *q = sf * (*q); }
        for (int k = 0; k < nilyr; k++) { double *q = A.Iswabsn + (lo * nilyr + k) * nn + o; *q = sf * (*q); }
    }
}
template __global__ void __launch_bounds__(64) k_prep_radiation<0, 0, 0>(Slab, const BlockDesc *, PrepRadArgs);
template __global__ void __launch_bounds__(64) k_prep_radiation<5, 4, 1>(Slab, const BlockDesc *, PrepRadArgs);

}  // namespace evpk
