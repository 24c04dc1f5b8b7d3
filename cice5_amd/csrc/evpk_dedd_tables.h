// evpk_dedd_tables.h -- the spectral tables and scalar constants of the Delta-Eddington shortwave (k_shortwave_dedd, evpk_dedd.hip), as
// plain numbers in the project's own layout: the snow tables are [band][radius] (the reference keeps the band fastest).  Each array names
// the lines of the reference it restates; tests/test_dedd_host.py compares every one bit for bit with the copy typed for the restatement
// (tests/npdedd.py) and, where the reference is present, with the literals of those lines.  Read through evpk_dedd_table().
#pragma once

namespace evpk {
namespace dedd {

constexpr int NSPINT = 3, NMBRAD = 32, NGMAX = 8;

// snow grain radii of the table, micrometres (source/ice_shortwave.F90:2368-2376)
constexpr double rsnw_tab[NMBRAD] = {
    5.0, 7.0, 10.0, 15.0, 20.0, 30.0, 40.0, 50.0, 65.0, 80.0, 100.0, 120.0, 140.0, 170.0, 200.0, 240.0,
    290.0, 350.0, 420.0, 500.0, 570.0, 660.0, 760.0, 870.0, 1000.0, 1100.0, 1250.0, 1400.0, 1600.0, 1800.0, 2000.0, 2500.0};

// snow extinction efficiency (:2380-2413)
constexpr double Qs_tab[NSPINT][NMBRAD] = {
    {2.131798, 2.104499, 2.081580, 2.062595, 2.051403, 2.039223, 2.032383, 2.027920, 2.023444, 2.020412, 2.017608, 2.015592, 2.014083,
     2.012368, 2.011092, 2.009837, 2.008668, 2.007627, 2.006764, 2.006037, 2.005528, 2.005025, 2.004562, 2.004155, 2.003794, 2.003555,
     2.003264, 2.003037, 2.002776, 2.002590, 2.002395, 2.002071},
    {2.187756, 2.148345, 2.116885, 2.088937, 2.072422, 2.055389, 2.045751, 2.039388, 2.033137, 2.028840, 2.024863, 2.022021, 2.019887,
     2.017471, 2.015675, 2.013897, 2.012252, 2.010813, 2.009577, 2.008520, 2.007807, 2.007079, 2.006440, 2.005898, 2.005379, 2.005041,
     2.004624, 2.004291, 2.003929, 2.003627, 2.003391, 2.002922},
    {2.267358, 2.236078, 2.175067, 2.130242, 2.106610, 2.080586, 2.066394, 2.057224, 2.048055, 2.041874, 2.036046, 2.031954, 2.028853,
     2.025353, 2.022759, 2.020168, 2.017781, 2.015678, 2.013880, 2.012382, 2.011307, 2.010280, 2.009333, 2.008523, 2.007795, 2.007329,
     2.006729, 2.006230, 2.005700, 2.005276, 2.004904, 2.004241}};

// snow single scattering albedo (:2417-2450)
constexpr double ws_tab[NSPINT][NMBRAD] = {
    {0.9999994, 0.9999992, 0.9999990, 0.9999985, 0.9999979, 0.9999970, 0.9999960, 0.9999951, 0.9999936, 0.9999922, 0.9999903, 0.9999885,
     0.9999866, 0.9999838, 0.9999810, 0.9999772, 0.9999726, 0.9999670, 0.9999605, 0.9999530, 0.9999465, 0.9999382, 0.9999289, 0.9999188,
     0.9999068, 0.9998975, 0.9998837, 0.9998699, 0.9998515, 0.9998332, 0.9998148, 0.9997691},
    {0.9999673, 0.9999547, 0.9999382, 0.9999123, 0.9998844, 0.9998317, 0.9997800, 0.9997288, 0.9996531, 0.9995783, 0.9994798, 0.9993825,
     0.9992862, 0.9991434, 0.9990025, 0.9988171, 0.9985890, 0.9983199, 0.9980117, 0.9976663, 0.9973693, 0.9969939, 0.9965848, 0.9961434,
     0.9956323, 0.9952464, 0.9946782, 0.9941218, 0.9933966, 0.9926888, 0.9919968, 0.9903277},
    {0.9954589, 0.9938576, 0.9917989, 0.9889724, 0.9866190, 0.9823021, 0.9785269, 0.9751601, 0.9706974, 0.9667577, 0.9621007, 0.9579541,
     0.9541924, 0.9490959, 0.9444940, 0.9389141, 0.9325819, 0.9256405, 0.9181533, 0.9101540, 0.9035031, 0.8953134, 0.8865789, 0.8773350,
     0.8668233, 0.8589990, 0.8476493, 0.8367318, 0.8227881, 0.8095131, 0.7968620, 0.7677887}};

// snow asymmetry parameter (:2454-2487)
constexpr double gs_tab[NSPINT][NMBRAD] = {
    {0.859913, 0.867130, 0.873381, 0.878368, 0.881462, 0.884361, 0.885937, 0.886931, 0.887894, 0.888515, 0.889073, 0.889452, 0.889730,
     0.890026, 0.890238, 0.890441, 0.890618, 0.890762, 0.890881, 0.890975, 0.891035, 0.891097, 0.891147, 0.891189, 0.891225, 0.891248,
     0.891277, 0.891299, 0.891323, 0.891340, 0.891356, 0.891386},
    {0.848003, 0.858150, 0.867221, 0.874879, 0.879661, 0.883903, 0.886256, 0.887769, 0.889255, 0.890236, 0.891127, 0.891750, 0.892213,
     0.892723, 0.893099, 0.893474, 0.893816, 0.894123, 0.894397, 0.894645, 0.894822, 0.895020, 0.895212, 0.895399, 0.895601, 0.895745,
     0.895951, 0.896142, 0.896388, 0.896623, 0.896851, 0.897399},
    {0.824415, 0.848445, 0.861714, 0.874036, 0.881299, 0.890184, 0.895393, 0.899072, 0.903285, 0.906588, 0.910152, 0.913100, 0.915621,
     0.918831, 0.921540, 0.924581, 0.927701, 0.930737, 0.933568, 0.936148, 0.937989, 0.939949, 0.941727, 0.943339, 0.944915, 0.945950,
     0.947288, 0.948438, 0.949762, 0.950916, 0.951945, 0.954156}};

// mean optical properties of the ice surface scattering layer (:2496-2499), the drained layer (:2502-2505), the interior (:2508-2511),
// the ice under a pond: its surface scattering layer (:2514-2517) and its interior (:2520-2523); pond water (:2529-2532)
constexpr double ki_ssl_mn[NSPINT] = {1000.1, 1003.7, 7042.0}, wi_ssl_mn[NSPINT] = {0.9999, 0.9963, 0.9088}, gi_ssl_mn[NSPINT] = {0.94, 0.94, 0.94};
constexpr double ki_dl_mn[NSPINT] = {100.2, 107.7, 1309.0}, wi_dl_mn[NSPINT] = {0.9980, 0.9287, 0.0305}, gi_dl_mn[NSPINT] = {0.94, 0.94, 0.94};
constexpr double ki_int_mn[NSPINT] = {20.2, 27.7, 1445.0}, wi_int_mn[NSPINT] = {0.9901, 0.7223, 0.0277}, gi_int_mn[NSPINT] = {0.94, 0.94, 0.94};
constexpr double ki_p_ssl_mn[NSPINT] = {70.2, 77.7, 1309.0}, wi_p_ssl_mn[NSPINT] = {0.9972, 0.9009, 0.0305}, gi_p_ssl_mn[NSPINT] = {0.94, 0.94, 0.94};
constexpr double ki_p_int_mn[NSPINT] = {20.2, 27.7, 1445.0}, wi_p_int_mn[NSPINT] = {0.9901, 0.7223, 0.0277}, gi_p_int_mn[NSPINT] = {0.94, 0.94, 0.94};
constexpr double kw[NSPINT] = {0.20, 12.0, 729.0}, ww[NSPINT] = {0.0, 0.0, 0.0}, gw[NSPINT] = {0.0, 0.0, 0.0};

// Gaussian points and weights of the hemisphere (:3475-3485)
constexpr double gauspt[NGMAX] = {0.9894009, 0.9445750, 0.8656312, 0.7554044, 0.6178762, 0.4580168, 0.2816036, 0.0950125};
constexpr double gauswt[NGMAX] = {0.0271525, 0.0622535, 0.0951585, 0.1246290, 0.1495960, 0.1691565, 0.1826034, 0.1894506};

// scalars.  hi_ssl, hs_ssl (:139-140); hpmin, hp0 (:143-144); hs_min (drivers/auscom/ice_constants.F90:91); Timelt (:65);
// rsnw_fresh, rsnw_nonmelt, rsnw_sig (ice_shortwave.F90:3832-3834); dT_pnd and the pond factor 0.3 (:3932, :3954-3955);
// cp67, cp78, cp01 (:2262-2266); rhoi, fr_max, fr_min, fp_ice, fm_ice, fp_pnd, fm_pnd (:2535-2543: rhoi is this routine's own 917);
// trmin (:3397); refindx, cp063, cp455 (:3431-3433); exp_min = exp(-argmax), argmax = 10 a parameter (:1376, :1383), which the compiler
// folds with correct rounding: the double nearest to e^-10 is 0x3F07CD79B5647C9B = 4.5399929762484854e-05 (exact arithmetic: it lies
// 2.6e-21 from e^-10, its neighbours 4.1e-21 and 9.4e-21).
constexpr double hi_ssl = 0.050, hs_ssl = 0.040, hpmin = 0.005, hp0 = 0.200, hs_min = 1.0e-4, Timelt = 0.0;
constexpr double rsnw_fresh = 100.0, rsnw_nonmelt = 500.0, rsnw_sig = 250.0, dT_pnd = 1.0, pnd_fac = 0.3;
constexpr double cp67 = 0.67, cp78 = 0.78, cp01 = 0.01;
constexpr double rhoi = 917.0, fr_max = 1.00, fr_min = 0.80, fp_ice = 0.15, fm_ice = 0.15, fp_pnd = 2.00, fm_pnd = 0.50;
constexpr double trmin = 0.001, refindx = 1.310, cp063 = 0.063, cp455 = 0.455;
constexpr double exp_min = 4.5399929762484854e-05;

constexpr int NSCALARS = 28;
constexpr double scalars[NSCALARS] = {hi_ssl, hs_ssl, hpmin, hp0, hs_min, Timelt, rsnw_fresh, rsnw_nonmelt, rsnw_sig, dT_pnd, pnd_fac, cp67, cp78,
                                      cp01, rhoi, fr_max, fr_min, fp_ice, fm_ice, fp_pnd, fm_pnd, trmin, refindx, cp063, cp455, exp_min, 30.0, 0.50};
// (the last two: the divisor of hi in the ice surface scattering layer, :2636, and the 0.50 m of the algal layer, :2881)

}  // namespace dedd
}  // namespace evpk
