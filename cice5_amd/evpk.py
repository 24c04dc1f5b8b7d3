"""ctypes binding of libevpk.so (include/evpk.h) -- the same C ABI the Fortran shim binds.

No torch types cross this boundary: arrays are numpy block-layout buffers
(nblocks, ny_block, nx_block), i.e. the reference's (nx_block, ny_block, max_blocks).
There is no CPU fallback: loading fails loudly if the library is missing, and
evpk_create fails if no gfx950 device is usable.
"""
from __future__ import annotations

import ctypes as ct
import os
from typing import Dict, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EVPK_LIB") or os.path.join(_HERE, "libevpk.so")      # (EVPK_LIB: A/B builds of the kernels, scripts/)

c_i32p = ct.POINTER(ct.c_int32)
c_f64p = ct.POINTER(ct.c_double)

UNIQUE_ID_BYTES = 128

GEOM_F64 = ["dxt", "dyt", "dxhy", "dyhx", "cxp", "cyp", "cxm", "cym",
            "tarear", "uarear", "tinyarea", "tarea", "uarea", "fcor"]
STEP_IN_F64 = ["aice", "vice", "vsno", "aice_init", "strairxT", "strairyT", "strax", "stray",
               "uocn", "vocn", "ss_tltx", "ss_tlty", "Cdn_ocn", "strength", "aicen", "vicen", "aice0"]
STATE_OUT_F64 = ["divu", "shear", "rdg_conv", "rdg_shear", "prs_sig", "strintx", "strinty",
                 "strocnx", "strocny", "strocnxT", "strocnyT", "strairx", "strairy",
                 "strtltx", "strtlty", "fm", "tmass", "aiu", "umass", "uvel_init", "vvel_init"]


class Geom(ct.Structure):
    _fields_ = ([("nx_global", ct.c_int32), ("ny_global", ct.c_int32),
                 ("nx_block", ct.c_int32), ("ny_block", ct.c_int32), ("nblocks", ct.c_int32),
                 ("ew_boundary", ct.c_int32), ("ns_boundary", ct.c_int32),
                 ("ilo", c_i32p), ("ihi", c_i32p), ("jlo", c_i32p), ("jhi", c_i32p),
                 ("iglob_lo", c_i32p), ("jglob_lo", c_i32p),
                 ("rank", ct.c_int32), ("nranks", ct.c_int32), ("device", ct.c_int32),
                 ("unique_id", ct.c_void_p)] +
                [(n, c_f64p) for n in GEOM_F64] + [("tmask", c_i32p), ("umask", c_i32p), ("HTN", c_f64p), ("HTE", c_f64p)])


class Params(ct.Structure):
    _fields_ = [("dt", ct.c_double), ("ndte", ct.c_int32), ("revised_evp", ct.c_int32),
                ("revp", ct.c_double), ("ecci", ct.c_double), ("denom1", ct.c_double),
                ("arlx1i", ct.c_double), ("brlx", ct.c_double),
                ("cosw", ct.c_double), ("sinw", ct.c_double),
                ("rhow", ct.c_double), ("rhoi", ct.c_double), ("rhos", ct.c_double), ("gravit", ct.c_double),
                ("a_min", ct.c_double), ("m_min", ct.c_double),
                ("tilt_from_slope", ct.c_int32), ("wind_on_ugrid", ct.c_int32),
                ("kstrength", ct.c_int32), ("krdg_partic", ct.c_int32), ("krdg_redist", ct.c_int32), ("ncat", ct.c_int32),
                ("mu_rdg", ct.c_double), ("Cf", ct.c_double), ("sparse_io", ct.c_int32), ("reserved_", ct.c_int32)]


class StepIn(ct.Structure):
    _fields_ = [(n, c_f64p) for n in STEP_IN_F64]


class State(ct.Structure):
    _fields_ = ([("uvel", c_f64p), ("vvel", c_f64p),
                 ("stressp", c_f64p * 4), ("stressm", c_f64p * 4), ("stress12", c_f64p * 4),
                 ("iceumask", c_i32p)] +
                [(n, c_f64p) for n in STATE_OUT_F64] + [("icetmask", c_i32p), ("strength", c_f64p)])


EAP_HISTORY = ["a11", "a12", "e11", "e12", "e22", "yieldstress11", "yieldstress12", "yieldstress22", "s11", "s12", "s22"]


class EapState(ct.Structure):
    _fields_ = [("a11_c", c_f64p * 4), ("a12_c", c_f64p * 4)] + [(n, c_f64p) for n in EAP_HISTORY]


class Stats(ct.Structure):
    _fields_ = [("icellt", ct.c_int64), ("icellu", ct.c_int64), ("ncell_slab", ct.c_int64),
                ("nstrips", ct.c_int32), ("nstrips_total", ct.c_int32), ("subcycles_done", ct.c_int32),
                ("loop_ms", ct.c_float), ("kernel_ms", ct.c_float), ("kernel_launches", ct.c_int32),
                ("kernel2_ms", ct.c_float), ("kernel2_launches", ct.c_int32),
                ("strip_rows", ct.c_int32), ("strip_rows2", ct.c_int32), ("nstrips2", ct.c_int32),
                ("zone_cols", ct.c_int32), ("zone_exchanges", ct.c_int32), ("zone_bytes", ct.c_int64),
                ("overlap_split", ct.c_int32), ("tile_kernel", ct.c_int32), ("kernel_timed", ct.c_int32),
                ("kernel2_timed", ct.c_int32), ("bound_ms", ct.c_float), ("bound_updates", ct.c_int32),
                ("compact_metrics", ct.c_int32), ("transport", ct.c_int32), ("band_row_exchanges", ct.c_int32),
                ("kernel3_ms", ct.c_float), ("kernel3_launches", ct.c_int32), ("kernel3_timed", ct.c_int32),
                ("strip_rows3", ct.c_int32), ("nstrips3", ct.c_int32),
                ("rccl_ranks", ct.c_int32), ("device", ct.c_int32), ("device_pci", ct.c_int32),
                ("delivery_checked", ct.c_int64), ("delivery_bad", ct.c_int64),
                ("bound_state_rounds", ct.c_int32), ("bound_state_planes", ct.c_int32)]

XP_NAMES = {0: "none", 1: "rccl", 2: "shm relay", 3: "ipc peer-mapped", 4: "self (forced exchange)"}


EXPORTS = ["evpk_get_unique_id", "evpk_create", "evpk_set_params", "evpk_run", "evpk_upload", "evpk_prep",
           "evpk_subcycle", "evpk_finish", "evpk_download", "evpk_sync", "evpk_get_stats", "evpk_destroy",
           "evpk_last_error", "evpk_slab_layout", "evpk_calibrate", "evpk_principal_stress", "evpk_pin_host",
           "evpk_unpin_host", "evpk_connect", "evpk_device_check", "evpk_restart_write", "evpk_restart_read",
           "evpk_transport_upwind", "evpk_remap_init", "evpk_transport_remap", "evpk_transport_remap_state",
           "evpk_eap_init", "evpk_eap_upload", "evpk_eap_download", "evpk_halo_update", "evpk_halo_update_stress",
           "evpk_transport_upwind_state", "evpk_host_alloc", "evpk_host_free", "evpk_host_is_mapped", "evpk_ridge_ice",
           "evpk_cleanup_itd", "evpk_aggregate", "evpk_bound_state", "evpk_step_dynamics", "evpk_linear_itd",
           "evpk_new_ice_lateral_melt", "evpk_step_therm2", "evpk_thermo_vertical", "evpk_step_therm1", "evpk_step_radiation",
           "evpk_prep_radiation", "evpk_step_radiation_dedd", "evpk_dedd_table", "evpk_step_therm1_lvl", "evpk_step_radiation_dedd_lvl"]

REMAP_BAD_DEPARTURE, REMAP_NEGATIVE_MASS = 11, 12        # include/evpk.h
RIDGE_STOP = 13
RIDGE_STOP_REASONS = {1: "aice0 < -puny", 2: "ardg > aicen + puny", 3: "20 ridging iterations exceeded", 4: "|asum - 1| > puny"}
RIDGE_TRACER_FIELDS = ["nt_qsno", "nslyr", "nt_alvl", "nt_vlvl", "nt_apnd", "nt_hpnd", "nt_fbri", "tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo"]
RIDGE_DIAG_2D = ["dardg1dt", "dardg2dt", "dvirdgdt", "opening", "fpond", "fresh", "fhocn"]
RIDGE_DIAG_3D = ["dardg1ndt", "dardg2ndt", "dvirdgndt", "aparticn", "krdgn", "araftn", "vraftn", "aredistn", "vredistn"]


class RidgeTracers(ct.Structure):
    _fields_ = [(n, ct.c_int32) for n in RIDGE_TRACER_FIELDS]


class RidgeDiag(ct.Structure):
    _fields_ = [(n, c_f64p) for n in RIDGE_DIAG_2D + RIDGE_DIAG_3D]


ITD_STOP = 14
ITD_STOP_REASONS = {1: "aggregate ice area out of bounds", 2: "shift_ice: negative daice", 3: "shift_ice: negative dvice",
                    4: "shift_ice: daice > aicen", 5: "shift_ice: dvice > vicen", 6: "zap ice: negative ice area", 7: "zap ice: excess ice area"}
LITD_STOP = 15                                           # reasons 2 .. 5 of ITD_STOP_REASONS
ITD_TRACER_FIELDS = ["nt_Tsfc", "nt_qice", "nilyr", "nt_qsno", "nslyr", "nt_alvl", "nt_apnd", "nt_hpnd", "nt_fbri", "tr_pond_cesm", "tr_pond_lvl",
                     "tr_pond_topo", "tr_brine"]
ITD_CONSTANT_FIELDS = ["Tocnfrz", "ice_ref_salinity", "hs_min", "cp_ice", "Lfresh", "Tmin", "puny"]


class ItdTracers(ct.Structure):
    _fields_ = [(n, ct.c_int32) for n in ITD_TRACER_FIELDS]


class ItdConstants(ct.Structure):
    _fields_ = [(n, ct.c_double) for n in ITD_CONSTANT_FIELDS]


class DynArgs(ct.Structure):
    """evpk_dyn_args (include/evpk.h), member for member"""
    _fields_ = ([("advection", ct.c_int32), ("ridge", ct.c_int32), ("dt", ct.c_double), ("ndtd", ct.c_int32),
                 ("ncat", ct.c_int32), ("ntrcr", ct.c_int32), ("ntrcr_dim", ct.c_int32), ("trcr_depend", c_i32p),
                 ("t", ItdTracers), ("nt_vlvl", ct.c_int32), ("nt_iage", ct.c_int32),
                 ("hin_max", c_f64p), ("k", ItdConstants),
                 ("tr_aero", ct.c_int32), ("nbtrcr", ct.c_int32), ("heat_capacity", ct.c_int32),
                 ("tracer_type", c_i32p), ("depend", c_i32p), ("has_dependents", c_i32p),
                 ("integral_order", ct.c_int32), ("l_dp_midpt", ct.c_int32), ("rhos_lfresh", ct.c_double)] +
                [(n, c_f64p) for n in ("aice0", "aicen", "vicen", "vsnon", "trcrn", "aice", "vice", "vsno", "trcr", "daidtd", "dvidtd", "dagedtd",
                                       "fpond", "fresh", "fsalt", "fhocn")] +
                [("first_ice", c_i32p), ("rdg_conv", c_f64p), ("rdg_shear", c_f64p), ("diag", ct.POINTER(RidgeDiag))])


DYN_STAGES = {1: "transport", 2: "ridge_ice", 3: "cleanup_itd"}


class Therm2Args(ct.Structure):
    """evpk_therm2_args (include/evpk.h), member for member"""
    _fields_ = ([("kitd", ct.c_int32), ("ktherm", ct.c_int32), ("update_ocn_f", ct.c_int32)] +
                [(n, ct.c_double) for n in ("dt", "yday", "hi_min", "hfrazilmin", "phi_init", "dSin0_frazil", "cp_ocn")] +
                [("ncat", ct.c_int32), ("ntrcr", ct.c_int32), ("ntrcr_dim", ct.c_int32), ("trcr_depend", c_i32p),
                 ("t", ItdTracers), ("nt_sice", ct.c_int32), ("nt_iage", ct.c_int32), ("nt_FY", ct.c_int32), ("nt_vlvl", ct.c_int32),
                 ("hin_max", c_f64p), ("k", ItdConstants),
                 ("tr_aero", ct.c_int32), ("nbtrcr", ct.c_int32), ("heat_capacity", ct.c_int32), ("skl_bgc", ct.c_int32)] +
                [(n, c_f64p) for n in ("aicen_init", "vicen_init", "aicen", "vicen", "vsnon", "trcrn", "aice", "aice0", "frain", "frzmlt", "Tf",
                                       "sss", "rside", "salinz", "frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn")] +
                [("first_ice", c_i32p)])


THERM2_STAGES = {1: "linear_itd", 3: "cleanup_itd"}
THERM2_STATE = ["aicen_init", "vicen_init", "aicen", "vicen", "vsnon", "trcrn", "aice", "aice0"]
THERM2_FORCING = ["frain", "frzmlt", "Tf", "sss", "rside", "salinz"]
THERM2_FLUXES = ["frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn"]


THERMO_STOP = 16
THERMO_STOP_REASONS = {1: "zTsn > Tmax", 2: "zTsn < Tmin", 3: "zSin < min_salin - puny", 4: "zTin > Tmlts", 5: "zTin < Tmin",
                       6: "no convergence after nitermax", 7: "ferr > ferrmax"}
THERMO_STATE = ["aicen", "vicen", "vsnon", "trcrn"]
THERMO_FORCING = ["flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "sss", "shcoef", "lhcoef"]
THERMO_INOUT = ["fswsfcn", "fswintn", "Sswabsn", "Iswabsn", "fpond", "mlt_onset", "frz_onset"]
THERMO_OUT = ["flwoutn", "evapn", "freshn", "fsaltn", "fhocnn", "fsensn", "flatn", "fsurfn", "fcondtopn", "melttn", "meltsn", "meltbn",
              "congeln", "snoicen", "dsnown"]


class ThermoArgs(ct.Structure):
    """evpk_thermo_args (include/evpk.h), member for member"""
    _fields_ = ([("dt", ct.c_double), ("yday", ct.c_double)] +
                [(n, ct.c_int32) for n in ("ktherm", "calc_Tsfc", "heat_capacity", "l_brine", "conduct")] + [("min_salin", ct.c_double)] +
                [("ncat", ct.c_int32), ("ntrcr", ct.c_int32), ("ntrcr_dim", ct.c_int32), ("t", ItdTracers), ("nt_sice", ct.c_int32),
                 ("k", ItdConstants)] +
                [(n, c_f64p) for n in THERMO_STATE + THERMO_FORCING + THERMO_INOUT + THERMO_OUT])


THERM1_IN2D = ["aice", "frzmlt", "sst", "Tf", "strocnxT", "strocnyT", "uatm", "vatm", "wind", "zlvl", "frain"]
THERM1_MASKS = ["lmask_n", "lmask_s"]
THERM1_OUT = ["rside", "aice_init", "aicen_init", "vicen_init"]
THERM1_MERGED = ["strairxT", "strairyT", "Cdn_atm_ratio", "fsurf", "fcondtop", "fsens", "flat", "fswabs", "flwout", "evap", "Tref", "Qref", "Uref",
                 "fresh", "fsalt", "fhocn", "fswthru", "meltt", "meltb", "melts", "congel", "snoice"]
THERM1_DIAG = ["strairxn", "strairyn", "Cdn_atm_ratio_n", "Trefn", "Qrefn", "Urefn"]
THERM1_SCALARS = ["chio", "ustar_min", "hi_min", "pndaspect", "rfracmin", "rfracmax"]
THERM1_FLAGS = ["natmiter", "calc_strair", "tr_iage", "tr_FY", "nt_iage", "nt_FY", "formdrag", "highfreq", "atmbndy_constant", "fbot_xfer_Cdn_ocn",
                "tr_aero"]


class Therm1Args(ct.Structure):
    """evpk_therm1_args (include/evpk.h), member for member"""
    _fields_ = ([("tv", ThermoArgs)] + [(n, c_f64p) for n in THERM1_IN2D] + [("fswthrun", c_f64p)] + [(n, c_i32p) for n in THERM1_MASKS] +
                [("Cdn_atm", c_f64p)] + [(n, c_f64p) for n in THERM1_OUT + THERM1_MERGED + THERM1_DIAG] +
                [(n, ct.c_double) for n in THERM1_SCALARS] + [(n, ct.c_int32) for n in THERM1_FLAGS])


RAD_FLAGS = ["shortwave_dEdd", "calc_Tsfc", "heat_capacity", "albedo_constant"]
RAD_SCALARS = ["albicev", "albicei", "albsnowv", "albsnowi", "ahmax", "snowpatch", "albocn", "awtvdr", "awtidr", "awtvdf", "awtidf"]
RAD_STATE = ["aicen", "vicen", "vsnon", "trcrn"]
RAD_FORCING = ["swvdr", "swvdf", "swidr", "swidf", "ocn_albedo2D"]
RAD_OUT = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun"]       # (nb, ncat, ny, nx)
RAD_OUT_LAYERS = ["Sswabsn", "Iswabsn", "fswpenln"]                                  # (nb, ncat, nslyr | nilyr | nilyr + 1, ny, nx)
RAD_OUT2D = ["coszen", "alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "scale_factor"]
# the reference's namelist defaults (source/ice_init.F90:305-321); albocn of ice_constants.F90
RAD_DEFAULTS = dict(albicev=0.78, albicei=0.36, albsnowv=0.98, albsnowi=0.70, ahmax=0.3, snowpatch=0.02, albocn=0.06,
                    awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282, awtidf=0.36218)
PREP_RAD_IN = ["aice", "aicen", "swvdr", "swvdf", "swidr", "swidf", "alvdr_ai", "alvdf_ai", "alidr_ai", "alidf_ai"]
PREP_RAD_INOUT = ["scale_factor", "fswsfcn", "fswintn", "fswthrun", "fswpenln", "Sswabsn", "Iswabsn"]


class RadArgs(ct.Structure):
    """evpk_rad_args (include/evpk.h), member for member"""
    _fields_ = ([(n, ct.c_int32) for n in RAD_FLAGS] + [("ncat", ct.c_int32), ("ntrcr", ct.c_int32), ("ntrcr_dim", ct.c_int32),
                                                       ("t", ItdTracers), ("puny", ct.c_double)] +
                [(n, ct.c_double) for n in RAD_SCALARS] + [(n, c_f64p) for n in RAD_STATE + RAD_FORCING + RAD_OUT + RAD_OUT_LAYERS + RAD_OUT2D])


class PrepRadArgs(ct.Structure):
    """evpk_prep_rad_args (include/evpk.h), member for member"""
    _fields_ = ([("ncat", ct.c_int32), ("nilyr", ct.c_int32), ("nslyr", ct.c_int32), ("puny", ct.c_double)] +
                [(n, c_f64p) for n in PREP_RAD_IN + PREP_RAD_INOUT] + [("fswfac", c_f64p)])


DEDD_FLAGS = ["calc_Tsfc", "heat_capacity", "tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo", "tr_aero"]
DEDD_SCALARS = ["R_ice", "R_pnd", "R_snw", "dT_mlt", "rsnw_mlt", "kalg", "hs0", "pndaspect", "awtvdr", "awtidr", "awtvdf", "awtidf"]
DEDD_STATE = ["aicen", "vicen", "vsnon", "trcrn"]
DEDD_FORCING = ["swvdr", "swvdf", "swidr", "swidf"]
DEDD_OUT = RAD_OUT + ["albpndn", "apeffn", "snowfracn"]                              # (nb, ncat, ny, nx)
DEDD_OUT_LAYERS = RAD_OUT_LAYERS
DEDD_OUT2D = [n for n in RAD_OUT2D if n != "coszen"] + ["albpnd", "apeff_ai"]        # coszen is in / out
# the reference's namelist defaults (source/ice_init.F90:289-304: R_ice, R_pnd, R_snw, dT_mlt, rsnw_mlt, kalg, hs0, pndaspect; :318-321 awt*)
DEDD_DEFAULTS = dict(R_ice=0.0, R_pnd=0.0, R_snw=1.5, dT_mlt=1.5, rsnw_mlt=1500.0, kalg=0.60, hs0=0.03, pndaspect=0.8,
                     awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282, awtidf=0.36218)
DEDD_TABLES = dict(rsnw_tab=32, Qs_tab=96, ws_tab=96, gs_tab=96, ki_ssl_mn=3, wi_ssl_mn=3, gi_ssl_mn=3, ki_dl_mn=3, wi_dl_mn=3, gi_dl_mn=3,
                   ki_int_mn=3, wi_int_mn=3, gi_int_mn=3, ki_p_ssl_mn=3, wi_p_ssl_mn=3, gi_p_ssl_mn=3, ki_p_int_mn=3, wi_p_int_mn=3,
                   gi_p_int_mn=3, kw=3, ww=3, gw=3, gauspt=8, gauswt=8, scalars=28)
DEDD_SCALAR_NAMES = ["hi_ssl", "hs_ssl", "hpmin", "hp0", "hs_min", "Timelt", "rsnw_fresh", "rsnw_nonmelt", "rsnw_sig", "dT_pnd", "pnd_fac",
                     "cp67", "cp78", "cp01", "rhoi", "fr_max", "fr_min", "fp_ice", "fm_ice", "fp_pnd", "fm_pnd", "trmin", "refindx", "cp063",
                     "cp455", "exp_min", "ssl_div", "alg_depth"]


class DeddArgs(ct.Structure):
    """evpk_dedd_args (include/evpk.h), member for member"""
    _fields_ = ([(n, ct.c_int32) for n in DEDD_FLAGS] + [("ncat", ct.c_int32), ("ntrcr", ct.c_int32), ("ntrcr_dim", ct.c_int32),
                                                        ("t", ItdTracers), ("puny", ct.c_double)] +
                [(n, ct.c_double) for n in DEDD_SCALARS] + [(n, c_f64p) for n in DEDD_STATE + DEDD_FORCING + ["coszen"] + RAD_OUT + RAD_OUT_LAYERS] +
                [(n, c_f64p) for n in RAD_OUT2D if n != "coszen"] + [(n, c_f64p) for n in ("albpndn", "apeffn", "snowfracn", "albpnd", "apeff_ai")])


POND_LVL_ARRAYS = ["dhsn", "ffracn", "Tair", "fsnow"]                                 # (nb, ncat, ny, nx) x 2, (nb, ny, nx) x 2
POND_LVL_SCALARS = ["dpscale", "hs1", "dt"]
POND_LVL_FLAGS = ["frzpnd", "nt_ipnd", "linitonly"]
FRZPND = {"cesm": 0, "hlid": 1}
# the values every ice_in the reference ships sets (input_templates/*/ice_in); the defaults of source/ice_init.F90:299-301 are 0.03, 1, 'cesm'
POND_LVL_DEFAULTS = dict(hs1=0.03, dpscale=1.0e-3, frzpnd="hlid")


class PondLvlArgs(ct.Structure):
    """evpk_pond_lvl_args (include/evpk.h), member for member"""
    _fields_ = ([(n, c_f64p) for n in POND_LVL_ARRAYS] + [(n, ct.c_double) for n in POND_LVL_SCALARS] + [(n, ct.c_int32) for n in POND_LVL_FLAGS])


def pond_lvl_args(ponds, tracers, dt=0.0, linitonly=False):
    """PondLvlArgs from a dict with any of POND_LVL_ARRAYS, dpscale, hs1 and frzpnd ('cesm' / 'hlid' or 0 / 1); nt_ipnd from tracers"""
    p = PondLvlArgs()
    for n in POND_LVL_ARRAYS:
        setattr(p, n, _p64(ponds.get(n)))
    p.dpscale, p.hs1, p.dt = float(ponds.get("dpscale", POND_LVL_DEFAULTS["dpscale"])), float(ponds.get("hs1", POND_LVL_DEFAULTS["hs1"])), float(dt)
    frz = ponds.get("frzpnd", POND_LVL_DEFAULTS["frzpnd"])
    p.frzpnd, p.nt_ipnd, p.linitonly = int(FRZPND.get(frz, frz)), int(tracers.get("nt_ipnd", 0)), int(bool(linitonly))
    return p


def dedd_table(name: str) -> np.ndarray:
    """evpk_dedd_table: one table of csrc/evpk_dedd_tables.h as the library holds it (the snow tables [band][radius], flattened)"""
    out = np.zeros(DEDD_TABLES[name])
    if lib().evpk_dedd_table(name.encode(), _p64(out), out.size):
        raise EvpkError(f"evpk_dedd_table: no table {name!r} of {out.size} numbers")
    return out


def remap_tracer_tables(trcr_depend):
    """tracer_type, depend, has_dependents of transport_remap as init_transport builds them from trcr_depend
    (ice_transport_driver.F90:90-118): hice and hsno first (type 1, no parent); a tracer of the area is type 1, one that hangs on a
    tracer that itself hangs on ice or snow volume is type 3, every other type 2; depend is trcr_depend itself (2 + the parent's
    tracer index is its position behind hice, hsno)."""
    dep = [int(d) for d in trcr_depend]
    depend = [0, 0] + dep
    ttype = [1, 1]
    for d in dep:
        ttype.append(1 if d == 0 else (3 if d > 2 and dep[d - 3] > 0 else 2))
    has = [0] * len(depend)
    for nt, d in enumerate(depend):
        if d > 0:
            if d > nt + 1:
                raise EvpkError(f"remap transport: tracer {nt + 1} depends on tracer {d}: must have nt2 > nt1")
            has[d - 1] = 1
    return (np.array(ttype, dtype=np.int32), np.array(depend, dtype=np.int32), np.array(has, dtype=np.int32))


_lib = None


class EvpkError(RuntimeError):
    pass


def lib():
    """Load libevpk.so; raises if it has not been built (python __graft_entry__.py / make -C cice5_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EvpkError(f"{LIB_PATH} not found: build it with `make -C cice5_amd/csrc` "
                            "(there is no CPU fallback for the EVP kernels)")
        L = ct.CDLL(LIB_PATH)
        ctxp = ct.c_void_p
        L.evpk_get_unique_id.argtypes = [ct.c_void_p]
        L.evpk_create.argtypes = [ct.POINTER(Geom), ct.POINTER(ctxp)]
        L.evpk_set_params.argtypes = [ctxp, ct.POINTER(Params)]
        L.evpk_run.argtypes = [ctxp, ct.POINTER(StepIn), ct.POINTER(State)]
        L.evpk_upload.argtypes = [ctxp, ct.POINTER(StepIn), ct.POINTER(State)]
        L.evpk_prep.argtypes = [ctxp]
        L.evpk_subcycle.argtypes = [ctxp, ct.c_int32]
        L.evpk_finish.argtypes = [ctxp]
        L.evpk_download.argtypes = [ctxp, ct.POINTER(State)]
        L.evpk_sync.argtypes = [ctxp]
        L.evpk_get_stats.argtypes = [ctxp, ct.POINTER(Stats)]
        L.evpk_destroy.argtypes = [ctxp]
        L.evpk_calibrate.argtypes = [ctxp, ct.c_int32]
        L.evpk_principal_stress.argtypes = [ctxp, c_f64p, c_f64p]
        L.evpk_last_error.argtypes = [ctxp]
        L.evpk_last_error.restype = ct.c_char_p
        L.evpk_slab_layout.argtypes = [ct.c_int32] * 6 + [c_i32p]
        L.evpk_pin_host.argtypes = [ct.c_void_p, ct.c_size_t]
        L.evpk_unpin_host.argtypes = [ct.c_void_p]
        L.evpk_host_alloc.argtypes = [ct.c_size_t, ct.POINTER(ct.c_void_p)]
        L.evpk_host_free.argtypes = [ct.c_void_p]
        L.evpk_host_is_mapped.argtypes = [ct.c_void_p, ct.c_size_t]
        L.evpk_connect.argtypes = [ctxp, ct.c_void_p]
        L.evpk_device_check.argtypes = [ct.c_int32]
        L.evpk_transport_upwind.argtypes = [ctxp, ct.c_double, ct.c_int32, c_f64p]
        L.evpk_transport_upwind_state.argtypes = ([ctxp, ct.c_double] + [ct.c_int32] * 3 + [c_i32p] + [ct.c_int32] * 7 + [ct.c_double] + [c_f64p] * 5)
        L.evpk_halo_update.argtypes = [ctxp, c_f64p, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_double]
        L.evpk_halo_update_stress.argtypes = [ctxp, c_f64p, c_f64p]
        L.evpk_remap_init.argtypes = [ctxp, c_f64p, c_f64p, c_f64p]
        L.evpk_transport_remap.argtypes = [ctxp, ct.c_double, ct.c_int32, ct.c_int32, c_f64p, c_f64p, c_i32p, c_i32p, c_i32p,
                                           ct.c_int32, ct.c_int32, ct.c_int32]
        L.evpk_transport_remap_state.argtypes = ([ctxp, ct.c_double] + [ct.c_int32] * 5 + [ct.c_double] + [c_f64p] * 5 + [c_i32p] * 3 +
                                                 [ct.c_int32] * 2)
        L.evpk_eap_init.argtypes = [ctxp, ct.c_int32, ct.c_int32, ct.c_int32] + [c_f64p] * 6
        L.evpk_eap_upload.argtypes = [ctxp, ct.POINTER(EapState)]
        L.evpk_eap_download.argtypes = [ctxp, ct.POINTER(EapState)]
        L.evpk_ridge_ice.argtypes = ([ctxp, ct.c_double] + [ct.c_int32] * 4 + [c_i32p, ct.POINTER(RidgeTracers)] + [c_f64p] * 8 +
                                     [ct.POINTER(RidgeDiag), c_i32p])
        L.evpk_cleanup_itd.argtypes = ([ctxp, ct.c_double] + [ct.c_int32] * 3 + [c_i32p, ct.POINTER(ItdTracers), c_f64p, ct.POINTER(ItdConstants)] +
                                       [ct.c_int32] * 3 + [c_f64p] * 10 + [c_i32p, c_i32p])
        L.evpk_linear_itd.argtypes = ([ctxp] + [ct.c_int32] * 3 + [c_i32p, ct.POINTER(ItdTracers), c_f64p, ct.c_double, ct.POINTER(ItdConstants)] +
                                      [c_f64p] * 9 + [c_i32p])
        L.evpk_aggregate.argtypes = ([ctxp, ct.c_double] + [ct.c_int32] * 4 + [c_i32p, ct.POINTER(ItdTracers), ct.c_int32, ct.c_double] +
                                     [c_f64p] * 12)
        L.evpk_bound_state.argtypes = [ctxp] + [ct.c_int32] * 3 + [c_f64p] * 4
        L.evpk_step_dynamics.argtypes = [ctxp, ct.POINTER(DynArgs), c_i32p]
        L.evpk_new_ice_lateral_melt.argtypes = [ctxp, ct.POINTER(Therm2Args)]
        L.evpk_step_therm2.argtypes = [ctxp, ct.POINTER(Therm2Args), c_i32p]
        L.evpk_thermo_vertical.argtypes = [ctxp, ct.POINTER(ThermoArgs), c_i32p]
        L.evpk_step_therm1.argtypes = [ctxp, ct.POINTER(Therm1Args), c_i32p]
        L.evpk_step_radiation.argtypes = [ctxp, ct.POINTER(RadArgs)]
        L.evpk_prep_radiation.argtypes = [ctxp, ct.POINTER(PrepRadArgs)]
        L.evpk_step_radiation_dedd.argtypes = [ctxp, ct.POINTER(DeddArgs)]
        L.evpk_dedd_table.argtypes = [ct.c_char_p, c_f64p, ct.c_int32]
        L.evpk_step_therm1_lvl.argtypes = [ctxp, ct.POINTER(Therm1Args), ct.POINTER(PondLvlArgs), c_i32p]
        L.evpk_step_radiation_dedd_lvl.argtypes = [ctxp, ct.POINTER(DeddArgs), ct.POINTER(PondLvlArgs)]
        L.evpk_restart_write.argtypes = [ctxp, ct.c_char_p, ct.c_int32, ct.c_int32]
        L.evpk_restart_read.argtypes = [ctxp, ct.c_char_p, ct.c_int64, ct.c_int32]
        for n in EXPORTS:
            if n != "evpk_last_error":
                getattr(L, n).restype = ct.c_int
        _lib = L
    return _lib


def pin_host(a: np.ndarray) -> bool:
    """Page-lock a host array for in-place transfers (evpk_pin_host); False if the runtime refuses."""
    assert a.flags["C_CONTIGUOUS"]
    return lib().evpk_pin_host(ct.c_void_p(a.ctypes.data), a.nbytes) == 0


def unpin_host(a: np.ndarray) -> bool:
    return lib().evpk_unpin_host(ct.c_void_p(a.ctypes.data)) == 0


class _HostBlock:
    """one evpk_host_alloc allocation; freed when the last array on it is gone"""

    def __init__(self, nbytes: int):
        self.ptr = ct.c_void_p()
        if lib().evpk_host_alloc(max(nbytes, 8), ct.byref(self.ptr)) != 0:
            raise EvpkError("evpk_host_alloc failed (no device, or out of page-locked memory)")
        self.nbytes = nbytes

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.evpk_host_free(self.ptr)
            self.ptr = ct.c_void_p()


class _HostMem:
    """array-interface owner of a _HostBlock: np.asarray(_HostMem) is a view whose base keeps the block alive"""

    def __init__(self, blk, shape, dt):
        self.blk = blk
        self.__array_interface__ = {"data": (blk.ptr.value, False), "shape": tuple(int(v) for v in shape), "typestr": dt.str, "version": 3}


def host_empty(shape, dtype=np.float64) -> np.ndarray:
    """An array on page-locked memory that the DRIVER allocated and pinned (evpk_host_alloc = hipHostMalloc, mapped into the
    device address space): the library reads / writes it in place, and its pages cannot move under a kernel.  Freed with the
    last view of it."""
    dt = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    return np.asarray(_HostMem(_HostBlock(int(np.prod(shape)) * dt.itemsize), shape, dt))


def host_copy(a: np.ndarray) -> np.ndarray:
    b = host_empty(a.shape, a.dtype)
    b[...] = a
    return b


def experimental() -> bool:
    """always False: the build that held the measured-and-rejected pair kernels was retired.  Kept because test modules
    of earlier revisions ask it when they are collected."""
    return False


def host_is_mapped(a: np.ndarray) -> bool:
    return lib().evpk_host_is_mapped(ct.c_void_p(a.ctypes.data), a.nbytes) == 1


def _p64(a: Optional[np.ndarray]):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):          # a torch tensor in device (or page-locked) memory: the library takes the pointer as it is
        if str(a.dtype) != "torch.float64" or not a.is_contiguous():
            raise TypeError("expected a contiguous float64 tensor")
        return ct.cast(a.data_ptr(), c_f64p)
    if a.dtype != np.float64 or not a.flags.c_contiguous:
        raise TypeError("expected a C-contiguous float64 block array")
    return a.ctypes.data_as(c_f64p)


def _p32(a: Optional[np.ndarray]):
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        if str(a.dtype) != "torch.int32" or not a.is_contiguous():
            raise TypeError("expected a contiguous int32 tensor")
        return ct.cast(a.data_ptr(), c_i32p)
    if a.dtype != np.int32 or not a.flags.c_contiguous:
        raise TypeError("expected a C-contiguous int32 block array")
    return a.ctypes.data_as(c_i32p)


def get_unique_id() -> bytes:
    buf = ct.create_string_buffer(UNIQUE_ID_BYTES)
    if lib().evpk_get_unique_id(buf):
        raise EvpkError("evpk_get_unique_id failed")
    return buf.raw


def device_check(device: int) -> Optional[str]:
    """None if `device` is a usable gfx950 part, else the reason (evpk_device_check)."""
    L = lib()
    if L.evpk_device_check(int(device)):
        return L.evpk_last_error(None).decode()
    return None


def slab_layout(nx_global, nranks, rank, ew_boundary, i0, i1):
    out = (ct.c_int32 * 5)()
    if lib().evpk_slab_layout(nx_global, nranks, rank, ew_boundary, i0, i1, out):
        raise EvpkError("evpk_slab_layout: bad arguments")
    return dict(west=out[0], east=out[1], i0=out[2], i1=out[3], wmax=out[4])


class Context:
    """Owns one evpk_ctx (one GPU, one rank)."""

    def __init__(self, decomp, fields: Dict[str, np.ndarray], device: int = 0, unique_id: Optional[bytes] = None,
                 defer_connect: bool = False):
        """defer_connect (nprocs > 1): evpk_create without a unique id -- nothing collective happens until connect(),
        so the host can first agree across ranks that every create succeeded."""
        L = lib()
        self._L = L
        self._ctx = ct.c_void_p()
        ga = decomp.geom_arrays()
        g = Geom()
        g.nx_global, g.ny_global = decomp.nx_global, decomp.ny_global
        g.nx_block, g.ny_block, g.nblocks = decomp.nx_block, decomp.ny_block, decomp.nblocks
        g.ew_boundary, g.ns_boundary = decomp.ew_boundary, decomp.ns_boundary
        for n in ("ilo", "ihi", "jlo", "jhi", "iglob_lo", "jglob_lo"):
            setattr(g, n, _p32(ga[n]))
        g.rank, g.nranks, g.device = decomp.rank, decomp.nprocs, device
        if defer_connect:
            unique_id = None
        self._uid = ct.create_string_buffer(unique_id, UNIQUE_ID_BYTES) if unique_id is not None else None
        g.unique_id = ct.cast(self._uid, ct.c_void_p) if self._uid is not None else None
        for n in GEOM_F64:
            setattr(g, n, _p64(fields[n]))
        g.tmask, g.umask = _p32(fields["tmask"]), _p32(fields["umask"])
        g.HTN, g.HTE = _p64(fields.get("HTN")), _p64(fields.get("HTE"))      # optional
        if L.evpk_create(ct.byref(g), ct.byref(self._ctx)):
            raise EvpkError("evpk_create: " + L.evpk_last_error(None).decode())
        self.decomp = decomp
        self.device_strength = False     # True: evpk_step_in.strength = NULL, ice_strength runs on the device

    def _chk(self, rc, what):
        if rc:
            e = EvpkError(f"{what}: " + self._L.evpk_last_error(self._ctx).decode())
            e.rc = int(rc)
            raise e

    def connect(self, unique_id: bytes):
        """evpk_connect: the collective half of the start (communicator / peer mapping)."""
        self._uid = ct.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        self._chk(self._L.evpk_connect(self._ctx, ct.cast(self._uid, ct.c_void_p)), "evpk_connect")

    def set_params(self, p: Params):
        self._chk(self._L.evpk_set_params(self._ctx, ct.byref(p)), "evpk_set_params")

    def _step_in(self, f) -> StepIn:
        si = StepIn()
        for n in STEP_IN_F64:
            setattr(si, n, _p64(f.get(n)))
        if self.device_strength:            # strength == NULL: ice_strength runs on the device
            si.strength = None
        return si

    def _state(self, f) -> State:
        """evpk_state from the arrays present in `f` (an absent output is a NULL pointer: skipped by evpk_download)"""
        st = State()
        st.uvel, st.vvel = _p64(f.get("uvel")), _p64(f.get("vvel"))
        for k in ("stressp", "stressm", "stress12"):
            setattr(st, k, (c_f64p * 4)(*[_p64(f.get(f"{k}_{c}")) for c in (1, 2, 3, 4)]))
        st.iceumask = _p32(f.get("iceumask"))
        for n in STATE_OUT_F64:
            setattr(st, n, _p64(f.get(n)))
        st.icetmask = _p32(f.get("icetmask"))
        st.strength = _p64(f.get("strength"))        # comes back with its ghost cells halo-updated (ice_dyn_evp.F90:311-312)
        return st

    def run(self, f):
        si, st = self._step_in(f), self._state(f)
        self._chk(self._L.evpk_run(self._ctx, ct.byref(si), ct.byref(st)), "evpk_run")

    def upload(self, f):
        si, st = self._step_in(f), self._state(f)
        self._chk(self._L.evpk_upload(self._ctx, ct.byref(si), ct.byref(st)), "evpk_upload")

    def upload_inputs(self, f):
        """inputs only; the prognostic state stays resident on the device (evpk_upload with state == NULL)"""
        si = self._step_in(f)
        self._chk(self._L.evpk_upload(self._ctx, ct.byref(si), None), "evpk_upload")

    def prep(self):
        self._chk(self._L.evpk_prep(self._ctx), "evpk_prep")

    def subcycle(self, nsub: int):
        self._chk(self._L.evpk_subcycle(self._ctx, int(nsub)), "evpk_subcycle")

    def finish(self):
        self._chk(self._L.evpk_finish(self._ctx), "evpk_finish")

    def download(self, f):
        st = self._state(f)
        self._chk(self._L.evpk_download(self._ctx, ct.byref(st)), "evpk_download")

    def sync(self):
        self._chk(self._L.evpk_sync(self._ctx), "evpk_sync")

    def stats(self) -> Stats:
        s = Stats()
        self._chk(self._L.evpk_get_stats(self._ctx, ct.byref(s)), "evpk_get_stats")
        return s

    def principal_stress(self, sig1: np.ndarray, sig2: np.ndarray):
        self._chk(self._L.evpk_principal_stress(self._ctx, _p64(sig1), _p64(sig2)), "evpk_principal_stress")

    def halo_update(self, a: np.ndarray, field_loc: int, field_type: int, fill: float = 0.0):
        """evpk_halo_update (ice_HaloUpdate): a is (nblocks, ny_block, nx_block) or (nblocks, nz, ny_block, nx_block), in place"""
        assert a.ndim in (3, 4)
        self._chk(self._L.evpk_halo_update(self._ctx, _p64(a), 0 if a.ndim == 3 else int(a.shape[1]), int(field_loc), int(field_type),
                                           float(fill)), "evpk_halo_update")

    def halo_update_stress(self, a1: np.ndarray, a2: np.ndarray):
        """evpk_halo_update_stress (ice_HaloUpdate_stress(array1 = a1, array2 = a2, centre, scalar)): a1 in place"""
        self._chk(self._L.evpk_halo_update_stress(self._ctx, _p64(a1), _p64(a2)), "evpk_halo_update_stress")

    def transport_upwind(self, dt: float, works: np.ndarray):
        """evpk_transport_upwind: works is (nblocks, narr, ny_block, nx_block), advected in place"""
        assert works.ndim == 4
        self._chk(self._L.evpk_transport_upwind(self._ctx, float(dt), int(works.shape[1]), _p64(works)), "evpk_transport_upwind")

    def transport_upwind_state(self, dt: float, aice0, aicen, vicen, vsnon, trcrn, ntrcr: int, trcr_depend, nt_Tsfc=1, nt_alvl=0, nt_apnd=0,
                               nt_fbri=0, ponds=(0, 0, 0), Tocnfrz=-1.8):
        """evpk_transport_upwind_state: aice0 (nb, ny, nx), aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), in place"""
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        self._chk(self._L.evpk_transport_upwind_state(self._ctx, float(dt), int(aicen.shape[1]), int(ntrcr), int(trcrn.shape[2]), _p32(dep),
                                                      int(nt_Tsfc), int(nt_alvl), int(nt_apnd), int(nt_fbri), *[int(p) for p in ponds], float(Tocnfrz),
                                                      _p64(aice0), _p64(aicen), _p64(vicen), _p64(vsnon), _p64(trcrn)), "evpk_transport_upwind_state")

    def remap_init(self, dxu: np.ndarray, dyu: np.ndarray, hm: np.ndarray):
        """evpk_remap_init: the grid arrays of horizontal_remap beyond the geometry's (block arrays)"""
        self._chk(self._L.evpk_remap_init(self._ctx, _p64(dxu), _p64(dyu), _p64(hm)), "evpk_remap_init")

    def transport_remap(self, dt: float, mm: np.ndarray, tm: Optional[np.ndarray], tracer_type, depend, has_dependents,
                        integral_order: int = 3, l_dp_midpt: bool = True, l_fixed_area: bool = False) -> int:
        """evpk_transport_remap: mm (nblocks, ncat+1, ny_block, nx_block), tm (nblocks, ncat, ntrace, ny_block, nx_block) in
        place.  Returns 0, REMAP_BAD_DEPARTURE or REMAP_NEGATIVE_MASS (the reference's two l_stop cases); raises otherwise."""
        assert mm.ndim == 4 and mm.flags["C_CONTIGUOUS"]
        ncat = mm.shape[1] - 1
        ntrace = 0 if tm is None else int(tm.shape[2])
        if ntrace:
            assert tm.ndim == 5 and tm.shape[1] == ncat and tm.flags["C_CONTIGUOUS"]
        tt, dp, hd = (np.ascontiguousarray(a, dtype=np.int32) for a in (tracer_type, depend, has_dependents))
        rc = self._L.evpk_transport_remap(self._ctx, float(dt), ncat, ntrace, _p64(mm), _p64(tm) if ntrace else None,
                                          _p32(tt) if ntrace else None, _p32(dp) if ntrace else None, _p32(hd) if ntrace else None,
                                          int(integral_order), int(l_dp_midpt), int(l_fixed_area))
        if rc not in (0, REMAP_BAD_DEPARTURE, REMAP_NEGATIVE_MASS):
            self._chk(rc, "evpk_transport_remap")
        return int(rc)

    def transport_remap_state(self, dt: float, aice0, aicen, vicen, vsnon, trcrn, ntrcr: int, nt_qsno: int, nslyr: int, rhos_lfresh: float,
                              tracer_type, depend, has_dependents, integral_order: int = 3, l_dp_midpt: bool = True) -> int:
        """evpk_transport_remap_state: aice0 (nblocks, ny, nx), aicen / vicen / vsnon (nblocks, ncat, ny, nx), trcrn (nblocks, ncat, ntrcr_dim,
        ny, nx) in place -- state_to_tracers, horizontal_remap, tracers_to_state and bound_state on the device"""
        ncat, ntrcr_dim = aicen.shape[1], (trcrn.shape[2] if trcrn is not None else 0)
        tt, dp, hd = (np.ascontiguousarray(a, dtype=np.int32) for a in (tracer_type, depend, has_dependents))
        rc = self._L.evpk_transport_remap_state(self._ctx, float(dt), ncat, int(ntrcr), ntrcr_dim, int(nt_qsno), int(nslyr), float(rhos_lfresh),
                                                _p64(aice0), _p64(aicen), _p64(vicen), _p64(vsnon), _p64(trcrn), _p32(tt), _p32(dp), _p32(hd),
                                                int(integral_order), int(l_dp_midpt))
        if rc not in (0, REMAP_BAD_DEPARTURE, REMAP_NEGATIVE_MASS):
            self._chk(rc, "evpk_transport_remap_state")
        return int(rc)

    def ridge_ice(self, dt: float, ndtd: int, aice0, aicen, vicen, vsnon, trcrn, ntrcr: int, trcr_depend, tracers, hin_max,
                  rdg_conv=None, rdg_shear=None, diag=None):
        """evpk_ridge_ice (ridge_ice, ice_mechred.F90:101-746): aice0 (nb, ny, nx), aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn
        (nb, ncat, ntrcr_dim, ny, nx) in place on the listed cells (physical cells with tmask).  tracers: dict of RIDGE_TRACER_FIELDS
        (absent = 0); hin_max: (ncat + 1,); rdg_conv / rdg_shear None: the planes the last evp / eap left on the device; diag: dict of
        the arrays of RIDGE_DIAG_2D (nb, ny, nx) / RIDGE_DIAG_3D (nb, ncat, ny, nx) that are wanted, or None.
        Returns None, or (reason, block, i, j) for the reference's l_stop cases (RIDGE_STOP_REASONS); raises on a refusal."""
        ncat = int(aicen.shape[1])
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        hin = np.ascontiguousarray(hin_max, dtype=np.float64)
        assert hin.shape == (ncat + 1,)
        rt = RidgeTracers(**{k: int(tracers.get(k, 0)) for k in RIDGE_TRACER_FIELDS})
        rd = None
        if diag is not None:
            rd = RidgeDiag()
            for k in RIDGE_DIAG_2D + RIDGE_DIAG_3D:
                setattr(rd, k, _p64(diag.get(k)))
        stop = np.zeros(4, dtype=np.int32)
        ntrcr_dim = int(trcrn.shape[2]) if trcrn is not None else 0
        rc = self._L.evpk_ridge_ice(self._ctx, float(dt), int(ndtd), ncat, int(ntrcr), ntrcr_dim, _p32(dep) if ntrcr else None, ct.byref(rt),
                                    _p64(hin), _p64(rdg_conv), _p64(rdg_shear), _p64(aice0), _p64(aicen), _p64(vicen), _p64(vsnon),
                                    _p64(trcrn), ct.byref(rd) if rd is not None else None, _p32(stop))
        if rc == RIDGE_STOP:
            return tuple(int(v) for v in stop)
        self._chk(rc, "evpk_ridge_ice")
        return None

    def cleanup_itd(self, dt: float, aicen, vicen, vsnon, trcrn, aice0, aice, ntrcr: int, trcr_depend, tracers, hin_max, constants=None,
                    fluxes=None, first_ice=None, tr_aero=False, nbtrcr=0, heat_capacity=True):
        """evpk_cleanup_itd (cleanup_itd, ice_itd.F90:1514-1769; dt = dt * ndtd of step_ridge): aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn
        (nb, ncat, ntrcr_dim, ny, nx) in place on the physical ocean cells, aice0 / aice (nb, ny, nx) on every cell.  tracers: dict of
        ITD_TRACER_FIELDS (absent = 0); hin_max: (ncat + 1,); constants: dict of ITD_CONSTANT_FIELDS (absent: cice5_amd.constants);
        fluxes: dict with any of fpond, fresh, fsalt, fhocn (nb, ny, nx), incremented; first_ice: int32 (nb, ncat, ny, nx) or None.
        Returns None, or (reason, block, i, j) for the reference's l_stop cases (ITD_STOP_REASONS); raises on a refusal."""
        from . import constants as C
        ncat = int(aicen.shape[1])
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        hin = np.ascontiguousarray(hin_max, dtype=np.float64)
        assert hin.shape == (ncat + 1,)
        it = ItdTracers(**{k: int(tracers.get(k, 0)) for k in ITD_TRACER_FIELDS})
        ik = ItdConstants(**{k: float((constants or {}).get(k, getattr(C, k))) for k in ITD_CONSTANT_FIELDS})
        fl = fluxes or {}
        stop = np.zeros(4, dtype=np.int32)
        ntrcr_dim = int(trcrn.shape[2]) if trcrn is not None else 0
        rc = self._L.evpk_cleanup_itd(self._ctx, float(dt), ncat, int(ntrcr), ntrcr_dim, _p32(dep) if ntrcr else None, ct.byref(it), _p64(hin),
                                      ct.byref(ik), int(bool(tr_aero)), int(nbtrcr), int(bool(heat_capacity)), _p64(aicen), _p64(vicen),
                                      _p64(vsnon), _p64(trcrn), _p64(aice0), _p64(aice), _p64(fl.get("fpond")), _p64(fl.get("fresh")),
                                      _p64(fl.get("fsalt")), _p64(fl.get("fhocn")), _p32(first_ice), _p32(stop))
        if rc == ITD_STOP:
            return tuple(int(v) for v in stop)
        self._chk(rc, "evpk_cleanup_itd")
        return None

    def linear_itd(self, aicen_init, vicen_init, aicen, vicen, vsnon, trcrn, aice, aice0, ntrcr: int, trcr_depend, tracers, hin_max,
                   hi_min: float, constants=None, fpond=None):
        """evpk_linear_itd (linear_itd, ice_therm_itd.F90:69-859, as step_therm2 calls it): aicen_init / vicen_init (nb, ncat, ny, nx) in;
        aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx) in place on the physical ocean cells, aice / aice0
        (nb, ny, nx) on every cell; fpond (nb, ny, nx) in / out, needed with tr_pond_topo only.  tracers, hin_max, constants as for
        cleanup_itd; hin_max[ncat] is taken as 999.9 inside the call.
        Returns None, or (reason, block, i, j) for shift_ice's l_stop cases (ITD_STOP_REASONS 2 .. 5); raises on a refusal."""
        from . import constants as C
        ncat = int(aicen.shape[1])
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        hin = np.ascontiguousarray(hin_max, dtype=np.float64)
        assert hin.shape == (ncat + 1,)
        it = ItdTracers(**{k: int(tracers.get(k, 0)) for k in ITD_TRACER_FIELDS})
        ik = ItdConstants(**{k: float((constants or {}).get(k, getattr(C, k))) for k in ITD_CONSTANT_FIELDS})
        stop = np.zeros(4, dtype=np.int32)
        ntrcr_dim = int(trcrn.shape[2]) if trcrn is not None else 0
        rc = self._L.evpk_linear_itd(self._ctx, ncat, int(ntrcr), ntrcr_dim, _p32(dep) if ntrcr else None, ct.byref(it), _p64(hin), float(hi_min),
                                     ct.byref(ik), _p64(aicen_init), _p64(vicen_init), _p64(aicen), _p64(vicen), _p64(vsnon), _p64(trcrn),
                                     _p64(aice), _p64(aice0), _p64(fpond), _p32(stop))
        if rc == LITD_STOP:
            return tuple(int(v) for v in stop)
        self._chk(rc, "evpk_linear_itd")
        return None

    def aggregate(self, dt: float, aicen, vicen, vsnon, trcrn, aice, vice, vsno, aice0, trcr, ntrcr: int, trcr_depend, tracers, bound=False,
                  daidtd=None, dvidtd=None, dagedtd=None, Tocnfrz=None):
        """evpk_aggregate: bound_state (bound = True: the ghost cells of aicen, vicen, vsnon, trcrn are rewritten), aggregate
        (ice_itd.F90:246-458) on every cell -- aice, vice, vsno, aice0 (nb, ny, nx), trcr (nb, ntrcr_dim, ny, nx) -- and the tendencies of
        step_dynamics on physical cells: daidtd, dvidtd, dagedtd in / out (on entry the pre-dynamics aice, vice, age), each may be None;
        tracers: dict of ITD_TRACER_FIELDS plus nt_iage."""
        from . import constants as C
        ncat = int(aicen.shape[1])
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        it = ItdTracers(**{k: int(tracers.get(k, 0)) for k in ITD_TRACER_FIELDS})
        ntrcr_dim = int(trcrn.shape[2]) if trcrn is not None else 0
        assert trcr is None or trcr.shape[1] == ntrcr_dim
        rc = self._L.evpk_aggregate(self._ctx, float(dt), int(bool(bound)), ncat, int(ntrcr), ntrcr_dim, _p32(dep) if ntrcr else None, ct.byref(it),
                                    int(tracers.get("nt_iage", 0)), float(C.Tocnfrz if Tocnfrz is None else Tocnfrz), _p64(aicen), _p64(vicen),
                                    _p64(vsnon), _p64(trcrn), _p64(aice), _p64(vice), _p64(vsno), _p64(aice0), _p64(trcr), _p64(daidtd),
                                    _p64(dvidtd), _p64(dagedtd))
        self._chk(rc, "evpk_aggregate")

    def bound_state(self, aicen, vicen, vsnon, trcrn, ntrcr: int):
        """evpk_bound_state (bound_state, ice_state.F90:173-238): the ghost cells of aicen / vicen / vsnon (nb, ncat, ny, nx) and of tracers
        1 .. ntrcr of trcrn (nb, ncat, ntrcr_dim, ny, nx; None when ntrcr == 0) in place, one launch.  On x-slab ranks the call is
        collective: one packed message per partner rank, then one launch (stats().bound_state_rounds / bound_state_planes); so are
        aggregate(bound=True) and step_dynamics"""
        ntrcr_dim = int(trcrn.shape[2]) if trcrn is not None else 0
        self._chk(self._L.evpk_bound_state(self._ctx, int(aicen.shape[1]), int(ntrcr), ntrcr_dim, _p64(aicen), _p64(vicen), _p64(vsnon),
                                           _p64(trcrn)), "evpk_bound_state")

    def step_dynamics(self, dt: float, ndtd: int, aice0, aicen, vicen, vsnon, trcrn, aice, vice, vsno, trcr, ntrcr: int, trcr_depend, tracers,
                      hin_max, advection=0, ridge=True, constants=None, fluxes=None, first_ice=None, daidtd=None, dvidtd=None, dagedtd=None,
                      rdg_conv=None, rdg_shear=None, diag=None, tracer_type=None, depend=None, has_dependents=None, integral_order=3,
                      l_dp_midpt=True, rhos_lfresh=None, tr_aero=False, nbtrcr=0, heat_capacity=True):
        """evpk_step_dynamics: everything of step_dynamics behind evp / eap in one call, the arrays staged once -- advection (0 none, 1
        transport_upwind, 2 transport_remap; also 'none' / 'upwind' / 'remap'), ridge_ice (ridge), cleanup_itd(dt * ndtd),
        bound_state and aggregate with the tendencies.  Arrays and keywords as for ridge_ice / cleanup_itd / aggregate; tracers: dict of
        ITD_TRACER_FIELDS plus nt_vlvl, nt_iage; tracer_type / depend / has_dependents default to remap_tracer_tables(trcr_depend),
        rhos_lfresh to rhos * Lfresh of cice5_amd.constants.
        Returns None, or (code, stage, reason, block, i, j) when a stage stops (code: REMAP_BAD_DEPARTURE, REMAP_NEGATIVE_MASS,
        RIDGE_STOP, ITD_STOP; stage: DYN_STAGES); raises on a refusal, which leaves every array untouched."""
        from . import constants as C
        adv = {"none": 0, "upwind": 1, "remap": 2}.get(advection, advection)
        a = DynArgs()
        a.advection, a.ridge, a.dt, a.ndtd = int(adv), int(ridge), float(dt), int(ndtd)
        a.ncat = int(aicen.shape[1]) if aicen is not None else 0
        a.ntrcr, a.ntrcr_dim = int(ntrcr), (int(trcrn.shape[2]) if trcrn is not None else 0)
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        a.trcr_depend = _p32(dep) if ntrcr else None
        a.t = ItdTracers(**{k: int(tracers.get(k, 0)) for k in ITD_TRACER_FIELDS})
        a.nt_vlvl, a.nt_iage = int(tracers.get("nt_vlvl", 0)), int(tracers.get("nt_iage", 0))
        hin = np.ascontiguousarray(hin_max, dtype=np.float64)
        assert hin.shape == (a.ncat + 1,) or aicen is None
        a.hin_max = _p64(hin)
        a.k = ItdConstants(**{k: float((constants or {}).get(k, getattr(C, k))) for k in ITD_CONSTANT_FIELDS})
        a.tr_aero, a.nbtrcr, a.heat_capacity = int(bool(tr_aero)), int(nbtrcr), int(bool(heat_capacity))
        keep = [dep, hin]
        if adv == 2:
            if tracer_type is None:
                tracer_type, depend, has_dependents = remap_tracer_tables(dep[:int(ntrcr)])
            tt, dp, hd = (np.ascontiguousarray(v, dtype=np.int32) for v in (tracer_type, depend, has_dependents))
            keep += [tt, dp, hd]
            a.tracer_type, a.depend, a.has_dependents = _p32(tt), _p32(dp), _p32(hd)
        a.integral_order, a.l_dp_midpt = int(integral_order), int(bool(l_dp_midpt))
        a.rhos_lfresh = float(C.rhos * C.Lfresh if rhos_lfresh is None else rhos_lfresh)
        fl = fluxes or {}
        for n, v in (("aice0", aice0), ("aicen", aicen), ("vicen", vicen), ("vsnon", vsnon), ("trcrn", trcrn), ("aice", aice), ("vice", vice),
                     ("vsno", vsno), ("trcr", trcr), ("daidtd", daidtd), ("dvidtd", dvidtd), ("dagedtd", dagedtd), ("fpond", fl.get("fpond")),
                     ("fresh", fl.get("fresh")), ("fsalt", fl.get("fsalt")), ("fhocn", fl.get("fhocn")), ("rdg_conv", rdg_conv),
                     ("rdg_shear", rdg_shear)):
            setattr(a, n, _p64(v))
        a.first_ice = _p32(first_ice)
        rd = None
        if diag is not None:
            rd = RidgeDiag()
            for k in RIDGE_DIAG_2D + RIDGE_DIAG_3D:
                setattr(rd, k, _p64(diag.get(k)))
            a.diag = ct.pointer(rd)
        stop = np.zeros(5, dtype=np.int32)
        rc = self._L.evpk_step_dynamics(self._ctx, ct.byref(a), _p32(stop))
        del keep
        if rc in (REMAP_BAD_DEPARTURE, REMAP_NEGATIVE_MASS, RIDGE_STOP, ITD_STOP):
            return (int(rc),) + tuple(int(v) for v in stop)
        self._chk(rc, "evpk_step_dynamics")
        return None

    @staticmethod
    def _itd_header(a, state, ntrcr, tracers):
        """a.ncat and a.ntrcr_dim from the shapes of state's aicen and trcrn, a.ntrcr, and a.t from the tracers dict"""
        aicen, trcrn = state.get("aicen"), state.get("trcrn")
        a.ncat = int(aicen.shape[1]) if aicen is not None else 0
        a.ntrcr, a.ntrcr_dim = int(ntrcr), (int(trcrn.shape[2]) if trcrn is not None else 0)
        a.t = ItdTracers(**{k: int(tracers.get(k, 0)) for k in ITD_TRACER_FIELDS})

    @staticmethod
    def _pointers(a, *tables):
        """a.<name> = the float64 array src[name], or NULL where src has none, for every (names, src) of tables"""
        for names, src in tables:
            for n in names:
                setattr(a, n, _p64(src.get(n)))

    @staticmethod
    def _scalars(a, who, scalars, names, defaults):
        """a.<name> for every name of names, from the keyword arguments scalars or else from defaults"""
        unknown = set(scalars) - set(names)
        if unknown:
            raise TypeError(f"{who}: unknown arguments {sorted(unknown)}")
        for n in names:
            setattr(a, n, float(scalars.get(n, defaults[n])))

    def _thermo_args(self, a, dt, state, forcing, inout, out, ntrcr, tracers, yday, conduct, min_salin, constants, ktherm, calc_Tsfc,
                     heat_capacity, l_brine):
        """fills the ThermoArgs a in place: thermo_vertical's own, or the tv of step_therm1's Therm1Args"""
        from . import constants as C
        a.dt, a.yday, a.min_salin = float(dt), float(yday), float(min_salin)
        a.ktherm, a.calc_Tsfc, a.heat_capacity, a.l_brine = int(ktherm), int(bool(calc_Tsfc)), int(bool(heat_capacity)), int(bool(l_brine))
        a.conduct = int({"MU71": 0, "bubbly": 1}.get(conduct, conduct))
        self._itd_header(a, state, ntrcr, tracers)
        a.nt_sice = int(tracers.get("nt_sice", 0))
        a.k = ItdConstants(**{k: float((constants or {}).get(k, getattr(C, k))) for k in ITD_CONSTANT_FIELDS})
        self._pointers(a, (THERMO_STATE, state), (THERMO_FORCING, forcing), (THERMO_INOUT, inout), (THERMO_OUT, out))

    def _therm2_args(self, dt, state, forcing, fluxes, ntrcr, trcr_depend, tracers, hin_max, kitd, ktherm, update_ocn_f, yday, hi_min, hfrazilmin,
                     phi_init, dSin0_frazil, cp_ocn, constants, first_ice, tr_aero, nbtrcr, heat_capacity, skl_bgc):
        from . import constants as C
        a = Therm2Args()
        a.kitd, a.ktherm, a.update_ocn_f = int(kitd), int(ktherm), int(bool(update_ocn_f))
        a.dt, a.yday, a.hi_min, a.hfrazilmin = float(dt), float(yday), float(hi_min), float(hfrazilmin)
        a.phi_init, a.dSin0_frazil, a.cp_ocn = float(phi_init), float(dSin0_frazil), float(C.cp_ocn if cp_ocn is None else cp_ocn)
        self._itd_header(a, state, ntrcr, tracers)
        dep = np.ascontiguousarray(trcr_depend, dtype=np.int32)
        a.trcr_depend = _p32(dep) if ntrcr else None
        a.nt_sice, a.nt_iage, a.nt_FY, a.nt_vlvl = (int(tracers.get(k, 0)) for k in ("nt_sice", "nt_iage", "nt_FY", "nt_vlvl"))
        hin = np.ascontiguousarray(hin_max, dtype=np.float64)
        assert hin.shape == (a.ncat + 1,) or state.get("aicen") is None
        a.hin_max = _p64(hin)
        a.k = ItdConstants(**{k: float((constants or {}).get(k, getattr(C, k))) for k in ITD_CONSTANT_FIELDS})
        a.tr_aero, a.nbtrcr, a.heat_capacity, a.skl_bgc = int(bool(tr_aero)), int(nbtrcr), int(bool(heat_capacity)), int(bool(skl_bgc))
        self._pointers(a, (THERM2_STATE, state), (THERM2_FORCING, forcing), (THERM2_FLUXES, fluxes))
        a.first_ice = _p32(first_ice)
        return a, [dep, hin]

    def new_ice_lateral_melt(self, dt: float, state, forcing, fluxes, ntrcr: int, trcr_depend, tracers, hin_max, ktherm=1, update_ocn_f=False,
                             yday=0.0, hfrazilmin=0.05, phi_init=0.75, dSin0_frazil=3.0, cp_ocn=None, constants=None, tr_aero=False, nbtrcr=0,
                             heat_capacity=True, skl_bgc=False):
        """evpk_new_ice_lateral_melt: add_new_ice, lateral_melt and (ncat = 1) reduce_area of step_therm2 in one launch, on the aice / aice0
        given.  state: dict of THERM2_STATE -- aicen_init / vicen_init / aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim,
        ny, nx), aice / aice0 (nb, ny, nx); forcing: dict of THERM2_FORCING (nb, ny, nx), salinz (nb, nilyr + 1, ny, nx), frain not read;
        fluxes: dict of THERM2_FLUXES (nb, ny, nx), frz_onset may be absent, fpond unless tr_pond_topo.  tracers: dict of
        ITD_TRACER_FIELDS plus nt_sice, nt_iage, nt_FY, nt_vlvl.  Raises on a refusal, which leaves every array untouched."""
        a, keep = self._therm2_args(dt, state, forcing, fluxes, ntrcr, trcr_depend, tracers, hin_max, 0, ktherm, update_ocn_f, yday, 0.0, hfrazilmin,
                                    phi_init, dSin0_frazil, cp_ocn, constants, None, tr_aero, nbtrcr, heat_capacity, skl_bgc)
        rc = self._L.evpk_new_ice_lateral_melt(self._ctx, ct.byref(a))
        del keep
        self._chk(rc, "evpk_new_ice_lateral_melt")

    def step_therm2(self, dt: float, state, forcing, fluxes, ntrcr: int, trcr_depend, tracers, hin_max, kitd=1, ktherm=1, update_ocn_f=False,
                    yday=0.0, hi_min=0.01, hfrazilmin=0.05, phi_init=0.75, dSin0_frazil=3.0, cp_ocn=None, constants=None, first_ice=None,
                    tr_aero=False, nbtrcr=0, heat_capacity=True, skl_bgc=False):
        """evpk_step_therm2: step_therm2 in one call, the arrays staged once -- the frain line, aggregate_area, linear_itd (kitd = 1),
        add_new_ice, lateral_melt, cleanup_itd(dt).  Arguments as for new_ice_lateral_melt; forcing may hold frain; first_ice: int32
        (nb, ncat, ny, nx) or None.
        Returns None, or (code, stage, reason, block, i, j) when a stage stops (code: LITD_STOP, ITD_STOP; stage: THERM2_STAGES); raises on
        a refusal, which leaves every array untouched."""
        a, keep = self._therm2_args(dt, state, forcing, fluxes, ntrcr, trcr_depend, tracers, hin_max, kitd, ktherm, update_ocn_f, yday, hi_min,
                                    hfrazilmin, phi_init, dSin0_frazil, cp_ocn, constants, first_ice, tr_aero, nbtrcr, heat_capacity, skl_bgc)
        stop = np.zeros(5, dtype=np.int32)
        rc = self._L.evpk_step_therm2(self._ctx, ct.byref(a), _p32(stop))
        del keep
        if rc in (LITD_STOP, ITD_STOP):
            return (int(rc),) + tuple(int(v) for v in stop)
        self._chk(rc, "evpk_step_therm2")
        return None

    def step_therm1(self, dt: float, state, forcing, inout, out, merged, ntrcr: int, tracers, yday=0.0, conduct=0, min_salin=0.1, constants=None,
                    ktherm=1, calc_Tsfc=True, heat_capacity=True, l_brine=True, chio=0.006, ustar_min=0.0005, natmiter=5, calc_strair=True,
                    hi_min=0.01, pndaspect=0.8, rfracmin=0.15, rfracmax=1.0, formdrag=False, highfreq=False, atmbndy="default",
                    fbot_xfer_type="constant", tr_aero=False, ponds=None):
        """evpk_step_therm1: step_therm1 in one call -- frzmlt_bottom_lateral, atmo_boundary_layer, increment_age, update_FYarea,
        thermo_vertical (BL99), compute_ponds_cesm, merge_fluxes -- on arrays staged once.  state, inout as for thermo_vertical; forcing:
        dict of THERMO_FORCING (fbot, Tbot, shcoef, lhcoef may be absent: given, they receive what the call computed) plus THERM1_IN2D
        (nb, ny, nx; frain only with tr_pond_cesm), fswthrun (nb, ncat, ny, nx), lmask_n / lmask_s (int32 (nb, ny, nx), only with tr_FY);
        out: dict of THERMO_OUT plus THERM1_OUT (rside, aice_init (nb, ny, nx); aicen_init, vicen_init (nb, ncat, ny, nx)) and, where
        wanted, THERM1_DIAG (nb, ncat, ny, nx); merged: dict of Cdn_atm and THERM1_MERGED (nb, ny, nx), in / out.  tracers: dict of
        ITD_TRACER_FIELDS plus nt_sice, tr_iage, tr_FY, nt_iage, nt_FY.
        Returns None, or (reason, block, category, i, j) as thermo_vertical; raises on a refusal, which leaves every array untouched.
        (ponds: see step_therm1_lvl, which passes it.)"""
        a = Therm1Args()
        self._thermo_args(a.tv, dt, state, forcing, inout, out, ntrcr, tracers, yday, conduct, min_salin, constants, ktherm, calc_Tsfc,
                          heat_capacity, l_brine)
        self._pointers(a, (THERM1_IN2D + ["fswthrun"], forcing), (THERM1_OUT + THERM1_DIAG, out), (["Cdn_atm"] + THERM1_MERGED, merged))
        for n in THERM1_MASKS:
            setattr(a, n, _p32(forcing.get(n)))
        a.chio, a.ustar_min, a.hi_min, a.pndaspect = float(chio), float(ustar_min), float(hi_min), float(pndaspect)
        a.rfracmin, a.rfracmax = float(rfracmin), float(rfracmax)
        a.natmiter, a.calc_strair = int(natmiter), int(bool(calc_strair))
        a.tr_iage, a.tr_FY, a.nt_iage, a.nt_FY = (int(tracers.get(k, 0)) for k in ("tr_iage", "tr_FY", "nt_iage", "nt_FY"))
        a.formdrag, a.highfreq, a.tr_aero = int(bool(formdrag)), int(bool(highfreq)), int(bool(tr_aero))
        a.atmbndy_constant, a.fbot_xfer_Cdn_ocn = int(atmbndy == "constant"), int(fbot_xfer_type == "Cdn_ocn")
        stop = np.zeros(5, dtype=np.int32)
        if ponds is None:
            rc, who = self._L.evpk_step_therm1(self._ctx, ct.byref(a), _p32(stop)), "evpk_step_therm1"
        else:
            p = pond_lvl_args(ponds, tracers)
            rc, who = self._L.evpk_step_therm1_lvl(self._ctx, ct.byref(a), ct.byref(p), _p32(stop)), "evpk_step_therm1_lvl"
        if rc == THERMO_STOP:
            return tuple(int(v) for v in stop)
        self._chk(rc, who)
        return None

    def step_therm1_lvl(self, dt: float, state, forcing, inout, out, merged, ponds, ntrcr: int, tracers, **kw):
        """evpk_step_therm1_lvl: step_therm1 under tr_pond_lvl -- everything step_therm1 does, with compute_ponds_lvl in the place of
        compute_ponds_cesm.  Arguments as for step_therm1 (forcing must hold frain; tracers has tr_pond_lvl = 1, nt_alvl, nt_apnd, nt_hpnd
        and nt_ipnd); ponds: dict of dhsn (nb, ncat, ny, nx; read), ffracn (nb, ncat, ny, nx; written on every cell), Tair (nb, ny, nx) and,
        where they differ from POND_LVL_DEFAULTS, dpscale and frzpnd ('cesm' / 'hlid').  Returns and raises as step_therm1."""
        return self.step_therm1(dt, state, forcing, inout, out, merged, ntrcr, tracers, ponds=ponds, **kw)

    def step_radiation(self, state, forcing, out, ntrcr: int, tracers, albedo_type="default", shortwave="default", calc_Tsfc=True,
                       heat_capacity=True, puny=1.0e-11, **scalars):
        """evpk_step_radiation: step_radiation (shortwave_ccsm3) and the albedo lines of coupling_prep in one launch.  state: dict of
        RAD_STATE -- aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), read only; forcing: dict of RAD_FORCING
        (nb, ny, nx), ocn_albedo2D may be absent (then the scalar albocn is the ocean albedo of every cell); out: dict of RAD_OUT (nb, ncat,
        ny, nx), RAD_OUT_LAYERS (Sswabsn (nb, ncat, nslyr, ny, nx), Iswabsn (nb, ncat, nilyr, ny, nx), fswpenln (nb, ncat, nilyr + 1, ny, nx),
        which may be absent) and RAD_OUT2D (nb, ny, nx), all written on every cell.  tracers: dict with nt_Tsfc, nilyr, nslyr; scalars: any
        of RAD_SCALARS (the rest take RAD_DEFAULTS).  Raises on a refusal, which leaves every array untouched."""
        a = RadArgs()
        a.shortwave_dEdd, a.calc_Tsfc, a.heat_capacity = int(shortwave == "dEdd"), int(bool(calc_Tsfc)), int(bool(heat_capacity))
        a.albedo_constant = int(albedo_type == "constant")
        self._itd_header(a, state, ntrcr, tracers)
        a.puny = float(puny)
        self._scalars(a, "step_radiation", scalars, RAD_SCALARS, RAD_DEFAULTS)
        self._pointers(a, (RAD_STATE, state), (RAD_FORCING, forcing), (RAD_OUT + RAD_OUT_LAYERS + RAD_OUT2D, out))
        self._chk(self._L.evpk_step_radiation(self._ctx, ct.byref(a)), "evpk_step_radiation")

    def step_radiation_dedd(self, state, forcing, coszen, out, ntrcr: int, tracers, calc_Tsfc=True, heat_capacity=True, tr_aero=False,
                            puny=1.0e-11, ponds=None, dt=0.0, linitonly=False, **scalars):
        """evpk_step_radiation_dedd: step_radiation on its Delta-Eddington branch (run_dEdd) and the albedo lines of coupling_prep in one
        launch.  state: dict of DEDD_STATE -- aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), read only;
        forcing: dict of DEDD_FORCING (nb, ny, nx); coszen (nb, ny, nx): what compute_coszen made, in / out -- max(puny, coszen) is stored
        on the listed, lit cells; out: dict of DEDD_OUT (nb, ncat, ny, nx), DEDD_OUT_LAYERS (Sswabsn (nb, ncat, nslyr, ny, nx), Iswabsn
        (nb, ncat, nilyr, ny, nx), fswpenln (nb, ncat, nilyr + 1, ny, nx), which may be absent) and DEDD_OUT2D (nb, ny, nx), all written
        on every cell.  tracers: dict with nt_Tsfc, nilyr, nslyr and, with tr_pond_cesm, nt_apnd, nt_hpnd; scalars: any of DEDD_SCALARS
        (the rest take DEDD_DEFAULTS, the reference's namelist defaults).  Raises on a refusal, which leaves every array untouched.
        (ponds, dt, linitonly: see step_radiation_dedd_lvl, which passes them.)"""
        a = DeddArgs()
        a.calc_Tsfc, a.heat_capacity, a.tr_aero = int(bool(calc_Tsfc)), int(bool(heat_capacity)), int(bool(tr_aero))
        a.tr_pond_cesm, a.tr_pond_lvl, a.tr_pond_topo = (int(bool(tracers.get(k, 0))) for k in ("tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo"))
        self._itd_header(a, state, ntrcr, tracers)
        a.puny = float(puny)
        self._scalars(a, "step_radiation_dedd", scalars, DEDD_SCALARS, DEDD_DEFAULTS)
        self._pointers(a, (DEDD_STATE, state), (DEDD_FORCING, forcing), (DEDD_OUT + DEDD_OUT_LAYERS + DEDD_OUT2D, out))
        a.coszen = _p64(coszen)
        if ponds is None:
            self._chk(self._L.evpk_step_radiation_dedd(self._ctx, ct.byref(a)), "evpk_step_radiation_dedd")
        else:
            p = pond_lvl_args(ponds, tracers, dt, linitonly)
            self._chk(self._L.evpk_step_radiation_dedd_lvl(self._ctx, ct.byref(a), ct.byref(p)), "evpk_step_radiation_dedd_lvl")

    def step_radiation_dedd_lvl(self, dt: float, state, forcing, coszen, out, ponds, ntrcr: int, tracers, linitonly=False, **kw):
        """evpk_step_radiation_dedd_lvl: step_radiation_dedd under tr_pond_lvl -- the level-ice block of run_dEdd sets the ponds and the
        snow the radiation sees.  Arguments as for step_radiation_dedd (tracers has tr_pond_lvl = 1, nt_alvl, nt_apnd, nt_hpnd, nt_ipnd);
        dt: the time step of fsnow dt; ponds: dict of dhsn (nb, ncat, ny, nx; in / out on the listed cells), ffracn (nb, ncat, ny, nx; read),
        fsnow (nb, ny, nx) and, where it differs from POND_LVL_DEFAULTS, hs1; linitonly: run_dEdd's initonly, which leaves dhsn as it is."""
        return self.step_radiation_dedd(state, forcing, coszen, out, ntrcr, tracers, ponds=ponds, dt=dt, linitonly=linitonly, **kw)

    def prep_radiation(self, arrays, nilyr: int, nslyr: int, puny=1.0e-11):
        """evpk_prep_radiation: prep_radiation in one launch (an AusCOM host does not call it).  arrays: dict of PREP_RAD_IN (aice and the
        eight 2-D planes (nb, ny, nx), aicen (nb, ncat, ny, nx)), PREP_RAD_INOUT (rescaled in place on the listed cells; fswpenln may be
        absent) and fswfac (nb, ny, nx; written on the physical cells).  Raises on a refusal, which leaves every array untouched."""
        a = PrepRadArgs()
        aicen = arrays.get("aicen")
        a.ncat = int(aicen.shape[1]) if aicen is not None else 0
        a.nilyr, a.nslyr, a.puny = int(nilyr), int(nslyr), float(puny)
        self._pointers(a, (PREP_RAD_IN + PREP_RAD_INOUT + ["fswfac"], arrays))
        self._chk(self._L.evpk_prep_radiation(self._ctx, ct.byref(a)), "evpk_prep_radiation")

    def thermo_vertical(self, dt: float, state, forcing, inout, out, ntrcr: int, tracers, yday=0.0, conduct=0, min_salin=0.1, constants=None,
                        ktherm=1, calc_Tsfc=True, heat_capacity=True, l_brine=True):
        """evpk_thermo_vertical: thermo_vertical (BL99) for every category of every block in one launch.  state: dict of THERMO_STATE --
        aicen / vicen / vsnon (nb, ncat, ny, nx), trcrn (nb, ncat, ntrcr_dim, ny, nx), in place on the listed cells; forcing: dict of
        THERMO_FORCING, (nb, ny, nx) and shcoef / lhcoef (nb, ncat, ny, nx); inout: dict of THERMO_INOUT -- fswsfcn / fswintn (nb, ncat, ny,
        nx), Sswabsn (nb, ncat, nslyr, ny, nx), Iswabsn (nb, ncat, nilyr, ny, nx), fpond (needed with tr_pond_topo only), mlt_onset,
        frz_onset (nb, ny, nx); out: dict of THERMO_OUT (nb, ncat, ny, nx), written on every cell.  tracers: dict of ITD_TRACER_FIELDS plus
        nt_sice; conduct: 0 / 'MU71' or 1 / 'bubbly'.
        Returns None, or (reason, block, category, i, j) for the reference's l_stop cases (THERMO_STOP_REASONS); raises on a refusal,
        which leaves every array untouched."""
        a = ThermoArgs()
        self._thermo_args(a, dt, state, forcing, inout, out, ntrcr, tracers, yday, conduct, min_salin, constants, ktherm, calc_Tsfc, heat_capacity,
                          l_brine)
        stop = np.zeros(5, dtype=np.int32)
        rc = self._L.evpk_thermo_vertical(self._ctx, ct.byref(a), _p32(stop))
        if rc == THERMO_STOP:
            return tuple(int(v) for v in stop)
        self._chk(rc, "evpk_thermo_vertical")
        return None

    def eap_init(self, tables):
        """evpk_eap_init: the six lookup tables of init_eap, each [na_yield][ny_yield][nx_yield]; the context then runs eap(dt)"""
        na, ny, nx = tables[0].shape
        assert all(t.shape == (na, ny, nx) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"] for t in tables) and len(tables) == 6
        self._chk(self._L.evpk_eap_init(self._ctx, nx, ny, na, *[_p64(t) for t in tables]), "evpk_eap_init")

    def _eap_state(self, f, names) -> EapState:
        st = EapState()
        st.a11_c = (c_f64p * 4)(*[_p64(f.get(f"a11_{c}") if f"a11_{c}" in names else None) for c in (1, 2, 3, 4)])
        st.a12_c = (c_f64p * 4)(*[_p64(f.get(f"a12_{c}") if f"a12_{c}" in names else None) for c in (1, 2, 3, 4)])
        for n in EAP_HISTORY:
            setattr(st, n, _p64(f.get(n) if n in names else None))
        return st

    def eap_upload(self, f):
        """evpk_eap_upload: a11_1..4, a12_1..4 of `f` (those present)"""
        st = self._eap_state(f, [n for n in f if n[:4] in ("a11_", "a12_")])
        self._chk(self._L.evpk_eap_upload(self._ctx, ct.byref(st)), "evpk_eap_upload")

    def eap_download(self, f, names=None):
        """evpk_eap_download: the structure tensor and the EAP history fields present in `f` (or only `names`)"""
        st = self._eap_state(f, list(f) if names is None else names)
        self._chk(self._L.evpk_eap_download(self._ctx, ct.byref(st)), "evpk_eap_download")

    def restart_write(self, path: str, append: bool = False, big_endian: bool = True):
        self._chk(self._L.evpk_restart_write(self._ctx, path.encode(), int(append), int(big_endian)), "evpk_restart_write")

    def restart_read(self, path: str, byte_offset: int = 0, big_endian: bool = True):
        self._chk(self._L.evpk_restart_read(self._ctx, path.encode(), int(byte_offset), int(big_endian)), "evpk_restart_read")

    def calibrate(self, nrep: int = 3):
        self._chk(self._L.evpk_calibrate(self._ctx, int(nrep)), "evpk_calibrate")

    def close(self):
        if self._ctx:
            self._L.evpk_destroy(self._ctx)
            self._ctx = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
