"""Makes tests/golden/ref_sw_*.npz from the reference's own shortwave_ccsm3 (compute_albedos, constant_albedos, absorbed_solar), run_dEdd
(compute_coszen, shortwave_dEdd_set_snow / _set_pond, shortwave_dEdd, compute_dEdd, solution_dEdd, its tr_pond_cesm / tr_pond_lvl / no-pond
blocks) and compute_ponds_lvl (brine_permeability): oracle/_ref/<build>/ref_shortwave (oracle/ref/Makefile, target shortwave +
oracle/ref/ref_shortwave.F90, built by __graft_entry__.build() where the reference is present).  Inputs come from radvec.rad_input,
deddvec.dedd_input and pondlvlvec.pondlvl_input; only the reference's OUTPUTS are stored, on the physical ocean cells in (block, j, i)
order, the category / layer axes last:

  ref_sw_c_*   (mode C: step_radiation's zeroing, shortwave_ccsm3, the albedo lines of coupling_prep)     radvec.WRITTEN
  ref_sw_d_*   (mode D: the zeroing, compute_coszen, run_dEdd with initonly absent, the same lines)       deddvec.WRITTEN, coszen, and
               coszen_in: what compute_coszen returned, before shortwave_dEdd raises it to puny on the lit cells it lists -- the value
               the restatement and the device are fed, since compute_coszen stays with the caller on the device; exp_min
  ref_sw_v_*   (mode D under tr_pond_lvl, initonly absent or .true.)                                      the same and dhsn
  ref_sw_p_*   (mode P: compute_ponds_lvl per category on the state and fluxes nptherm1s.step leaves)     apnd, hpnd, ipnd, ffracn

The albedo aggregation and scale_factor (the 2-D arrays) are the DRIVER'S restatement of coupling_prep on the reference's category
arrays: that part, step_radiation's call order and its zeroing stay formally unpinned.

dEdd coszen: the reference computes coszen itself, from tlat, tlon, yday and sec.  Per ocean cell coszen_place() draws tlat on the
declination's side of the equator and solves the hour-angle formula (ice_orbital.F90:130-132) for tlon, with the delta the driver reports
for (yday, sec), so that compute_coszen lands within rounding of deddvec's target; main() asserts from the RETURNED coszen that the three
sun classes of deddvec.SUN are populated in every record.

The reference's AusCOM build fixes its constants at compile time; run_reference() asserts every one the restatements carry against the
driver's header.  Stated departure of the device (include/evpk.h): its cell lists require tmask where the reference's ask aicen > puny
alone; check_departures() asserts what makes that harmless -- no ice on a physical land cell -- and the comparison stays on the physical
ocean cells.

main() asserts coverage from the restatements' info counts (coverage()), prints per record in which arrays the restatement on libm
differs from the reference, and prints the distance of the restatement on the device's fixed-algorithm exp / atan (PORTS) from the
reference per array, relative to the array's largest magnitude in the record: SPREAD_MEASURED below is the largest over the family, and
tests/test_shortwave_ref_gpu.py allows four times as much.

    python -m tests.golden.make_ref_shortwave
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import deddvec as dv         # noqa: E402
from tests.golden import itdvec as iv          # noqa: E402
from tests.golden import pondlvlvec as pv      # noqa: E402
from tests.golden import radvec as rv          # noqa: E402
from tests.golden import refrun                # noqa: E402
from tests.golden import refvec                # noqa: E402
from tests.golden.refrun import Writer, bits, on_cells, padded, same          # noqa: E402,F401
from tests.golden.refvec import hash01, seed_of                               # noqa: E402

BIG, SMALL = "g26x18_b8x5", "g24x16_b6x4"
LAYERS = {"plain": (4, 1), "deep": (7, 2)}
IDX = ("nt_Tsfc", "nt_qice", "nt_sice", "nt_alvl", "nt_apnd", "nt_hpnd", "nt_ipnd", "tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo")
C3D = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun", "albpndn", "apeffn", "snowfracn"]
LAYER_KEYS = ["Sswabsn", "Iswabsn", "fswpenln"]
AGG = ["alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "albpnd", "apeff_ai", "scale_factor"]
C_KEYS = rv.WRITTEN
D_KEYS = dv.WRITTEN + ["coszen"]
V_KEYS = D_KEYS + ["dhsn"]
P_KEYS = ["apnd", "hpnd", "ipnd", "ffracn"]
SEC, HP1, DALB_MLT = 21600, 0.01, -0.075
REF_CP_OCN = 3989.24495292815                    # drivers/auscom/ice_constants.F90:30; the stock build and the device carry 4218
DT_SW = 3600.0                                   # (tests/test_pondlvl_host.py: the time step of the level-ice shortwave call)
# arrays through which no exp / atan / sin / cos flows: bit for bit under PORTS as under LIBM, on the device too
EXACT_D = ["snowfracn", "apeffn", "apeff_ai", "dhsn"]
EXACT_CONSTANT = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "alvdr", "alidr", "alvdf", "alidf", "albice", "albsno",
                  "scale_factor", "coszen", "Sswabsn"]

# The largest |restatement on PORTS - reference record| per array, relative to the array's largest magnitude in the record, over every
# record of the family; measured 2026-10-21 by `python -m tests.golden.make_ref_shortwave` (the table it prints last; DESIGN.md section
# 20), per family: C shortwave_ccsm3, D run_dEdd, V run_dEdd under tr_pond_lvl, P compute_ponds_lvl.  Arrays that are not named were
# bit-equal in every record.  main() asserts that what it measures does not exceed this table.
SPREAD_MEASURED = {
    "C": {"alvdrn": 1.14e-16, "alidrn": 1.61e-16, "alvdfn": 1.14e-16, "alidfn": 1.61e-16, "albicen": 1.77e-16, "fswsfcn": 2.5e-16,
          "fswintn": 4.63e-16, "fswthrun": 1.69e-16, "Iswabsn": 3.51e-16, "fswpenln": 2.03e-16, "alvdr": 5.91e-17, "alidr": 4.47e-17,
          "alvdf": 5.91e-17, "alidf": 4.47e-17, "albice": 4.43e-17, "scale_factor": 9.29e-17},
    "D": {"alvdrn": 2.25e-15, "alidrn": 7.71e-16, "alvdfn": 2.61e-15, "alidfn": 6.58e-16, "albicen": 1.02e-15, "albsnon": 4.86e-15,
          "fswsfcn": 2.64e-15, "fswintn": 1.65e-15, "fswthrun": 7.32e-16, "albpndn": 9.09e-16, "Sswabsn": 6.35e-14, "Iswabsn": 1.28e-15,
          "fswpenln": 1.08e-15, "alvdr": 6.53e-16, "alidr": 3.41e-16, "alvdf": 7.81e-16, "alidf": 2.15e-16, "albice": 2.14e-16,
          "albsno": 8.38e-16, "scale_factor": 3.88e-16, "albpnd": 4.88e-16},
    "V": {"alvdrn": 1.23e-15, "alidrn": 6.7e-16, "alvdfn": 1.82e-15, "alidfn": 6.15e-16, "albicen": 6.79e-16, "albsnon": 2.13e-15,
          "fswsfcn": 1.46e-15, "fswintn": 6.82e-16, "fswthrun": 7.93e-16, "albpndn": 1.05e-15, "Sswabsn": 4.23e-15, "Iswabsn": 6.92e-16,
          "fswpenln": 1.08e-15, "alvdr": 4.54e-16, "alidr": 2.52e-16, "alvdf": 4.64e-16, "alidf": 4e-16, "albice": 3.27e-16,
          "albsno": 5.81e-16, "scale_factor": 1.78e-16, "albpnd": 4.62e-16},
    "P": {"apnd": 1.11e-16, "hpnd": 2.76e-16},
}


def build_of(cfg, tcase, ncat):
    return cfg + ("" if tcase == "plain" else "_l7s2") + ("" if ncat == 5 else f"_ncat{ncat}")


# (grid, table, ncat, albedo_type)
C_RECORDS = [(cfg, t, 5, "default") for cfg in (BIG, SMALL) for t in rv.TABLES] + [(BIG, "plain", 5, "constant"), (BIG, "plain", 3, "default")]
# (grid, table, pond, ncat, namelist variant of tests/test_dedd_host.py or None)
D_VARIANTS = ["rsnw_mlt_3000", "rsnw_mlt_4", "R_snw_2", "R_ice_neg", "R_pnd_neg", "hs0_0", "kalg_0"]
D_RECORDS = [(cfg, t, pond, 5, None) for cfg in (BIG, SMALL) for t in dv.TABLES for pond in dv.PONDS] + \
            [(SMALL, "plain", "cesm", 5, v) for v in D_VARIANTS] + [(BIG, "plain", "cesm", 3, None)]
# (grid, table of pondlvlvec.TABLES, linitonly)
V_RECORDS = [(cfg, t, li) for cfg in (BIG, SMALL) for t in pv.TABLES for li in (0, 1)]
# (grid, table, frzpnd, dpscale)
P_RECORDS = [(cfg, t, fz, dp) for cfg in (BIG, SMALL) for t in pv.TABLES for fz in pv.FRZPND for dp in pv.DPSCALES]

# the builds: name -> (grid, ncat, (nilyr, nslyr)); all three are compile-time parameters of the reference
BUILDS = {}
for _cfg, _t, _n, _ in C_RECORDS:
    BUILDS[build_of(_cfg, _t, _n)] = (_cfg, _n, LAYERS[_t])
for _cfg, _t, _, _n, _ in D_RECORDS:
    BUILDS[build_of(_cfg, _t, _n)] = (_cfg, _n, LAYERS[_t])
for _cfg, _t, _ in V_RECORDS:
    BUILDS[build_of(_cfg, _t, pv.TABLES[_t])] = (_cfg, pv.TABLES[_t], LAYERS[_t])


def max_ntrcr(tcase):
    """ice_domain_size.F90:37-48 under the defines of oracle/ref/Makefile"""
    nilyr, nslyr = LAYERS[tcase]
    return 1 + 2 * nilyr + nslyr + 1 + 1 + 2 + 3 + 0 + 1 + 2


def c_path(cfg, tcase, ncat, atype, outdir=HERE):
    tag = tcase + ("" if atype == "default" else "_" + atype) + ("" if ncat == 5 else f"_ncat{ncat}")
    return os.path.join(outdir, f"ref_sw_c_{cfg}.{tag}.npz")


def d_path(cfg, tcase, pond, ncat, variant, outdir=HERE):
    tag = f"{tcase}_{pond}" + ("" if variant is None else "_" + variant) + ("" if ncat == 5 else f"_ncat{ncat}")
    return os.path.join(outdir, f"ref_sw_d_{cfg}.{tag}.npz")


def v_path(cfg, tcase, linitonly, outdir=HERE):
    return os.path.join(outdir, f"ref_sw_v_{cfg}.{tcase}{'_initonly' if linitonly else ''}.npz")


def p_path(cfg, tcase, frzpnd, dpscale, outdir=HERE):
    return os.path.join(outdir, f"ref_sw_p_{cfg}.{tcase}_{frzpnd}_dp{DPTAG[dpscale]}.npz")


DPTAG = {0.0: "0", 1.0e-3: "1em3", 1.0: "1"}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def c_input(cfg, tcase, ncat):
    return rv.rad_input(cfg, tcase, ncat=ncat)


def d_input(cfg, tcase, pond, ncat, variant=None):
    """deddvec's input under the namelist variant; a new dict, the arrays are deddvec's"""
    x = dv.dedd_input(cfg, tcase, pond, ncat=ncat)
    if variant is not None:
        from tests.test_dedd_host import VARIANTS
        x = dict(x, **VARIANTS[variant][0])
    return x


def v_input(cfg, tcase):
    return pv.pondlvl_input(cfg, tcase)


def with_coszen(x, rec):
    """the input x with the reference's compute_coszen (rec["coszen_in"]) on its ocean cells; a new dict"""
    cz = x["coszen"].copy()
    cz[x["ocean"]] = rec["coszen_in"]
    return dict(x, coszen=cz)


def coszen_place(x, delta):
    """tlat, tlon (nb, ny, nx) so that compute_coszen at sec = SEC returns x["coszen"] within rounding on the ocean cells"""
    shape = x["coszen"].shape
    side = 1.0 if delta >= 0.0 else -1.0
    tlat = side * 0.25 * hash01(shape, seed_of(x["cfg"], "swref", "tlat"))
    arg = (x["coszen"] - np.sin(tlat) * np.sin(delta)) / (np.cos(tlat) * np.cos(delta))
    assert (np.abs(arg[x["ocean"]]) < 1.0).all()
    hour = np.arccos(np.clip(arg, -1.0, 1.0))
    tlon = hour - (SEC / 86400.0 - 0.5) * 2.0 * np.pi
    return np.ascontiguousarray(tlat), np.ascontiguousarray(tlon)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def _open(x, tcase):
    cfg = x["cfg"]
    ew, ns, land = iv.BOUNDS[x["bcase"]]
    kmt, ulat = refvec.kmt_ulat(*rv.CONFIGS[cfg][:4], ew, ns, land)
    w = Writer()
    w.arr(kmt.astype(np.float64)); w.arr(ulat.astype(np.float64))
    return w, refrun.domain_nml(ew, ns)


def _state(w, x, tcase, mode):
    ncat, ntrcr = x["aicen"].shape[1], x["ntrcr"]
    mxb = rv.CONFIGS[x["cfg"]][4]
    nb, ny, nx = x["aice"].shape
    assert ntrcr <= max_ntrcr(tcase), (ntrcr, max_ntrcr(tcase))
    tr = x["tracers"]
    t = np.zeros((mxb, ncat, max_ntrcr(tcase), ny, nx))
    t[:nb, :, :x["trcrn"].shape[2]] = x["trcrn"]
    w.i4(mode); w.i4(ntrcr); w.i4(*[tr.get(k, 0) for k in IDX]); w.arr(x["tmask"].astype(np.int32))
    for k in ("aicen", "vicen", "vsnon"):
        w.arr(padded(x[k], mxb))
    w.arr(t)


def _header(r, x, tcase):
    cfg = x["cfg"]
    mxb = rv.CONFIGS[cfg][4]
    nb, ny, nx = x["aice"].shape
    ncat = x["aicen"].shape[1]
    nilyr, nslyr = LAYERS[tcase]
    hdr = r.take(np.int32, (8,))
    assert tuple(hdr) == (nx, ny, ncat, max_ntrcr(tcase), mxb, nb, nilyr, nslyr), hdr
    assert (x["tracers"]["nilyr"], x["tracers"]["nslyr"]) == (nilyr, nslyr)
    blk = r.take(np.int32, (nb, 4))
    assert [tuple(q) for q in blk] == iv.blocks_of(x["d"])
    check_constants(r.take(np.float64, (20,)), x)


def check_constants(const, x):
    """the reference's compile-time constants against what the restatements carry"""
    from tests import npdedd, nppondlvl, nprad, nptherm1
    names = ["rhos", "rhoi", "rhow", "rhofresh", "puny", "hs_min", "Timelt", "kappav", "hi_ssl", "hs_ssl",
             "hpmin", "hp0", "gravit", "viscosity_dyn", "Lfresh", "cp_ice", "cp_ocn", "depressT", "kice", "Tffresh"]
    k = x["k"]
    want = [k["rhos"], k["rhoi"], x["rhow"], nppondlvl.RHOFRESH, nprad.PUNY, npdedd.HS_MIN, nprad.TIMELT, nprad.KAPPAV, npdedd.HI_SSL, npdedd.HS_SSL, npdedd.HPMIN, npdedd.HP0, nppondlvl.GRAVIT, nppondlvl.VISCOSITY_DYN, k["Lfresh"],
            k["cp_ice"], REF_CP_OCN, nptherm1.DEPRESST, nptherm1.KICE, nptherm1.TFFRESH]
    got = dict(zip(names, (float(v) for v in const)))
    assert list(got.values()) == [float(v) for v in want], [(n, got[n], w) for n, w in zip(names, want) if got[n] != float(w)]
    assert npdedd.RHOI == got["rhoi"] and k["puny"] == got["puny"] and k["hs_min"] == got["hs_min"]


def _take_cat(r, x, n):
    mxb = rv.CONFIGS[x["cfg"]][4]
    nb, ny, nx = x["aice"].shape
    return r.take(np.float64, (n, mxb, x["aicen"].shape[1], ny, nx))[:, :nb]


def _take_layers(r, x, tcase):
    mxb = rv.CONFIGS[x["cfg"]][4]
    nb, ny, nx = x["aice"].shape
    nilyr, nslyr = LAYERS[tcase]
    return {k: r.take(np.float64, (mxb, x["aicen"].shape[1], nl, ny, nx))[:nb] for k, nl in zip(LAYER_KEYS, (nslyr, nilyr, nilyr + 1))}


def _take_2d(r, x, n):
    mxb = rv.CONFIGS[x["cfg"]][4]
    nb, ny, nx = x["aice"].shape
    return r.take(np.float64, (n, mxb, ny, nx))[:, :nb]


def run_c(x, tcase, atype):
    """shortwave_ccsm3 on one input: dict of full block arrays"""
    mxb = rv.CONFIGS[x["cfg"]][4]
    w, nml = _open(x, tcase)
    _state(w, x, tcase, 1)
    for k in ("swvdr", "swvdf", "swidr", "swidf", "ocn_albedo2D"):
        w.arr(padded(x[k], mxb))
    w.i4(int(atype == "constant"))
    w.r8(x["albicev"], x["albicei"], x["albsnowv"], x["albsnowi"], x["ahmax"], x["snowpatch"], DALB_MLT, x["awtvdr"], x["awtidr"], x["awtvdf"],
         x["awtidf"])
    w.i4(0)
    r, _ = refrun.run(refrun.exe("ref_shortwave", build_of(x["cfg"], tcase, x["aicen"].shape[1])), w.payload(), nml)
    _header(r, x, tcase)
    out = dict(zip(C3D[:9], _take_cat(r, x, 9)))
    out.update(_take_layers(r, x, tcase))
    out["coszen"] = _take_2d(r, x, 1)[0]
    out.update(zip(["alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "scale_factor"], _take_2d(r, x, 7)))
    r.done()
    return out


def run_d(x, tcase, linitonly=-1, dt=DT_SW):
    """compute_coszen and run_dEdd on one input: (dict of full block arrays with coszen_in and dhsn, exp_min, delta)"""
    mxb = rv.CONFIGS[x["cfg"]][4]
    ncat = x["aicen"].shape[1]
    exe = refrun.exe("ref_shortwave", build_of(x["cfg"], tcase, ncat))
    w, nml = _open(x, tcase)
    w.i4(4); w.r8(x["yday"]); w.i4(SEC); w.i4(0)
    r, _ = refrun.run(exe, w.payload(), nml)
    _header(r, x, tcase)
    delta = float(r.take(np.float64, (2,))[0])
    r.done()
    tlat, tlon = coszen_place(x, delta)
    zero3 = np.zeros_like(x["aicen"])
    w, nml = _open(x, tcase)
    _state(w, x, tcase, 2)
    for a in (x["swvdr"], x["swvdf"], x["swidr"], x["swidf"], tlat, tlon, x["fsnow"]):
        w.arr(padded(a, mxb))
    w.arr(padded(x.get("dhsn", zero3), mxb)); w.arr(padded(x.get("ffracn", zero3), mxb))
    w.i4(SEC, linitonly)
    w.r8(x["R_ice"], x["R_pnd"], x["R_snw"], x["dT_mlt"], x["rsnw_mlt"], x["kalg"], x["hs0"], HP1, x.get("hs1", pv.NAMELIST["hs1"]), x["pndaspect"],
         dt, x["yday"], x["awtvdr"], x["awtidr"], x["awtvdf"], x["awtidf"])
    w.i4(0)
    r, _ = refrun.run(exe, w.payload(), nml)
    _header(r, x, tcase)
    exp_min, delta2 = (float(v) for v in r.take(np.float64, (2,)))
    assert delta2 == delta
    out = dict(zip(["coszen_in", "coszen"], _take_2d(r, x, 2)))
    out.update(zip(C3D, _take_cat(r, x, 12)))
    out["dhsn"] = _take_cat(r, x, 1)[0]
    out.update(_take_layers(r, x, tcase))
    out.update(zip(AGG, _take_2d(r, x, 9)))
    r.done()
    return out, exp_min, delta


def run_p(x, y, tcase, frzpnd, dpscale):
    """compute_ponds_lvl per category on the state y (what nptherm1s.step left of the input x): dict of full block arrays"""
    from tests import nppondlvl
    mxb = rv.CONFIGS[x["cfg"]][4]
    nb, ny, nx = x["aice"].shape
    ncat = x["aicen"].shape[1]
    tr = x["tracers"]
    w, nml = _open(x, tcase)
    _state(w, dict(x, **{k: y[k] for k in ("aicen", "vicen", "vsnon", "trcrn")}), tcase, 3)
    w.arr(padded(y["frain"], mxb)); w.arr(padded(y["Tair"], mxb))
    for k in ("melttn", "meltsn", "fsurfn"):
        w.arr(padded(y[k], mxb))
    w.arr(padded(y["dhsn"], mxb))
    w.i4(nppondlvl.FRZPND[frzpnd])
    w.r8(x["dt"], x["hi_min"], dpscale, x["pndaspect"], x["rfracmin"], x["rfracmax"])
    w.i4(0)
    r, _ = refrun.run(refrun.exe("ref_shortwave", build_of(x["cfg"], tcase, ncat)), w.payload(), nml)
    _header(r, x, tcase)
    t = r.take(np.float64, (mxb, ncat, max_ntrcr(tcase), ny, nx))[:nb]
    out = {q: np.ascontiguousarray(t[:, :, tr["nt_" + q] - 1]) for q in ("apnd", "hpnd", "ipnd")}
    out["ffracn"] = r.take(np.float64, (mxb, ncat, ny, nx))[:nb]
    rest = [k for k in range(x["ntrcr"]) if k not in [tr["nt_" + q] - 1 for q in ("apnd", "hpnd", "ipnd")]]
    assert same(t[:, :, rest], y["trcrn"][:, :, rest])                                   # no other tracer plane moves
    r.done()
    return out


def check_departures(x, out, keys):
    """the device's cell lists require tmask, the reference's ask aicen > puny alone: no physical land cell carries ice, and there the
    reference leaves every category output at zero (or at the ocean albedo, which the comparison on ocean cells does not see)"""
    land = x["phys"] & ~x["ocean"]
    for q in ("aicen", "vicen", "vsnon"):
        assert not on_cells(x[q], land).any(), q
    assert (x["tmask"].astype(bool) & x["phys"] == x["ocean"]).all()
    for q in keys:
        if q in ("fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn", "fswpenln", "apeffn", "snowfracn"):
            assert not on_cells(out[q], land).any(), q


def record(x, out, keys):
    return {k: on_cells(out[k], x["ocean"]) for k in keys}


# ---- the restatements -------------------------------------------------------------------------------------------------------------
def math_of(which):
    from tests import npdedd, nprad
    return {"LIBM": (nprad.LIBM, npdedd.LIBM), "PORTS": (nprad.PORTS, npdedd.PORTS)}[which]


def restate_c(x, atype, which):
    from tests.test_rad_host import restate
    y, infos, _ = restate(x, M=math_of(which)[0], albedo_type=atype)
    return record(x, y, C_KEYS), infos


def restate_d(x, rec, variant, which):
    """tests/npdedd.py fed the reference's coszen"""
    from tests.test_dedd_host import VARIANTS, restate
    kw = VARIANTS[variant][0] if variant is not None else {}
    y, infos = restate(with_coszen(x, rec), M=math_of(which)[1], **kw)
    return record(x, y, D_KEYS), infos


def restate_v(x, rec, linitonly, which):
    from tests import nppondlvl
    from tests.test_pondlvl_host import sw_arrays, sw_params
    xx = with_coszen(x, rec)
    y = sw_arrays(xx)
    infos, pinfos = nppondlvl.step_radiation_dedd_lvl(iv.blocks_of(x["d"]), x["tmask"], sw_params(xx, linitonly), y, math_of(which)[1])
    return record(x, y, V_KEYS), infos, pinfos


def p_state(cfg, tcase):
    """(x, y): pondlvlvec's input and the state, melttn, meltsn, fsurfn tests/nptherm1s.step leaves of it without a pond scheme -- what
    compute_ponds_lvl reads inside step_therm1's category loop (tests/nppondlvl.py); shared, not modified"""
    from tests.test_pondlvl_host import th_base
    x, y, _ = th_base(cfg, tcase)
    return x, y


def restate_p(x, y0, frzpnd, dpscale, which):
    from tests import nppondlvl, nptherm1s
    from tests.test_pondlvl_host import TH_WRITTEN
    y = {k: (v.copy() if isinstance(v, np.ndarray) and k in TH_WRITTEN else v) for k, v in y0.items()}
    M = nptherm1s.PORTS if which == "PORTS" else dict(nptherm1s.PORTS, exp=math_of("LIBM")[0]["exp"])
    pinfos = nppondlvl.apply_ponds(iv.blocks_of(x["d"]), x["tmask"], dict(nppondlvl.therm_params(x, frzpnd, dpscale), cp_ocn_build=REF_CP_OCN), y, M)
    tr = x["tracers"]
    out = {q: np.ascontiguousarray(y["trcrn"][:, :, tr["nt_" + q] - 1]) for q in ("apnd", "hpnd", "ipnd")}
    out["ffracn"] = y["ffracn"]
    return record(x, out, P_KEYS), pinfos


def differing(ref, got, keys):
    """[(key, count)] of the arrays that differ bit for bit (NaN-aware)"""
    return [(k, int((~((ref[k] == got[k]) | (np.isnan(ref[k]) & np.isnan(got[k])))).sum())) for k in keys if not same(np.asarray(ref[k]), got[k])]


def spread(ref, got, keys, into):
    """the largest |got - ref| per array relative to the array's largest magnitude in the record, kept as the largest in `into`"""
    for k in keys:
        scale = float(np.abs(ref[k]).max()) if ref[k].size else 0.0
        if scale > 0.0:
            into[k] = max(into.get(k, 0.0), float(np.abs(got[k] - ref[k]).max()) / scale)


def sun_classes(x, rec):
    """the three classes of deddvec.SUN counted from the reference's returned coszen: high; between puny and 0.01; below the horizon
    under a lit forcing"""
    cz = rec["coszen_in"]
    lit = (x["swvdr"] + x["swidr"] + x["swvdf"] + x["swidf"])[x["ocean"]] > dv.PUNY
    return int((cz > 0.01).sum()), int(((cz > dv.PUNY) & (cz < 0.01)).sum()), int(((cz < 0.0) & lit).sum())


def coverage(seen):
    """what the fixtures must contain, from the info counts of the restatements: every counter of nprad over the C records, of npdedd over
    the D and D-lvl records, of nppondlvl's shortwave block over the D-lvl records and of compute_ponds_lvl over the P records --
    tests/test_rad_host.py, test_dedd_host.py and test_pondlvl_host.py show each reachable.  Returns the keys that are missing."""
    return [(fam, k) for fam, s in seen.items() for k, n in s.items() if n == 0]


def add(seen, infos):
    for i in infos:
        for k in seen:
            seen[k] += i[k]


def main(outdir=HERE):
    from tests import npdedd, nppondlvl, nprad
    seen = dict(C={k: 0 for k in nprad.INFO_KEYS}, D={k: 0 for k in npdedd.INFO_KEYS}, V={k: 0 for k in nppondlvl.SW_KEYS},
                P={k: 0 for k in nppondlvl.THERM_KEYS})
    spr = {}

    def save(path, rec):
        np.savez_compressed(path, **rec)
        print(f"   {os.path.getsize(path) / 1024:.0f} KiB")

    for cfg, tcase, ncat, atype in C_RECORDS:
        x = c_input(cfg, tcase, ncat)
        out = run_c(x, tcase, atype)
        check_departures(x, out, C_KEYS)
        rec = record(x, out, C_KEYS)
        got, infos = restate_c(x, atype, "LIBM")
        print(f"C {cfg}.{tcase} ncat={ncat} {atype}: restatement (libm) vs reference differs in {differing(rec, got, C_KEYS) or 'nothing'}")
        spread(rec, restate_c(x, atype, "PORTS")[0], C_KEYS, spr.setdefault("C", {}))
        add(seen["C"], infos)
        save(c_path(cfg, tcase, ncat, atype, outdir), rec)
    for cfg, tcase, pond, ncat, variant in D_RECORDS:
        x = d_input(cfg, tcase, pond, ncat, variant)
        out, exp_min, delta = run_d(x, tcase)
        assert exp_min == npdedd.EXP_MIN, exp_min.hex()
        check_departures(x, out, D_KEYS)
        rec = record(x, out, D_KEYS + ["coszen_in"])
        classes = sun_classes(x, rec)
        assert min(classes) > 10, classes
        assert not out["dhsn"].any()
        got, infos = restate_d(x, rec, variant, "LIBM")
        print(f"D {cfg}.{tcase} {pond} ncat={ncat} {variant or ''}: sun classes {classes}; restatement (libm) vs reference differs in "
              f"{differing(rec, got, D_KEYS) or 'nothing'}")
        spread(rec, restate_d(x, rec, variant, "PORTS")[0], D_KEYS, spr.setdefault("D", {}))
        add(seen["D"], infos)
        rec["exp_min"] = np.float64(exp_min)
        save(d_path(cfg, tcase, pond, ncat, variant, outdir), rec)
    for cfg, tcase, linitonly in V_RECORDS:
        x = v_input(cfg, tcase)
        out, exp_min, delta = run_d(x, tcase, linitonly=1 if linitonly else -1)
        assert exp_min == npdedd.EXP_MIN
        check_departures(x, out, V_KEYS)
        rec = record(x, out, V_KEYS + ["coszen_in"])
        classes = sun_classes(x, rec)
        assert min(classes) > 10, classes
        got, infos, pinfos = restate_v(x, rec, linitonly, "LIBM")
        print(f"V {cfg}.{tcase} linitonly={linitonly}: sun classes {classes}; restatement (libm) vs reference differs in "
              f"{differing(rec, got, V_KEYS) or 'nothing'}")
        spread(rec, restate_v(x, rec, linitonly, "PORTS")[0], V_KEYS, spr.setdefault("V", {}))
        add(seen["D"], infos)
        add(seen["V"], pinfos)
        rec["exp_min"] = np.float64(exp_min)
        save(v_path(cfg, tcase, linitonly, outdir), rec)
    for cfg, tcase, frzpnd, dpscale in P_RECORDS:
        x, y = p_state(cfg, tcase)
        out = run_p(x, y, tcase, frzpnd, dpscale)
        rec = record(x, out, P_KEYS)
        got, pinfos = restate_p(x, y, frzpnd, dpscale, "LIBM")
        print(f"P {cfg}.{tcase} {frzpnd} dpscale={dpscale}: restatement (libm) vs reference differs in {differing(rec, got, P_KEYS) or 'nothing'}")
        spread(rec, restate_p(x, y, frzpnd, dpscale, "PORTS")[0], P_KEYS, spr.setdefault("P", {}))
        add(seen["P"], pinfos)
        save(p_path(cfg, tcase, frzpnd, dpscale, outdir), rec)
    print(seen)
    assert not coverage(seen), coverage(seen)
    print("distance of the restatement on PORTS from the reference, largest over each family (arrays at 0 are bit-equal):")
    for fam, s in spr.items():
        print("  ", fam, {k: float(f"{v:.2e}") for k, v in s.items() if v > 0.0})
    worst = max(v for s in spr.values() for v in s.values())
    assert worst < 1.0e-12, worst                                   # (a larger one is a finding to explain, not a tolerance)
    over = [(fam, k, v) for fam, s in spr.items() for k, v in s.items() if v > 1.01 * SPREAD_MEASURED[fam].get(k, 0.0)]
    assert not over, over                                           # (1.01: the table is printed to three digits)


if __name__ == "__main__":
    main()
