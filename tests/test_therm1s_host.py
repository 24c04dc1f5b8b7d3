"""evpk_step_therm1 without a GPU: the entry point is declared, exported and bound (header, ctypes structure and Fortran type member by
member), and the numpy restatement tests/nptherm1s.py -- the checker of tests/test_therm1s_gpu.py -- takes every branch the inputs of
tests/golden/therm1svec.py are drawn for, converges in every listed column, trips no stop, and satisfies, recomputed from outside its
own code, the bounds of frzmlt_bottom_lateral and the sums of merge_fluxes.

**Parity with the reference is unpinned**: no reference-built record exists for these routines.

The spread between the restatement on the ports of the device's math (tests/npfmath2.py, npridge.dev_exp) and on libm is printed per
array and bounded by four times the spread measured here with libm, as
tests/test_ridge_ref.py::test_spread_between_the_two_exps does; at most 1 % of the listed (cell, category) columns may take another branch.
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from cice5_amd import evpk
from tests import nptherm1, nptherm1s
from tests.golden import itdvec as iv
from tests.golden import therm1svec as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTED = ["frzmlt_neg", "frzmlt_pos", "fbot_product", "fbot_frzmlt", "ustar_below", "ustar_above", "deltaT_zero", "deltaT_pos", "xtmp_limits",
           "xtmp_one", "rside_one", "wind_below", "wind_above", "stable", "unstable", "hol_clamped", "hol_free", "delq_pos", "delq_neg",
           "zlvl_not_zref", "in_lmask_n", "in_lmask_s", "in_neither", "pond_thin", "pond_grow", "pond_frozen", "pond_capped", "listed", "merged"]
# the largest |ports - libm| measured here per array, relative to the array's largest magnitude, over both grids and both tables
# (printed by test_spread_between_ports_and_libm); the test allows four times as much
SPREAD_MEASURED = 2.6e-15


def arrays(x):
    """copies of every array a call may write, and the read-only ones as they are"""
    y = {k: (x[k].copy() if x[k] is not None else None) for k in sv.WRITTEN}
    y.update({k: x[k] for k in sv.IN2D + ["flw", "potT", "Qa", "rhoa", "fsnow", "sss", "fswthrun", "lmask_n", "lmask_s", "yday"]})
    return y


def restate(x, M=nptherm1s.PORTS, iters=None, **kw):
    """(arrays, infos, stop, sig) of the restatement on copies; kw: members that replace those of x (natmiter, calc_strair, yday, tracers)"""
    y = arrays(dict(x, **kw))
    p = nptherm1s.params(dict(x, **kw))
    infos, stop, sig = nptherm1s.step(iv.blocks_of(x["d"]), x["tmask"], p, y, M, iters)
    return y, infos, stop, sig


_cache = {}


def restated(cfg, tcase, ncat=5, **kw):
    """the inputs and the restatement on the ports: computed once per case, shared, not modified"""
    key = (cfg, tcase, ncat) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _cache:
        x = sv.therm1s_input(cfg, tcase, ncat=ncat)
        its = []
        _cache[key] = (x,) + restate(x, iters=its, **kw) + (its,)
    return _cache[key]


def _struct_names(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [w.strip().split()[-1].lstrip("*") for part in body.split(";") for w in part.split(",") if w.strip()]


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "evpk.h")).read()
    assert re.search(r"^#define EVPK_HAS_STEP_THERM1 1$", hdr, re.M)
    assert re.search(r"^#define EVPK_VERSION 6$", hdr, re.M)
    assert re.search(r"^int evpk_step_therm1\(evpk_ctx \*c, const evpk_therm1_args \*a, int32_t stop\[5\]", hdr, re.M)
    assert _struct_names(hdr, "evpk_therm1_args") == [n for n, _ in evpk.Therm1Args._fields_]      # the ctypes mirror, member for member
    assert evpk.Therm1Args._fields_[0] == ("tv", evpk.ThermoArgs)
    block = hdr[hdr.index("SURVEY S8 row f-11"):hdr.index("#define EVPK_HAS_STEP_THERM1")]
    assert "**Parity unpinned**" in block
    for word in ("neutral_drag_coeffs", "highfreq", "atmo_boundary_const", "compute_ponds_lvl", "compute_ponds_topo", "update_aerosol",
                 "set_sfcflux", "prep_radiation", "ktherm = 2", "ACCESS", "tmask", "icells > 0"):
        assert word in block, word


def test_symbol_is_exported_and_bound():
    L = ct.CDLL(evpk.LIB_PATH)
    assert "evpk_step_therm1" in evpk.EXPORTS and hasattr(L, "evpk_step_therm1")
    assert callable(evpk.Context.step_therm1)
    assert evpk.THERM1_MERGED == nptherm1s.MERGED == sv.MERGED and len(evpk.THERM1_MERGED) == 22
    assert evpk.THERM1_IN2D == sv.IN2D


def test_fortran_interface():
    src = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    assert "bind(C, name='evpk_step_therm1')" in src and "type, bind(C) :: evpk_therm1_args" in src
    body = src[src.index("type, bind(C) :: evpk_therm1_args"):src.index("end type evpk_therm1_args")]
    body = re.sub(r"!.*", "", body)
    names = [re.sub(r"\s*=.*", "", w).strip() for line in body.splitlines()[1:] if "::" in line for w in re.split(r",(?![^(]*\))", line.split("::")[1])]
    assert names == [n for n, _ in evpk.Therm1Args._fields_]
    assert "type (evpk_thermo_args) :: tv" in body


@pytest.mark.parametrize("cfg", list(sv.CONFIGS))
def test_inputs_take_every_branch_converge_and_trip_no_stop(cfg):
    """the counts of the restatement's info records, summed over the blocks and the two tracer tables of one grid: every item of the
    input list of tests/golden/therm1svec.py, each non-zero; every listed column converges and no stop trips"""
    tot = {k: 0 for k in COUNTED}
    for tcase in sv.TABLES:
        x, y, infos, stop, sig, its = restated(cfg, tcase)
        assert stop is None, (tcase, stop)
        listed = int(((x["aicen"] > sv.PUNY) & x["ocean"][:, None]).sum())
        assert len(its) == listed > 300 and max(i[-1] for i in its) < nptherm1.NITERMAX
        for i in infos:
            for k in tot:
                tot[k] += i[k]
        assert (x["aicen"][1] == 0.0).all() and infos[1]["listed"] == 0, "an ice-free block"
        for q in sv.MERGED + ["Cdn_atm"]:
            assert (x[q][x["ocean"]] != 0.0).all(), q
    print(cfg, tot)
    for k in COUNTED:
        assert tot[k] > 0, k
    for yday, key in ((259.0, "in_lmask_n"), (75.0, "in_lmask_s")):                     # the two windows of update_FYarea
        _, _, infos, stop, _, _ = restated(cfg, "plain", yday=yday)
        assert stop is None and sum(i["fy_reset"] for i in infos) == sum(i[key] for i in infos) > 0
    assert sum(i["fy_reset"] for i in restated(cfg, "plain")[2]) == 0                   # yday = 123: outside both


@pytest.mark.parametrize("cfg", list(sv.CONFIGS))
@pytest.mark.parametrize("tcase", sv.TABLES)
def test_bounds_and_sums_from_the_returned_arrays(cfg, tcase):
    """from outside the restatement's own code: frzmlt <= fbot <= 0 and 0 <= rside <= 1; fbot + fside >= frzmlt after limiting, to
    rounding, with fside recomputed from the state of entry; each merged plane equals the caller's value plus the category-ordered sum of
    aicen_init times the per-category plane"""
    x, y, infos, stop, sig, its = restated(cfg, tcase)
    tr, dt = x["tracers"], x["dt"]
    ncat = x["aicen"].shape[1]
    phys = np.zeros(x["aice"].shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(iv.blocks_of(x["d"])):
        phys[b, jlo - 1:jhi, ilo - 1:ihi] = True
    melt = phys & (x["aice"] > sv.PUNY) & (x["frzmlt"] < 0.0)
    assert melt.sum() > 20
    assert (y["fbot"][melt] >= x["frzmlt"][melt]).all() and (y["fbot"] <= 0.0).all()
    assert (y["rside"] >= 0.0).all() and (y["rside"] <= 1.0).all()
    assert not y["fbot"][~melt].any() and not y["rside"][~melt].any() and np.array_equal(y["Tbot"], x["Tf"])
    etot = np.zeros(x["aice"].shape)
    for n in range(ncat):
        for l in range(tr["nslyr"]):
            etot = etot + x["trcrn"][:, n, tr["nt_qsno"] - 1 + l] * x["vsnon"][:, n] / tr["nslyr"]
        for l in range(tr["nilyr"]):
            etot = etot + x["trcrn"][:, n, tr["nt_qice"] - 1 + l] * x["vicen"][:, n] / tr["nilyr"]
    fside = y["rside"] * etot / dt
    slack = 1.0e-9 * np.abs(x["frzmlt"]) + 1.0e-9
    assert ((y["fbot"] + fside)[melt] >= (x["frzmlt"] - slack)[melt]).all()
    for q in ("aice_init", "aicen_init", "vicen_init"):
        assert np.array_equal(y[q], x[q[:-5]]), q
    listed = (x["aicen"] > sv.PUNY) & x["ocean"][:, None]
    for q in sv.PERCAT8:
        assert not y[q][~listed].any() and y[q][listed].any(), q
    fswabsn = (y["fswsfcn"] + y["fswintn"]) + x["fswthrun"]
    per = dict(y, fswabsn=fswabsn, flwoutn=y["flwoutn"] - (1.0 - nptherm1.EMISSIVITY) * x["flw"][:, None])
    for m, q in nptherm1s.MERGE:
        want = x[m].copy()
        for n in range(ncat):
            want = want + np.where(listed[:, n], per[q][:, n] * x["aicen"][:, n], 0.0)
        assert np.array_equal(want, y[m]), m
        assert not np.array_equal(y[m], x[m]), m


def _branches_differ(sa, sb):
    keys = [k for k in sa if len(k) == 4]                                              # the listed (block, category, j, i) columns
    return sum(1 for k in keys if sa[k] != sb[k]) + sum(1 for k in sa if len(k) == 3 and sa[k] != sb[k]), len(keys)


def test_spread_between_ports_and_libm():
    """the restatement on the ports against the restatement on math.exp / log / atan / pow: the device's fixed algorithms are within
    1 - 2 ulp of glibc, and the call amplifies that no further than this"""
    worst = 0.0
    for cfg in sv.CONFIGS:
        for tcase in sv.TABLES:
            x, y, infos, stop, sig, its = restated(cfg, tcase)
            z, _, stop2, sig2 = restate(x, nptherm1s.LIBM)
            assert stop is None and stop2 is None
            differ, n = _branches_differ(sig, sig2)
            print(cfg, tcase, "columns on another branch:", differ, "of", n)
            assert differ <= 0.01 * n
            for k in sv.WRITTEN:
                if y[k] is None:
                    continue
                scale = float(np.abs(y[k]).max())
                spread = float(np.abs(y[k] - z[k]).max()) / scale if scale else 0.0
                print(f"  {k:16s} {spread:.3e}")
                worst = max(worst, spread)
    print("largest relative spread", worst)
    assert worst <= 4.0 * SPREAD_MEASURED
