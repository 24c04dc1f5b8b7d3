"""ridge_ice pinned to the reference's own output (tests/golden/ref_ridge_*.npz, made by tests/golden/make_ref_ridge.py from
oracle/_ref/<cfg>/ref_ridge): the numpy restatement tests/npridge.py against every fixture record, and the measurement the GPU
tolerance rests on.  No GPU.

Restatement with libm's exp against the reference: bit for bit.  The Fortran intrinsic of the reference build and Python's math.exp
are the same libm routine here (measured: max relative difference 0 on every array of every record), so the bound is equality.

Restatement with the port of the device's exp (npridge.dev_exp) against restatement with libm: exp enters ridge_ice through
differences of exponentials (apartic = Gsum(n-1) - Gsum(n), farea = expL - expR), so a last-bit difference of exp is not a last-bit
difference of the result and the spread is not derivable in ulps.  It is measured here per array, as max |a - b| / max |a| over the
listed cells of a record in which both runs took the same branches; the GPU test bounds device-vs-reference by 4 x the largest value
over the records (spread_bounds()).
"""
import ctypes as ct
import functools
import math
import os
import re

import numpy as np
import pytest

from cice5_amd import evpk
from tests import npridge
from tests.golden import make_ref_ridge as gen
from tests.golden import ridgevec as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARRAYS = rv.STATE + rv.DIAG_2D + rv.DIAG_3D
RECORDS = [(cfg, t, s) for cfg, recs in rv.RECORDS.items() for t, s in recs]
BRANCH_CAP = 0.01                   # share of listed cells that may take another branch with another exp (ISSUE: at most 1 %)


def fixture(cfg, tcase, swn):
    return np.load(os.path.join(GOLDEN, f"ref_ridge_{cfg}.{rv.record_name(tcase, swn)}.npz"))


@functools.lru_cache(maxsize=None)
def restated(cfg, tcase, swn, which):
    """(arrays on the listed cells, per-block results) of the restatement with libm's exp ('libm') or the device's ('dev')"""
    x = rv.ridge_input(cfg, tcase)
    y, res, stop = gen.restate(x, rv.SWITCHES[swn], exp=math.exp if which == "libm" else npridge.dev_exp)
    assert stop is None
    return {k: gen.on_listed(y[k], x["listed"]) for k in ARRAYS}, res


def same_branches(cfg, tcase, swn):
    """bool per listed cell: the libm and the dev_exp restatement took the same side of every comparison"""
    r1, r2 = restated(cfg, tcase, swn, "libm")[1], restated(cfg, tcase, swn, "dev")[1]
    return np.array([a == b for ra, rb in zip(r1, r2) for a, b in zip(ra["sig"], rb["sig"])], dtype=bool)


@functools.lru_cache(maxsize=None)
def spread(cfg, tcase, swn):
    a, b, same = restated(cfg, tcase, swn, "libm")[0], restated(cfg, tcase, swn, "dev")[0], same_branches(cfg, tcase, swn)
    out = {}
    for k in ARRAYS:
        scale = float(np.abs(a[k]).max())
        out[k] = float(np.abs(a[k][same] - b[k][same]).max()) / scale if scale > 0 else 0.0
    return out


@functools.lru_cache(maxsize=None)
def spread_bounds():
    """per array: 4 x the largest measured spread over the records"""
    return {k: 4.0 * max(spread(*r)[k] for r in RECORDS) for k in ARRAYS}


@pytest.mark.parametrize("cfg,tcase,swn", RECORDS)
def test_restatement_with_libm_exp_equals_the_reference(cfg, tcase, swn):
    ref = fixture(cfg, tcase, swn)
    got, res = restated(cfg, tcase, swn, "libm")
    for k in ARRAYS:
        a, b = ref[k], got[k]
        assert a.shape == b.shape, k
        neq = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert not neq.any(), (k, int(neq.sum()), float(np.abs(a - b)[neq].max()))
    assert [r["repeats"] for r in res] == ref["repeats"].tolist()
    assert not ref["l_stop"].any()


def test_fixtures_hold_what_they_must():
    """block-wide iteration, both reductions, the round-off clamp, both values of the rafting mask -- from the reference's output and
    the restatement that equals it"""
    rep = norep = conv = t0 = tn = clamp = 0
    for cfg, tcase, swn in RECORDS:
        ref = fixture(cfg, tcase, swn)
        res = restated(cfg, tcase, swn, "libm")[1]
        for b, r in enumerate(res):
            if ref["icells"][b] == 0:
                continue
            if ref["repeats"][b] > 0:
                rep += 1
                if cfg == "g26x18_b8x5":
                    conv = max(conv, int(r["conv1"].sum()))
            else:
                norep += 1
            t0 += r.get("tmpfac0", 0); tn += r.get("tmpfacn", 0); clamp += r.get("clamp", 0)
    assert rep >= 1 and norep >= 1 and conv >= 10, (rep, norep, conv)
    assert t0 >= 1 and tn >= 1 and clamp >= 1, (t0, tn, clamp)
    ref = fixture("g26x18_b8x5", "lvl_ponds", "p1r1")
    ridged = ref["dardg2ndt"] > 0
    assert (ridged & (ref["araftn"] > 0)).any() and (ridged & (ref["araftn"] == 0)).any()


@pytest.mark.parametrize("name", list(rv.STOPS))
def test_stop_cells_equal_the_reference(name):
    ref = np.load(os.path.join(GOLDEN, "ref_ridge_stops.npz"))[name]
    x = rv.stop_input(name)
    _, _, stop = gen.restate(x, (1, 1))
    assert stop == (rv.STOPS[name]["reason"], 1, int(ref[1]), int(ref[2]))
    assert ref[0] == 1


def test_spread_between_the_two_exps(capsys):
    """measurement: restatement(dev_exp port) against restatement(libm), per array; and the branch cap holds on the CPU"""
    bounds = spread_bounds()
    with capsys.disabled():
        print("\nridge_ice: restatement(dev_exp) vs restatement(libm), max |a - b| / max |a| per array over the records; bound = 4 x")
        for k in ARRAYS:
            print(f"  {k:10s} spread {bounds[k] / 4.0:.3e}   bound {bounds[k]:.3e}")
    for r in RECORDS:
        same = same_branches(*r)
        assert (~same).sum() <= BRANCH_CAP * same.size, (r, int((~same).sum()), same.size)
    # exp is within an ulp or two on both sides, so no array may be off by more than rounding noise amplified by cancellation
    assert max(bounds.values()) < 1e-12


def test_dev_exp_port_is_close_to_libm():
    xs = np.concatenate([-np.logspace(-12, 2.5, 400), [0.0, -20.0, -0.34657359027997264, -1.0397207708399179]])
    for x in xs:
        a, b = npridge.dev_exp(float(x)), math.exp(float(x))
        assert abs(a - b) <= 2.0 * np.spacing(b), (x, a, b)


def test_exports_header_and_fortran_interface_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evpk.h")).read(), flags=re.S)
    assert "evpk_ridge_ice" in evpk.EXPORTS and re.search(r"\bevpk_ridge_ice\s*\(", hdr)
    assert re.search(r"#define\s+EVPK_VERSION\s+6\b", hdr)
    assert int(re.search(r"#define\s+EVPK_RIDGE_STOP\s+(\d+)", hdr).group(1)) == evpk.RIDGE_STOP
    assert hasattr(ct.CDLL(evpk.LIB_PATH), "evpk_ridge_ice")
    # the members of the two structs, in the header's order
    for name, cls in (("evpk_ridge_tracers", evpk.RidgeTracers), ("evpk_ridge_diag", evpk.RidgeDiag)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name, hdr).group(1)
        members = re.findall(r"\*?([A-Za-z_0-9]+)\s*[,;]", body)
        assert members == [f[0] for f in cls._fields_], name
    assert ct.sizeof(evpk.RidgeTracers) == 4 * 10 and ct.sizeof(evpk.RidgeDiag) == 8 * 16
    # the number of arguments of the C prototype, the ctypes binding and the Fortran interface
    nargs = len(re.search(r"int evpk_ridge_ice\(([^;]*)\);", hdr).group(1).split(","))
    evpk.lib()
    assert nargs == len(evpk.lib().evpk_ridge_ice.argtypes) == 18
    f90 = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    m = re.search(r"function evpk_ridge_ice \(([^)]*)\)", f90)
    assert m and len(m.group(1).replace("&", "").split(",")) == nargs
    assert re.search(r"EVPK_RIDGE_STOP = (\d+)", f90).group(1) == str(evpk.RIDGE_STOP)
    for name, cls in (("evpk_ridge_tracers", evpk.RidgeTracers), ("evpk_ridge_diag", evpk.RidgeDiag)):
        body = re.search(r"type, bind\(C\) :: " + name + r"(.*?)end type", f90, flags=re.S).group(1)
        members = re.findall(r"([A-Za-z_0-9]+) = (?:0|c_null_ptr)", body)
        assert members == [f[0] for f in cls._fields_], name
