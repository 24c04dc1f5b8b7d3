"""cleanup_itd, bound_state and aggregate pinned to the reference's own output (tests/golden/ref_itd_*.npz, made by
tests/golden/make_ref_itd.py from oracle/_ref/<cfg>/ref_itd): the numpy restatement tests/npitd.py against every fixture record -- bit
for bit, the routines use only + - x / and comparisons -- the paths the fixtures must contain, and the interface of the two entry points
evpk_cleanup_itd / evpk_aggregate in the header, the ctypes binding and the Fortran module.  No GPU.
"""
import ctypes as ct
import functools
import os
import re

import numpy as np
import pytest

from cice5_amd import constants as C
from cice5_amd import evpk
from tests.golden import itdvec as iv
from tests.golden import make_ref_itd as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RECORDS = [(cfg, t, b) for cfg, recs in iv.RECORDS.items() for t, b in recs]


def fixture(cfg, tcase, bcase):
    return np.load(os.path.join(GOLDEN, f"ref_itd_{cfg}.{iv.record_name(tcase, bcase)}.npz"))


@functools.lru_cache(maxsize=None)
def restated(cfg, tcase, bcase):
    """(the restatement's record, its per-block infos); computed once and shared -- do not modify"""
    x = iv.itd_input(cfg, tcase, bcase)
    y, z, infos, stop = gen.restate(x)
    assert stop is None
    return gen.restated_record(x, y, z), infos


@pytest.mark.parametrize("cfg,tcase,bcase", RECORDS)
def test_restatement_equals_the_reference(cfg, tcase, bcase):
    """arrays after cleanup_itd, flux increments, first_ice, no stop; the ghost cells after bound_state, aggregate's outputs on every
    cell, the tendencies"""
    ref = fixture(cfg, tcase, bcase)
    got, _ = restated(cfg, tcase, bcase)
    assert sorted(ref.files) == sorted(got)
    for k in ref.files:
        assert gen.same(ref[k], got[k]), k
    assert not ref["l_stop"].any()


def test_fixtures_hold_what_they_must():
    """every path of the issue's list, counted from the reference's records (and the restatement that equals them)"""
    seen = {k: 0 for k in gen.COVER}
    for cfg, tcase, bcase in RECORDS:
        gen.coverage(iv.itd_input(cfg, tcase, bcase), fixture(cfg, tcase, bcase), restated(cfg, tcase, bcase)[1], seen)
    assert all(seen[k] >= 1 for k in gen.COVER), seen
    # the chain records cover open, cyclic and tripole boundaries
    assert {b for _, _, b in RECORDS} == set(iv.BOUNDS)


@pytest.mark.parametrize("name", list(iv.STOPS))
def test_stops_equal_the_reference(name):
    """reason, lowest block, and the reference's cell: the last failing one of the loops that do not exit, the first one of zap_small_areas"""
    ref = np.load(os.path.join(GOLDEN, "ref_itd_stops.npz"))[name]
    x = iv.stop_input(name)
    _, _, _, stop = gen.restate(x)
    blocks = np.nonzero(ref[0])[0]
    assert len(blocks) == 2                                   # two blocks stop; the lowest is reported
    b = int(blocks[0])
    assert stop == (iv.STOPS[name]["reason"], b + 1, int(ref[1][b]), int(ref[2][b]))
    assert stop[1:] == iv.STOPS[name]["expect"]


def test_python_defaults_are_the_reference_constants():
    for k in evpk.ITD_CONSTANT_FIELDS:
        assert getattr(C, k) == iv.K[k], k
    assert C.rhoi == iv.K["rhoi"] and C.rhos == iv.K["rhos"]


def test_exports_header_and_fortran_interface_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evpk.h")).read(), flags=re.S)
    assert re.search(r"#define\s+EVPK_HAS_CLEANUP_ITD\s+1\b", hdr)
    assert re.search(r"#define\s+EVPK_VERSION\s+6\b", hdr)
    assert int(re.search(r"#define\s+EVPK_ITD_STOP\s+(\d+)", hdr).group(1)) == evpk.ITD_STOP
    f90 = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    assert re.search(r"EVPK_ITD_STOP = (\d+)", f90).group(1) == str(evpk.ITD_STOP)
    evpk.lib()
    for fn, nargs_want in (("evpk_cleanup_itd", 24), ("evpk_aggregate", 22)):
        assert fn in evpk.EXPORTS and re.search(r"\b" + fn + r"\s*\(", hdr)
        assert hasattr(ct.CDLL(evpk.LIB_PATH), fn)
        nargs = len(re.search(r"int " + fn + r"\(([^;]*)\);", hdr).group(1).split(","))
        assert nargs == len(getattr(evpk.lib(), fn).argtypes) == nargs_want, fn
        m = re.search(r"function " + fn + r" \(([^)]*)\)", f90)
        assert m and len(m.group(1).replace("&", "").split(",")) == nargs, fn
    for name, cls in (("evpk_itd_tracers", evpk.ItdTracers), ("evpk_itd_constants", evpk.ItdConstants)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name, hdr).group(1)
        assert re.findall(r"([A-Za-z_0-9]+)\s*[,;]", body) == [f[0] for f in cls._fields_], name
        body = re.search(r"type, bind\(C\) :: " + name + r"(.*?)end type", f90, flags=re.S).group(1)
        decl = ",".join(l.split("::")[1] for l in body.strip().splitlines())
        assert [w.split("=")[0].strip() for w in decl.split(",")] == [f[0] for f in cls._fields_], name
    assert ct.sizeof(evpk.ItdTracers) == 4 * 13 and ct.sizeof(evpk.ItdConstants) == 8 * 7
    # the sentence that said clean-up and aggregate stay with the host is gone
    assert "stay with the host.\n *   dt, ndtd" not in open(os.path.join(ROOT, "include", "evpk.h")).read()
