"""evpk_step_therm2 / evpk_new_ice_lateral_melt without a GPU: the entry points are declared, exported and bound, and the numpy restatement
tests/nptherm2.py -- the checker of tests/test_therm2_gpu.py -- takes every branch of add_new_ice, lateral_melt and reduce_area on the
inputs of tests/golden/therm2vec.py and conserves what the reference's own (compile-time disabled) check asks for.

Parity with the reference is pinned for add_new_ice, lateral_melt, reduce_area and the mushy liquidus: tests/test_therm2_ref.py holds the
restatement to reference-built records stage by stage.  Unpinned stay step_therm2's call order, a non-uniform salinz, aerosols / bgc and
l_conservation_check = .true.

Reported, not asserted (a count that depends on rounding, not on a rule of the routine):
  fy_clamped    FY = 1 in category 1 makes (FY area1 + ai0new) / aicen(1) exceed 1 only when the division rounds up; the input FY = 1 is
                asserted (fy_is_one), the clamp's count is printed.
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from cice5_amd import evpk
from tests import nptherm2
from tests.golden import itdvec as iv
from tests.golden import therm2vec as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMERIC = [k for k in tv.OUT if k != "first_ice"]


def arrays(x):
    """copies of every array a call may write, and the read-only ones as they are"""
    y = {k: (x[k].copy() if x[k] is not None else None) for k in tv.OUT}
    y.update({k: x[k] for k in ("aicen_init", "vicen_init", "frain", "frzmlt", "Tf", "sss", "rside", "salinz")})
    return y


def restate(x, ktherm=1, update_ocn_f=False, debug=None, **kw):
    """section 1 alone (add_new_ice, lateral_melt, reduce_area) on copies: (arrays, infos)"""
    y = arrays(dict(x, **kw))
    p = nptherm2.params(x, ktherm, update_ocn_f)
    if y.get("frz_onset") is None:
        p["use_frz_onset"] = False
    infos = nptherm2.new_ice_lateral_melt(iv.blocks_of(x["d"]), x["tmask"], p, y, debug)
    return y, infos


def restate_step(x, kitd, ktherm=1, update_ocn_f=False, **kw):
    """the chain of step_therm2 on copies: (arrays, infos, stop)"""
    y = arrays(dict(x, **kw))
    p = nptherm2.params(x, ktherm, update_ocn_f)
    infos, stop = nptherm2.step_therm2(iv.blocks_of(x["d"]), x["tmask"], p, y, kitd, x["hi_min"], y["first_ice"])
    return y, infos, stop


_cache = {}


def restated(cfg, tcase, ktherm, ncat=5):
    key = (cfg, tcase, ktherm, ncat)
    if key not in _cache:
        x = tv.therm2_input(cfg, tcase, ncat=ncat)
        dbg = []
        _cache[key] = (x,) + restate(x, ktherm, debug=dbg) + (dbg,)
    return _cache[key]


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "evpk.h")).read()
    assert re.search(r"^#define EVPK_HAS_STEP_THERM2 1$", hdr, re.M)
    assert re.search(r"^#define EVPK_VERSION 6$", hdr, re.M)
    assert re.search(r"^int evpk_new_ice_lateral_melt\(evpk_ctx \*c, const evpk_therm2_args \*a\);", hdr, re.M)
    assert re.search(r"^int evpk_step_therm2\(evpk_ctx \*c, const evpk_therm2_args \*a, int32_t stop\[5\]", hdr, re.M)
    body = re.search(r"typedef struct \{([^}]*)\} evpk_therm2_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [w.strip().split()[-1].lstrip("*") for part in body.split(";") for w in part.split(",") if w.strip()]
    assert names == [n for n, _ in evpk.Therm2Args._fields_]                            # the ctypes mirror, member for member


def test_symbols_are_exported_and_bound():
    L = ct.CDLL(evpk.LIB_PATH)
    for n in ("evpk_new_ice_lateral_melt", "evpk_step_therm2"):
        assert n in evpk.EXPORTS and hasattr(L, n)
    assert callable(evpk.Context.new_ice_lateral_melt) and callable(evpk.Context.step_therm2)
    assert evpk.THERM2_STAGES == {1: "linear_itd", 3: "cleanup_itd"}


def test_fortran_interface():
    src = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    assert "bind(C, name='evpk_new_ice_lateral_melt')" in src and "bind(C, name='evpk_step_therm2')" in src
    assert "type, bind(C) :: evpk_therm2_args" in src


REPORTED = {"fy_clamped", "fpond_changed", "reduce_hin", "reduce_dhi", "reduce_none", "untouched"}


@pytest.mark.parametrize("cfg", list(tv.CONFIGS))
def test_inputs_take_every_branch(cfg):
    """the counts of the restatement's info records, summed over the blocks, the four pond tables and both ktherm of one grid"""
    tot = {k: 0 for k in nptherm2.INFO_KEYS}
    for tcase in tv.POND_CASES:
        for ktherm in (1, 2):
            x, y, infos, dbg = restated(cfg, tcase, ktherm)
            for i in infos:
                for k in tot:
                    tot[k] += i[k]
            assert any(i["jcells"] and i["kcells"] and i["rside_part"] and i["frzmlt_neg"] for i in infos), "a block that mixes the kinds"
            assert (x["aicen"][1] == 0.0).all() and infos[1]["jcells"] > 0, "an ice-free block that grows new ice"
            if x["tracers"].get("tr_pond_topo"):
                assert sum(i["fpond_changed"] for i in infos) > 0
            if x["tracers"].get("tr_pond_lvl"):
                assert sum(i["pond_lvl"] for i in infos) > 0 and sum(i["pond_lvl_skipped"] for i in infos) > 0
    print(cfg, tot)
    for k in nptherm2.INFO_KEYS:
        if k not in REPORTED:
            assert tot[k] > 0, k
    assert tot["untouched"] > 0


def test_single_category_takes_reduce_area():
    x, y, infos, dbg = restated("g26x18_b8x5", "lvl_ponds", 1, ncat=1)
    tot = {k: sum(i[k] for i in infos) for k in nptherm2.INFO_KEYS}
    print(tot)
    assert tot["reduce_hin"] == 0                       # (hin_max(0) = 0 under this table)
    assert tot["reduce_dhi"] > 0 and tot["reduce_none"] > 0 and tot["surplus_open"] == 0
    x, y, infos, dbg = restated("g26x18_b8x5", "cesm_ponds", 2, ncat=1)
    assert sum(i["reduce_hin"] for i in infos) > 0      # hin_max(0) = 0.1: new ice thinner than that is made thicker


@pytest.mark.parametrize("cfg", list(tv.CONFIGS))
@pytest.mark.parametrize("ktherm", [1, 2])
def test_add_new_ice_passes_the_references_own_conservation_check(cfg, ktherm):
    """ice_therm_itd.F90:1426-1451, :1511-1514, :1790-1829 from outside, independent of the restatement's tracer code: volume and ice energy
    per cell after add_new_ice alone (rside = 0), to puny and puny * Lfresh * rhoi"""
    for tcase in ("plain", "lvl_ponds"):
        x = tv.therm2_input(cfg, tcase)
        dbg = []
        y, infos = restate(x, ktherm, debug=dbg, rside=np.zeros_like(x["rside"]))
        k, tr = x["k"], x["tracers"]
        q0 = tr["nt_qice"] - 1

        def sums(z):
            vice = np.zeros(z["aice"].shape); eice = np.zeros(z["aice"].shape)
            for n in range(x["ncat"]):
                vice = vice + z["vicen"][:, n]
                e = np.zeros(z["aice"].shape)
                for l in range(tr["nilyr"]):
                    e = e + z["trcrn"][:, n, q0 + l] * z["vicen"][:, n] / float(tr["nilyr"])
                eice = eice + e
            return vice, eice
        v0, e0 = sums(x)
        v1, e1 = sums(y)
        checked = 0
        for b, loc in enumerate(dbg):
            J, I = loc["J"], loc["I"]
            vi0 = y["frazil"][b, J, I]                  # vi0new before the distribution decision
            dv = np.abs(v1[b, J, I] - (v0[b, J, I] + vi0))
            de = np.abs(e1[b, J, I] - (e0[b, J, I] + vi0 * loc["qi0new"]))
            assert dv.max() <= nptherm2.PUNY, (tcase, b, float(dv.max()))
            assert de.max() <= nptherm2.PUNY * k["Lfresh"] * k["rhoi"], (tcase, b, float(de.max()))
            checked += int((vi0 > 0.0).sum())
        assert checked > 100


@pytest.mark.parametrize("cfg", list(tv.CONFIGS))
def test_lateral_melt_removes_the_mass_it_reports(cfg):
    """frzmlt = 0, ktherm = 1: fresh changes through lateral_melt alone, and (fresh - fresh0) dt is the ice and snow mass that left"""
    x = tv.therm2_input(cfg, "topo_ponds")
    y, infos = restate(x, 1, frzmlt=np.zeros_like(x["frzmlt"]))
    k, dt = x["k"], x["dt"]
    dv = np.zeros(x["aice"].shape); ds = np.zeros(x["aice"].shape)
    for n in range(x["ncat"]):
        dv = dv + (x["vicen"][:, n] - y["vicen"][:, n])
        ds = ds + (x["vsnon"][:, n] - y["vsnon"][:, n])
    err = np.abs((y["fresh"] - x["fresh"]) * dt - (k["rhoi"] * dv + k["rhos"] * ds))
    melted = x["ocean"] & (x["rside"] > 0.0)
    assert melted.sum() > 50 and (dv[melted] > 0.0).any()
    assert err.max() <= nptherm2.PUNY * k["rhoi"], float(err.max())
    assert np.array_equal(y["fresh"][~melted], x["fresh"][~melted])
    full = x["ocean"] & (x["rside"] == 1.0)
    assert full.any()
    for q in ("aicen", "vicen", "vsnon"):
        assert not np.moveaxis(y[q], 1, -1)[full].any(), q


@pytest.mark.parametrize("ktherm", [1, 2])
def test_no_growth_and_no_melt_leaves_the_state_bitwise(ktherm):
    x = tv.therm2_input("g26x18_b8x5", "lvl_ponds", quiet=True)
    assert (x["frzmlt"] <= 0.0).all() and (x["rside"] <= 0.0).all()
    y, infos = restate(x, ktherm)
    assert sum(i["untouched"] for i in infos) == int(x["ocean"].sum()) > 100
    for q in NUMERIC:
        if q != "frazil":
            assert np.array_equal(y[q], x[q]), q
    assert not y["frazil"][x["ocean"]].any() and np.array_equal(y["frazil"][~x["ocean"]], x["frazil"][~x["ocean"]])


def test_step_chain_restatement_runs_and_rebins_the_thick_new_ice():
    """an ice-free cell whose new ice is thicker than hi0max goes into category 1 alone; cleanup_itd's rebin then moves it up"""
    x = tv.therm2_input("g26x18_b8x5", "plain")
    y1, _ = restate(x, 1)
    y, infos, stop = restate_step(x, 1)
    assert stop is None
    thick = (x["kinds"] == "thick_free") & (x["rside"] <= 0.0)          # (not melted again)
    assert thick.sum() >= 3
    assert (y1["aicen"][:, 0][thick] > 0.0).all() and (y["aicen"][:, 0][thick] == 0.0).all() and (y["aicen"][:, 1:].sum(axis=1)[thick] > 0.0).all()
    x2 = tv.stop_input()
    _, _, stop = restate_step(x2, 0)
    assert stop == (3,) + x2["stop_expect"]
