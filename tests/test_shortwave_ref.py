"""shortwave_ccsm3 (compute_albedos, constant_albedos, absorbed_solar), run_dEdd (shortwave_dEdd_set_snow / _set_pond, shortwave_dEdd,
compute_dEdd, solution_dEdd, with its tr_pond_cesm, tr_pond_lvl and no-pond blocks) and compute_ponds_lvl (brine_permeability) pinned to
the reference's own output (tests/golden/ref_sw_*.npz, made by tests/golden/make_ref_shortwave.py from oracle/_ref/<build>/ref_shortwave):
the numpy restatements tests/nprad.py, tests/npdedd.py and tests/nppondlvl.py against every fixture record, array by array, on the physical
ocean cells.

On LIBM (math.exp / math.atan) the restatements equal the reference BIT FOR BIT, NaN-aware, in every array of every record: both sides are
built without fused multiply-add, and the reference's exp / atan and Python's are the same libm here.  On PORTS (the device's
fixed-algorithm exp / atan) every array is within the distance make_ref_shortwave.SPREAD_MEASURED records -- the table
tests/test_shortwave_ref_gpu.py takes its tolerance from, recounted here from the committed files -- and the arrays and cells through which
no exp / atan flows are bit-equal under PORTS too, asserted on their own so that no tolerance elsewhere can blur a misread branch:
  snowfracn, apeffn, apeff_ai, the coszen run_dEdd returns and the pond-lvl block's dhsn;
  under albedo_type = 'constant': every albedo and what is built from albedos alone (fswsfcn, Sswabsn, the aggregates, scale_factor) --
  absorbed_solar's exp still enters Iswabsn, fswintn, fswthrun and fswpenln of those records;
  on night cells (all four sw* zero): every output of run_dEdd, and the radiation arrays of shortwave_ccsm3 (its albedos go through atan
  whatever the sun does);
  every zero of the reference (unlisted cells, the ice-free block) is a zero.

The dEdd restatements are fed the coszen the reference's compute_coszen returned (coszen_in): compute_coszen stays with the caller on the
device.  Mode P holds nppondlvl.compute_ponds_lvl with brine_permeability to the reference on the CPU only -- the device has no entry
point for it alone, and evpk_step_therm1_lvl as a whole stays unpinned with step_therm1.  The reference's AusCOM build fixes cp_ocn =
3989.24495292815 where the device's thermodynamics carry the stock 4218 (include/evpk.h); brine_permeability is held to the reference
with the build's value handed in, so its algebra is pinned and the constant is not.

Still unpinned: step_radiation's own call order, its zeroing and the albedo aggregation / scale_factor lines of coupling_prep (the driver
restates them), the stock scalar albocn path, aerosols, topographic ponds, evpk_step_therm1_lvl beyond compute_ponds_lvl and thermo_vertical
/ step_therm1.  No GPU.
"""
import functools
import os

import numpy as np
import pytest

from tests import npdedd, nppondlvl, nprad
from tests.golden import deddvec as dv
from tests.golden import make_ref_shortwave as gen
from tests.golden import radvec as rv

C_IDS = [f"{c}-{t}-ncat{n}-{a}" for c, t, n, a in gen.C_RECORDS]
D_IDS = [f"{c}-{t}-{p}-ncat{n}{'-' + v if v else ''}" for c, t, p, n, v in gen.D_RECORDS]
V_IDS = [f"{c}-{t}-linitonly{li}" for c, t, li in gen.V_RECORDS]
P_IDS = [f"{c}-{t}-{fz}-dp{gen.DPTAG[dp]}" for c, t, fz, dp in gen.P_RECORDS]


@functools.lru_cache(maxsize=None)
def c_case(cfg, tcase, ncat, atype):
    """(input, fixture, restated on LIBM, restated on PORTS, infos): computed once and shared -- do not modify"""
    x = gen.c_input(cfg, tcase, ncat)
    libm, infos = gen.restate_c(x, atype, "LIBM")
    return x, np.load(gen.c_path(cfg, tcase, ncat, atype)), libm, gen.restate_c(x, atype, "PORTS")[0], infos


@functools.lru_cache(maxsize=None)
def d_case(cfg, tcase, pond, ncat, variant):
    x = gen.d_input(cfg, tcase, pond, ncat, variant)
    ref = np.load(gen.d_path(cfg, tcase, pond, ncat, variant))
    libm, infos = gen.restate_d(x, ref, variant, "LIBM")
    return x, ref, libm, gen.restate_d(x, ref, variant, "PORTS")[0], infos


@functools.lru_cache(maxsize=None)
def v_case(cfg, tcase, linitonly):
    x = gen.v_input(cfg, tcase)
    ref = np.load(gen.v_path(cfg, tcase, linitonly))
    libm, infos, pinfos = gen.restate_v(x, ref, linitonly, "LIBM")
    return x, ref, libm, gen.restate_v(x, ref, linitonly, "PORTS")[0], infos, pinfos


@functools.lru_cache(maxsize=None)
def p_case(cfg, tcase, frzpnd, dpscale):
    x, y = gen.p_state(cfg, tcase)
    libm, pinfos = gen.restate_p(x, y, frzpnd, dpscale, "LIBM")
    return x, np.load(gen.p_path(cfg, tcase, frzpnd, dpscale)), libm, gen.restate_p(x, y, frzpnd, dpscale, "PORTS")[0], pinfos


def count(ref, got):
    return int((~((ref == got) | (np.isnan(ref) & np.isnan(got)))).sum())


def assert_bit_equal(ref, got, keys, what):
    for k in keys:
        assert gen.same(ref[k], got[k]), (what, k, count(ref[k], got[k]))


def assert_within(ref, got, keys, fam, factor, what):
    """bit-equal where SPREAD_MEASURED names no distance; else max |got - ref| <= factor x distance x max |ref|"""
    for k in keys:
        bound = gen.SPREAD_MEASURED[fam].get(k, 0.0)
        if bound == 0.0 or not ref[k].any():
            assert gen.same(ref[k], got[k]), (what, k, count(ref[k], got[k]))
        else:
            assert np.array_equal(np.isnan(ref[k]), np.isnan(got[k])), (what, k)
            err = float(np.nanmax(np.abs(got[k] - ref[k]), initial=0.0))
            assert err <= factor * bound * float(np.abs(ref[k]).max()), (what, k, err / float(np.abs(ref[k]).max()), bound)


def night(x):
    """the ocean cells on which all four shortwave bands are zero, in the records' order"""
    return ((x["swvdr"] == 0.0) & (x["swvdf"] == 0.0) & (x["swidr"] == 0.0) & (x["swidf"] == 0.0))[x["ocean"]]


def assert_exact_cells(x, ref, got, keys, night_keys, what):
    """the night cells of night_keys and every zero of the reference, bit for bit"""
    dark = night(x)
    assert dark.sum() > 50
    for k in night_keys:
        assert gen.same(ref[k][dark], got[k][dark]), (what, "night", k, count(ref[k][dark], got[k][dark]))
    for k in keys:
        zero = ref[k] == 0.0
        assert not got[k][zero].any(), (what, "zeros", k, int((got[k][zero] != 0.0).sum()))


@pytest.mark.parametrize("cfg,tcase,ncat,atype", gen.C_RECORDS, ids=C_IDS)
def test_ccsm3_restatement_equals_the_reference(cfg, tcase, ncat, atype):
    x, ref, libm, ports, infos = c_case(cfg, tcase, ncat, atype)
    assert_bit_equal(ref, libm, gen.C_KEYS, "libm")
    assert_within(ref, ports, gen.C_KEYS, "C", 1.01, "ports")
    assert_exact_cells(x, ref, ports, gen.C_KEYS, rv.RADIATION, "ports")
    if atype == "constant":
        assert_bit_equal(ref, ports, gen.EXACT_CONSTANT, "ports, constant albedos")
    assert (ref["coszen"] == 0.5).all() and ref["fswsfcn"].any() and ref["Iswabsn"].any()


@pytest.mark.parametrize("cfg,tcase,pond,ncat,variant", gen.D_RECORDS, ids=D_IDS)
def test_dedd_restatement_equals_the_reference(cfg, tcase, pond, ncat, variant):
    x, ref, libm, ports, infos = d_case(cfg, tcase, pond, ncat, variant)
    assert float(ref["exp_min"]) == npdedd.EXP_MIN
    assert_bit_equal(ref, libm, gen.D_KEYS, "libm")
    assert_within(ref, ports, gen.D_KEYS, "D", 1.01, "ports")
    assert_bit_equal(ref, ports, ["snowfracn", "apeffn", "apeff_ai", "coszen"], "ports, no exp")
    assert_exact_cells(x, ref, ports, gen.D_KEYS, dv.WRITTEN, "ports")
    assert min(gen.sun_classes(x, ref)) > 10
    assert ref["fswsfcn"].any() and ref["Sswabsn"].any() and ref["apeffn"].any()


@pytest.mark.parametrize("cfg,tcase,linitonly", gen.V_RECORDS, ids=V_IDS)
def test_dedd_lvl_restatement_equals_the_reference(cfg, tcase, linitonly):
    x, ref, libm, ports, infos, pinfos = v_case(cfg, tcase, linitonly)
    assert_bit_equal(ref, libm, gen.V_KEYS, "libm")
    assert_within(ref, ports, gen.V_KEYS, "V", 1.01, "ports")
    assert_bit_equal(ref, ports, ["snowfracn", "apeffn", "apeff_ai", "coszen", "dhsn"], "ports, no exp")
    assert_exact_cells(x, ref, ports, gen.V_KEYS, dv.WRITTEN, "ports")
    assert min(gen.sun_classes(x, ref)) > 10
    # under initonly = .true. dhsn keeps the caller's values; otherwise the block initialises and resets some
    assert gen.same(ref["dhsn"], gen.on_cells(x["dhsn"], x["ocean"])) == bool(linitonly)


def test_the_lvl_block_differs_from_the_cesm_block_and_initonly_from_the_step():
    """the records are held to different text of run_dEdd: apeffn under tr_pond_lvl is not apeffn under tr_pond_cesm, and initonly moves it"""
    a = v_case(gen.BIG, "plain", 0)[1]
    b = v_case(gen.BIG, "plain", 1)[1]
    assert not gen.same(a["apeffn"], b["apeffn"]) and not gen.same(a["snowfracn"], b["snowfracn"])
    c = d_case(gen.BIG, "plain", "cesm", 5, None)[1]
    n = d_case(gen.BIG, "plain", "none", 5, None)[1]
    assert not gen.same(c["apeffn"], n["apeffn"]) and not gen.same(c["albpndn"], n["albpndn"])


@pytest.mark.parametrize("cfg,tcase,frzpnd,dpscale", gen.P_RECORDS, ids=P_IDS)
def test_compute_ponds_lvl_restatement_equals_the_reference(cfg, tcase, frzpnd, dpscale):
    """CPU only: the device has no entry point for compute_ponds_lvl alone; evpk_step_therm1_lvl as a whole stays unpinned with
    step_therm1.  The restatement is handed the AusCOM build's cp_ocn for brine_permeability (see the module docstring)"""
    x, ref, libm, ports, pinfos = p_case(cfg, tcase, frzpnd, dpscale)
    assert_bit_equal(ref, libm, gen.P_KEYS, "libm")
    assert_within(ref, ports, gen.P_KEYS, "P", 1.01, "ports")
    assert_bit_equal(ref, ports, ["ipnd", "ffracn"], "ports, no exp")
    tr = x["tracers"]
    moved = [not gen.same(ref[q], gen.on_cells(x["trcrn"][:, :, tr["nt_" + q] - 1], x["ocean"])) for q in ("apnd", "hpnd", "ipnd")]
    assert moved[0] and moved[1] and moved[2] == (frzpnd == "hlid")
    assert ref["ffracn"].any() == (frzpnd == "hlid")


def test_fixtures_hold_what_they_must():
    """coverage recounted from the committed files: every counter of the restatements (which equal the records bit for bit, asserted above
    and again here) over its family, the sun classes in every dEdd record, and the records the issue names"""
    seen = dict(C={k: 0 for k in nprad.INFO_KEYS}, D={k: 0 for k in npdedd.INFO_KEYS}, V={k: 0 for k in nppondlvl.SW_KEYS},
                P={k: 0 for k in nppondlvl.THERM_KEYS})
    for c in gen.C_RECORDS:
        x, ref, libm, ports, infos = c_case(*c)
        assert all(gen.same(ref[k], libm[k]) for k in gen.C_KEYS), c
        gen.add(seen["C"], infos)
    for c in gen.D_RECORDS:
        x, ref, libm, ports, infos = d_case(*c)
        assert all(gen.same(ref[k], libm[k]) for k in gen.D_KEYS), c
        gen.add(seen["D"], infos)
    for c in gen.V_RECORDS:
        x, ref, libm, ports, infos, pinfos = v_case(*c)
        assert all(gen.same(ref[k], libm[k]) for k in gen.V_KEYS), c
        gen.add(seen["D"], infos)
        gen.add(seen["V"], pinfos)
    for c in gen.P_RECORDS:
        x, ref, libm, ports, pinfos = p_case(*c)
        assert all(gen.same(ref[k], libm[k]) for k in gen.P_KEYS), c
        gen.add(seen["P"], pinfos)
    assert gen.coverage(seen) == []
    grids, tables = {gen.BIG, gen.SMALL}, set(rv.TABLES)
    assert {(c[0], c[1]) for c in gen.C_RECORDS if c[3] == "default" and c[2] == 5} == {(g, t) for g in grids for t in tables}
    assert any(c[3] == "constant" for c in gen.C_RECORDS) and any(c[2] in (1, 3) for c in gen.C_RECORDS)
    assert {c[:3] for c in gen.D_RECORDS if c[3] == 5 and c[4] is None} == {(g, t, p) for g in grids for t in tables for p in dv.PONDS}
    from tests.test_dedd_host import VARIANTS
    assert {c[4] for c in gen.D_RECORDS if c[4]} == set(VARIANTS) and any(c[3] == 3 for c in gen.D_RECORDS)
    assert {(c[1], c[2]) for c in gen.V_RECORDS} == {(t, li) for t in gen.pv.TABLES for li in (0, 1)}
    assert {(c[2], c[3]) for c in gen.P_RECORDS} == {(fz, dp) for fz in gen.pv.FRZPND for dp in gen.pv.DPSCALES}


def test_spread_table_is_what_the_committed_records_give():
    """SPREAD_MEASURED, from which the GPU test takes its tolerance, recounted: per family and array the largest distance of the
    restatement on PORTS from the reference over the records is the table's entry to its three printed digits, none above 1e-12, and an
    array without an entry is bit-equal in every record"""
    spr = {}
    for c in gen.C_RECORDS:
        gen.spread(c_case(*c)[1], c_case(*c)[3], gen.C_KEYS, spr.setdefault("C", {}))
    for c in gen.D_RECORDS:
        gen.spread(d_case(*c)[1], d_case(*c)[3], gen.D_KEYS, spr.setdefault("D", {}))
    for c in gen.V_RECORDS:
        gen.spread(v_case(*c)[1], v_case(*c)[3], gen.V_KEYS, spr.setdefault("V", {}))
    for c in gen.P_RECORDS:
        gen.spread(p_case(*c)[1], p_case(*c)[3], gen.P_KEYS, spr.setdefault("P", {}))
    for fam, s in spr.items():
        print(fam, {k: float(f"{v:.2e}") for k, v in s.items() if v > 0.0})
        for k, v in s.items():
            want = gen.SPREAD_MEASURED[fam].get(k, 0.0)
            assert (v == 0.0) == (want == 0.0) and abs(v - want) <= 0.01 * want and v < 1.0e-12, (fam, k, v, want)


def test_fixture_sizes():
    """no fixture of this family is larger than the largest ref_itd_* / ref_ridge_* one"""
    paths = [gen.c_path(*c) for c in gen.C_RECORDS] + [gen.d_path(*c) for c in gen.D_RECORDS] + [gen.v_path(*c) for c in gen.V_RECORDS] + \
            [gen.p_path(*c) for c in gen.P_RECORDS]
    assert max(os.path.getsize(p) for p in paths) <= 313333
