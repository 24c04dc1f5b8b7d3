"""linear_itd (with fit_line and the boundary integrals), add_new_ice (with update_vertical_tracers and the mushy liquidus), lateral_melt
and reduce_area pinned to the reference's own output (tests/golden/ref_litd_*.npz, ref_therm2_*.npz, made by
tests/golden/make_ref_therm2.py from oracle/_ref/<build>/ref_therm2): the numpy restatements tests/nplitd.py and tests/nptherm2.py
against every fixture record -- bit for bit, NaN-aware: the routines use only + - x / , comparisons and selects, and both sides are built
without fused multiply-add -- stage by stage for step_therm2 (after linear_itd, after add_new_ice, after lateral_melt / reduce_area, after
cleanup_itd), so that a fault cannot hide behind a compensating one downstream; the stop record; and the paths the fixtures must
contain.  No GPU: tests/test_therm2_ref_gpu.py holds the device to the same fixtures.

Still unpinned: step_therm2's call order (the driver restates it), a horizontally non-uniform salinz (include/evpk.h, departure (b)),
aerosols / bgc (refused by the device), l_conservation_check = .true. (compile-time .false. in the reference).
"""
import functools
import os

import numpy as np
import pytest

from tests import nplitd, nptherm2
from tests.golden import make_ref_therm2 as gen
from tests.golden import therm2vec as tv

L_IDS = [f"{c}-{t}-ncat{n}" for c, t, n in gen.L_RECORDS]
T_IDS = [f"{c}-{t}-ncat{n}-kitd{ki}-k{kt}{'-ocnf' if o else ''}" for c, t, n, ki, kt, o in gen.T_RECORDS]


@functools.lru_cache(maxsize=None)
def l_case(cfg, tcase, ncat):
    """(input, fixture, restated record, infos, stop): computed once and shared -- do not modify"""
    x = gen.l_input(cfg, tcase, ncat)
    return (x, np.load(gen.l_path(cfg, tcase, ncat))) + gen.restate_l(x)


@functools.lru_cache(maxsize=None)
def t_case(cfg, tcase, ncat, kitd, ktherm, ocnf):
    """(input, fixture, the reference's four stages, the restatement's four stages, infos, stop): computed once and shared"""
    x = gen.t_input(cfg, tcase, ncat)
    rec = np.load(gen.t_path(cfg, tcase, ncat, kitd, ktherm, ocnf))
    return (x, rec, gen.stages(rec, x)) + gen.restate_t(x, kitd, ktherm, ocnf)


@pytest.mark.parametrize("cfg,tcase,ncat", gen.L_RECORDS, ids=L_IDS)
def test_linear_itd_restatement_equals_the_reference(cfg, tcase, ncat):
    x, ref, got, infos, stop = l_case(cfg, tcase, ncat)
    assert stop is None and not ref["l_stop"].any()
    for k in gen.L_OUT:
        assert gen.same(ref[k], got[k]), (k, int((gen.bits(ref[k]) != gen.bits(got[k])).sum()))
    # what linear_itd leaves in the module for whatever runs after it (ice_therm_itd.F90:208)
    assert float(ref["hin_top"]) == nplitd.HIN_TOP != x["hin_max"][ncat]


@pytest.mark.parametrize("cfg,tcase,ncat,kitd,ktherm,ocnf", gen.T_RECORDS, ids=T_IDS)
def test_step_therm2_restatement_equals_the_reference_stage_by_stage(cfg, tcase, ncat, kitd, ktherm, ocnf):
    x, rec, ref, got, infos, stop = t_case(cfg, tcase, ncat, kitd, ktherm, ocnf)
    assert stop is None and not rec["stop"][:, 0].any()
    assert len(ref) == len(got) == 4
    for name, r, g in zip(gen.STAGES, ref, got):
        for k in tv.OUT:
            assert gen.same(r[k], g[k]), (name, k, int((gen.bits(r[k]) != gen.bits(g[k])).sum()))
    assert float(rec["hin_top"]) == (nplitd.HIN_TOP if kitd == 1 else x["hin_max"][ncat])
    # every stage does something in every record (a stage that changed nothing would be held to nothing)
    changed = [sum(len(rec[f"s{s}_{k}_at"]) for k in tv.OUT) for s in range(1, 5)]
    assert all(c > 0 for c in changed), changed
    if ocnf or ktherm == 2:
        assert len(rec["s2_fresh_at"]) > 0 and len(rec["s2_fsalt_at"]) > 0              # add_new_ice's own flux lines (:1531-1545)


def test_update_ocn_f_and_the_single_category_records_differ_from_their_neighbours():
    """update_ocn_f changes fresh / fsalt and nothing else; the ncat = 1 records end stage 3 in reduce_area"""
    for kt in (1, 2):
        on = t_case("g26x18_b8x5", "plain", 5, 1, kt, True)[2]
        off = t_case("g26x18_b8x5", "plain", 5, 1, kt, False)[2]
        for k in tv.OUT:
            assert gen.same(on[3][k], off[3][k]) == (k not in ("fresh", "fsalt")), (kt, k)
    for c in gen.T_RECORDS:
        if c[2] == 1:
            x, rec, ref, got, infos, stop = t_case(*c)
            tot = {k: sum(i[k] for i in infos) for k in ("reduce_hin", "reduce_dhi", "reduce_none")}
            assert tot["reduce_dhi"] > 0 and (tot["reduce_hin"] > 0) == (x["hin_max"][0] > 0.0), tot


def test_stop_record():
    """reason, lowest block and cell equal stop_expect: the reference stops in cleanup_itd alone, in two blocks; the lowest is reported"""
    st = np.load(os.path.join(gen.HERE, "ref_therm2_stop.npz"))["stop"]
    cfg, tcase, ncat, kitd, ktherm, ocnf = gen.STOP_RECORD
    x = gen.t_input(cfg, tcase, ncat, stop=True)
    assert not st[:, 0, :3].any()
    blocks = np.nonzero(st[:, 0, 3])[0]
    assert len(blocks) == 2
    b = int(blocks[0])
    _, _, stop = gen.restate_t(x, kitd, ktherm, ocnf)
    assert stop == (3,) + x["stop_expect"]                     # (3: cleanup_itd in evpk's stage numbering)
    assert stop[2:] == (b + 1, int(st[b, 1, 3]), int(st[b, 2, 3]))


def test_fixtures_hold_what_they_must():
    """counted from the reference's records and from the info counts of the restatement that equals them bit for bit (asserted above and
    again here): every path of linear_itd over the L records, every path of add_new_ice / lateral_melt over the T records at each ktherm"""
    seen_l = {k: 0 for k in nplitd.INFO_KEYS}
    moved = 0
    for c in gen.L_RECORDS:
        x, ref, got, infos, stop = l_case(*c)
        assert all(gen.same(ref[k], got[k]) for k in gen.L_OUT), c
        for i in infos:
            for k in seen_l:
                seen_l[k] += i[k]
        moved += int((gen.bits(ref["aicen"]) != gen.bits(gen.on_cells(x["aicen"], x["ocean"]))).any(axis=1).sum())
    assert moved > 500
    seen_t = {}
    for ktherm in (1, 2):
        seen = seen_t[ktherm] = {k: 0 for k in nptherm2.INFO_KEYS}
        grown = melted = rebinned = 0
        for c in gen.T_RECORDS:
            if c[4] != ktherm:
                continue
            x, rec, ref, got, infos, stop = t_case(*c)
            assert not gen.differing(ref, got), c
            for i in infos:
                for k in seen:
                    seen[k] += i[k]
            grown += len(rec["s2_aicen_at"])
            melted += len(rec["s3_aicen_at"])
            rebinned += len(rec["s4_aicen_at"])
        assert grown > 500 and melted > 500 and rebinned > 50, (grown, melted, rebinned)
    assert gen.coverage(seen_l, seen_t) == []
    assert all(seen_t[2][k] > 0 for k in gen.MUSHY_ONLY)
    # the pond tables, the table without age / FY / level ice, update_ocn_f, kitd = 0, ncat = 3 and 1
    assert {c[1] for c in gen.T_RECORDS} == set(tv.TRACER_CASES)
    assert {c[2] for c in gen.L_RECORDS} == {5, 3} and {c[2] for c in gen.T_RECORDS} == {5, 1}
    assert any(c[5] for c in gen.T_RECORDS) and any(c[3] == 0 and c[2] == 5 for c in gen.T_RECORDS)


def test_fixture_sizes():
    """no fixture of this family is larger than the largest ref_itd_* / ref_ridge_* one"""
    paths = [gen.l_path(*c) for c in gen.L_RECORDS] + [gen.t_path(*c) for c in gen.T_RECORDS]
    assert max(os.path.getsize(p) for p in paths) <= 313333
