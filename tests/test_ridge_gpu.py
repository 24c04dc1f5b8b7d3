"""evpk_ridge_ice on the device against the numpy restatement tests/npridge.py and the reference fixtures
tests/golden/ref_ridge_*.npz.  Inputs: tests/golden/ridgevec.py (no shape larger than 26 x 18 cells).

Tolerances.  Device against the restatement with the port of the device's exp: bit for bit, every array ridge_ice writes and every
diagnostic (same operations, same order, -ffp-contract=off).  Device against the reference: per array 4 x the spread measured on the
CPU between the restatement with the device's exp and the restatement with libm's (tests/test_ridge_ref.py: spread_bounds(); the
restatement with libm equals the reference bit for bit), as max |a - b| / max |ref| over the listed cells where both take the same
branches; at most 1 % of the listed cells of a record may take another branch and are left out.
"""
import os

import numpy as np
import pytest

from cice5_amd import dyn, evpk, synth
from oracle import orc
from tests import npridge, util
from tests.golden import make_ref_ridge as gen
from tests.golden import ridgevec as rv
from tests.test_ridge_ref import ARRAYS, BRANCH_CAP, GOLDEN, fixture, restated, same_branches, spread_bounds

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
# both configurations, both switch pairs, every tracer table
CASES = [("g26x18_b8x5", "lvl_ponds", "p1r1"), ("g26x18_b8x5", "topo_ponds", "p0r1"), ("g26x18_b8x5", "plain", "p0r1"),
         ("g26x18_b8x5", "cesm_ponds", "p1r1"), ("g24x16_b24x16", "lvl_ponds", "p1r1"), ("g24x16_b24x16", "cesm_ponds", "p0r1")]


def geometry(cfg):
    nx, ny, bx, by, _ = rv.CONFIGS[cfg]
    _, d, f = util.make_case(nx, ny, bx, by)
    f["tmask"] = rv.tmask(cfg, d)               # the land of the fixtures
    return d, f


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(cfg):
        if cfg not in made:
            d, f = geometry(cfg)
            made[cfg] = (evpk.Context(d, f), d, f)
        return made[cfg][0]
    yield get
    for c, _, _ in made.values():
        c.close()


def params(ctx, krdg_partic, krdg_redist=1, ncat=5):
    ctx.set_params(dyn.set_evp_parameters(rv.DT, 4, False, 1.0e4, krdg_partic=krdg_partic, krdg_redist=krdg_redist, ncat=ncat,
                                          mu_rdg=rv.MU_RDG))


def with_sentinel(x):
    """the inputs with every unlisted cell of every in / out array overwritten: ghost cells, land, padding"""
    y = {k: x[k].copy() for k in ARRAYS}
    m = x["listed"]
    for k in ARRAYS:
        a = y[k]
        if a.ndim == 3:
            a[~m] = SENTINEL
        else:
            np.moveaxis(a, (0, -2, -1), (0, 1, 2))[~m] = SENTINEL
    return y


def device_run(ctx, x, y, diag=True, rdg=True):
    dg = {k: y[k] for k in rv.DIAG_2D + rv.DIAG_3D} if diag else None
    return ctx.ridge_ice(x["dt"], x["ndtd"], y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], x["ntrcr"], x["trcr_depend"],
                         x["tracers"], x["hin_max"], x["rdg_conv"] if rdg else None, x["rdg_shear"] if rdg else None, dg)


def assert_bitwise(got, want, m, names=ARRAYS):
    for k in names:
        a, b = gen.on_listed(got[k], m), gen.on_listed(want[k], m)
        neq = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert not neq.any(), (k, int(neq.sum()), float(np.abs(a - b)[neq].max()))


def assert_unlisted_untouched(got, before, m, names=ARRAYS):
    for k in names:
        a, b = got[k], before[k]
        if a.ndim == 3:
            assert np.array_equal(a[~m], b[~m]), k
        else:
            assert np.array_equal(np.moveaxis(a, (0, -2, -1), (0, 1, 2))[~m], np.moveaxis(b, (0, -2, -1), (0, 1, 2))[~m]), k


@pytest.mark.parametrize("cfg,tcase,swn", CASES)
def test_device_equals_restatement_bitwise_and_leaves_unlisted_cells(contexts, cfg, tcase, swn):
    """the ncat = 5 template path: every array and diagnostic on the listed cells; ghost, land and padding cells keep the sentinel"""
    ctx = contexts(cfg)
    sw = rv.SWITCHES[swn]
    params(ctx, sw[0])
    x = rv.ridge_input(cfg, tcase)
    y = with_sentinel(x)
    before = {k: v.copy() for k, v in y.items()}
    assert device_run(ctx, x, y) is None
    want, _, stop = gen.restate(x, sw, exp=npridge.dev_exp)
    assert stop is None
    assert_bitwise(y, want, x["listed"])
    assert_unlisted_untouched(y, before, x["listed"])


def test_generic_path_ncat3_equals_restatement_bitwise(contexts):
    ctx = contexts("g26x18_b8x5")
    params(ctx, 1, ncat=3)
    x = rv.ridge_input("g26x18_b8x5", "lvl_ponds", ncat=3, tag="ncat3")
    y = with_sentinel(x)
    before = {k: v.copy() for k, v in y.items()}
    assert device_run(ctx, x, y) is None
    want, res, stop = gen.restate(x, (1, 1), exp=npridge.dev_exp)
    assert stop is None and sum(r["repeats"] for r in res) >= 1
    assert_bitwise(y, want, x["listed"])
    assert_unlisted_untouched(y, before, x["listed"])


def test_all_diagnostics_null(contexts):
    ctx = contexts("g26x18_b8x5")
    params(ctx, 1)
    x = rv.ridge_input("g26x18_b8x5", "cesm_ponds")
    y = with_sentinel(x)
    before = {k: v.copy() for k, v in y.items()}
    assert device_run(ctx, x, y, diag=False) is None
    want, _, _ = gen.restate(x, (1, 1), exp=npridge.dev_exp)
    assert_bitwise(y, want, x["listed"], rv.STATE)
    for k in rv.DIAG_2D + rv.DIAG_3D:
        assert np.array_equal(y[k], before[k]), k
    assert_unlisted_untouched(y, before, x["listed"], rv.STATE)


@pytest.mark.parametrize("cfg,tcase,swn", CASES)
def test_device_against_the_reference_fixture(contexts, cfg, tcase, swn):
    ctx = contexts(cfg)
    sw = rv.SWITCHES[swn]
    params(ctx, sw[0])
    x = rv.ridge_input(cfg, tcase)
    y = {k: x[k].copy() for k in ARRAYS}
    assert device_run(ctx, x, y) is None
    ref = fixture(cfg, tcase, swn)
    same = same_branches(cfg, tcase, swn)          # (the device takes the branches of the restatement with its exp: the test above)
    assert (~same).sum() <= BRANCH_CAP * same.size
    bounds = spread_bounds()
    for k in ARRAYS:
        a, b = ref[k][same], gen.on_listed(y[k], x["listed"])[same]
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(a - b).max()) / scale if scale > 0 else float(np.abs(a - b).max())
        print(f"{cfg}.{tcase}_{swn} {k}: {err:.3e} (bound {bounds[k]:.3e})")
        assert err <= bounds[k], (k, err, bounds[k])


def test_iteration_is_block_wide(contexts):
    """g26x18_b8x5: in a block that repeats, the cells that were converged after the first pass carry the reference's second-pass
    values, which are not those of a per-cell iteration; a block that does not repeat sees no second pass"""
    cfg, tcase, swn = "g26x18_b8x5", "lvl_ponds", "p1r1"
    ctx = contexts(cfg)
    params(ctx, 1)
    x = rv.ridge_input(cfg, tcase)
    y = {k: x[k].copy() for k in ARRAYS}
    assert device_run(ctx, x, y) is None
    ref = fixture(cfg, tcase, swn)
    _, res = restated(cfg, tcase, swn, "libm")
    percell, _, _ = gen.restate(x, (1, 1), exp=npridge.dev_exp, per_cell_iteration=True)
    blockwide, _, _ = gen.restate(x, (1, 1), exp=npridge.dev_exp)
    m = x["listed"]
    conv = np.zeros(m.shape, dtype=bool)            # converged after pass 1, in a block that repeats
    quiet = np.zeros(m.shape, dtype=bool)           # listed cells of blocks that do not repeat
    for b, r in enumerate(res):
        if ref["repeats"][b] > 0:
            conv[b] = r["conv1"]
        else:
            quiet[b] = m[b]
    assert conv.sum() >= 10 and quiet.sum() >= 10
    same = same_branches(cfg, tcase, swn)
    bounds = spread_bounds()
    lst = lambda a, sel: gen.on_listed(a, m)[sel[m]]
    differs = 0
    for k in ("trcrn", "aparticn", "krdgn"):        # what the second pass rewrites in a converged cell
        got, pc = lst(y[k], conv), lst(percell[k], conv)
        differs += int((got != pc).sum())
        # ... and they are the reference's second-pass values
        ok = same[conv[m]]
        scale = float(np.abs(ref[k]).max())
        assert float(np.abs(ref[k][conv[m]][ok] - got[ok]).max()) / scale <= bounds[k], k
        assert np.array_equal(got, lst(blockwide[k], conv)), k
    assert differs > 0
    for k in ARRAYS:                                # no second pass where the block has converged
        assert np.array_equal(lst(y[k], quiet), lst(percell[k], quiet)), k


def test_resident_deformation_rates_and_evp_undisturbed():
    """after evp, ridge_ice(rdg_conv = None) reads the planes evp left on the device: equal to ridge_ice given the arrays just
    downloaded; and a following evp on the same context still equals the oracle"""
    nx, ny, bx, by, _ = rv.CONFIGS["g26x18_b8x5"]
    case, d, f = util.make_case(nx, ny, bx, by)
    xmin = synth.global_min_dx(case)
    fo, fg = util.clone(f), util.clone(f)
    P = orc.make_params(3600.0, 24, xmin)
    orc.evp(d, P, fo)
    orc.evp(d, P, fo)
    s = dyn.EvpDynamics(d, fg, ndte=24, xmin=xmin, device=0)
    try:
        s.init_evp(3600.0)
        s.evp(3600.0)
        assert np.count_nonzero(fg["rdg_conv"]) > 0 and np.count_nonzero(fg["rdg_shear"]) > 0
        x = rv.ridge_input("g26x18_b8x5", "lvl_ponds", tag="resident")
        x["rdg_conv"], x["rdg_shear"] = fg["rdg_conv"].copy(), fg["rdg_shear"].copy()
        y1 = {k: x[k].copy() for k in ARRAYS}
        y2 = {k: x[k].copy() for k in ARRAYS}
        assert device_run(s.ctx, x, y1, rdg=False) is None
        assert device_run(s.ctx, x, y2, rdg=True) is None
        for k in ARRAYS:
            assert np.array_equal(y1[k], y2[k], equal_nan=True), k
        assert not np.array_equal(y1["aicen"], x["aicen"])
        s.evp(3600.0)
    finally:
        s.close()
    assert util.compare(d, fg, fo) == []


@pytest.mark.parametrize("name", list(rv.STOPS))
def test_stop_codes_and_cells(contexts, name):
    ref = np.load(os.path.join(GOLDEN, "ref_ridge_stops.npz"))[name]
    ctx = contexts("g24x16_b24x16")
    params(ctx, 1)
    x = rv.stop_input(name)
    y = {k: x[k].copy() for k in ARRAYS}
    stop = device_run(ctx, x, y)
    assert stop == (rv.STOPS[name]["reason"], 1, int(ref[1]), int(ref[2]))


def test_refusals(contexts):
    ctx = contexts("g26x18_b8x5")
    x = rv.ridge_input("g26x18_b8x5", "plain")
    y = {k: x[k].copy() for k in ARRAYS}
    params(ctx, 1, krdg_redist=0)
    with pytest.raises(evpk.EvpkError, match="krdg_redist = 0"):
        device_run(ctx, x, y)
    params(ctx, 1)
    nb, ncat, _, nyb, nxb = x["trcrn"].shape
    x33 = dict(x, ntrcr=33, trcr_depend=np.zeros(33, dtype=np.int32))
    y33 = dict(y, trcrn=np.zeros((nb, ncat, 33, nyb, nxb)))
    with pytest.raises(evpk.EvpkError, match="ntrcr = 33 exceeds 32"):
        device_run(ctx, x33, y33)
    for k in ARRAYS:                                # a refused call touches nothing
        assert np.array_equal(y[k], x[k]), k


def test_refusal_on_more_than_one_rank():
    nx, ny, bx, by, _ = rv.CONFIGS["g26x18_b8x5"]
    _, d, f = util.make_case(nx, ny, bx, by, nprocs=2, rank=0)
    ctx = evpk.Context(d, f, defer_connect=True)    # (the geometry says two ranks; nothing collective has happened)
    try:
        nb, nyb, nxb = d.nblocks, d.ny_block, d.nx_block
        z = lambda *s: np.zeros(s)
        with pytest.raises(evpk.EvpkError, match="nranks = 2"):
            ctx.ridge_ice(3600.0, 1, z(nb, nyb, nxb), z(nb, 5, nyb, nxb), z(nb, 5, nyb, nxb), z(nb, 5, nyb, nxb), z(nb, 5, 1, nyb, nxb), 1,
                          [0], {}, rv.HIN_MAX, z(nb, nyb, nxb), z(nb, nyb, nxb))
    finally:
        ctx.close()
