"""evpk_linear_itd, evpk_new_ice_lateral_melt and evpk_step_therm2 on the device, compared DIRECTLY with the reference's own output
(tests/golden/ref_litd_*.npz, ref_therm2_*.npz; tests/golden/make_ref_therm2.py) on the physical ocean cells -- bit for bit, NaN-aware:
the routines use only + - x / , comparisons and selects, and both sides are built without fused multiply-add.  The restatements are
not consulted; tests/test_therm2_ref.py holds them to the same fixtures on the CPU.  Reads tests/golden/ only.

evpk_new_ice_lateral_melt is fed the reference's state after linear_itd, so that it is held to the reference on its own; with rside = 0
it is add_new_ice alone (the reference's state after add_new_ice), with frzmlt = 0 on that state lateral_melt alone.
"""
import os

import numpy as np
import pytest

try:
    import torch          # before libevpk: the process must end up with ONE HIP runtime (torch bundles its own)
    torch.cuda.is_available()
except ImportError:
    torch = None

from cice5_amd import evpk
from tests.golden import make_ref_therm2 as gen
from tests.golden import therm2vec as tv
from tests.test_therm2_gpu import contexts, eq, leads, outputs, step          # noqa: F401  (contexts: the module-scoped fixture)
from tests.test_therm2_ref import L_IDS, T_IDS

pytestmark = pytest.mark.gpu

NUMERIC = [k for k in tv.OUT if k != "first_ice"]
_inputs = {}


def t_input(cfg, tcase, ncat):
    """computed once per case, shared, not modified"""
    key = (cfg, tcase, ncat)
    if key not in _inputs:
        _inputs[key] = gen.t_input(cfg, tcase, ncat)
    return _inputs[key]


def t_stages(x, c):
    return gen.stages(np.load(gen.t_path(*c)), x)


def put(x, y, one, keys):
    """the record `one` (ocean cells) into the block arrays y"""
    for k in keys:
        if y[k].ndim == 3:
            y[k][x["ocean"]] = one[k]
        else:
            np.moveaxis(y[k], (0, -2, -1), (0, 1, 2))[x["ocean"]] = one[k]


def assert_equals_record(x, y, one, keys, what):
    for k in keys:
        got = gen.on_cells(y[k], x["ocean"])
        assert eq(got, one[k]), (what, k, int((gen.bits(np.asarray(got, dtype=one[k].dtype)) != gen.bits(one[k])).sum()))


@pytest.mark.parametrize("cfg,tcase,ncat", gen.L_RECORDS, ids=L_IDS)
def test_linear_itd_equals_the_reference_fixture(contexts, cfg, tcase, ncat):
    ctx = contexts(cfg)
    x = gen.l_input(cfg, tcase, ncat)
    ref = np.load(gen.l_path(cfg, tcase, ncat))
    y = {k: x[k].copy() for k in gen.L_OUT}
    stop = ctx.linear_itd(x["aicen_init"], x["vicen_init"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["aice0"], x["ntrcr"],
                          x["trcr_depend"], x["tracers"], x["hin_max"], x["hi_min"], x["k"], y["fpond"])
    assert stop is None and not ref["l_stop"].any()
    assert_equals_record(x, y, ref, gen.L_OUT, "linear_itd")


@pytest.mark.parametrize("cfg,tcase,ncat,kitd,ktherm,ocnf", gen.T_RECORDS, ids=T_IDS)
def test_new_ice_lateral_melt_equals_the_reference_fixture(contexts, cfg, tcase, ncat, kitd, ktherm, ocnf):
    ctx = contexts(cfg)
    x = t_input(cfg, tcase, ncat)
    after_litd, after_new_ice, after_melt, _ = t_stages(x, (cfg, tcase, ncat, kitd, ktherm, ocnf))
    # from the reference's state after linear_itd to its state after lateral_melt / reduce_area
    y = outputs(x)
    put(x, y, after_litd, NUMERIC)
    leads(ctx, x, y, ktherm, update_ocn_f=ocnf)
    assert_equals_record(x, y, after_melt, NUMERIC, "add_new_ice + lateral_melt")
    if ncat > 1:                                               # (ncat = 1 ends in reduce_area whatever rside is)
        # add_new_ice alone: no cell melts laterally
        y = outputs(x)
        put(x, y, after_litd, NUMERIC)
        leads(ctx, dict(x, rside=np.zeros_like(x["rside"])), y, ktherm, update_ocn_f=ocnf)
        assert_equals_record(x, y, after_new_ice, NUMERIC, "add_new_ice")
    # lateral_melt alone: no cell freezes (add_new_ice then sets frazil = 0 and adds 0 to the fluxes)
    y = outputs(x)
    put(x, y, after_new_ice, NUMERIC)
    leads(ctx, dict(x, frzmlt=np.zeros_like(x["frzmlt"])), y, ktherm, update_ocn_f=ocnf)
    assert_equals_record(x, y, after_melt, [k for k in NUMERIC if k != "frazil"], "lateral_melt")
    assert not gen.on_cells(y["frazil"], x["ocean"]).any()


@pytest.mark.parametrize("cfg,tcase,ncat,kitd,ktherm,ocnf", gen.T_RECORDS, ids=T_IDS)
def test_step_therm2_equals_the_reference_fixture(contexts, cfg, tcase, ncat, kitd, ktherm, ocnf):
    ctx = contexts(cfg)
    x = t_input(cfg, tcase, ncat)
    final = t_stages(x, (cfg, tcase, ncat, kitd, ktherm, ocnf))[3]
    y = outputs(x)
    assert step(ctx, x, y, kitd, ktherm, update_ocn_f=ocnf) is None
    assert_equals_record(x, y, final, tv.OUT, "step_therm2")


def test_stop_equals_the_reference_record(contexts):
    """stage, reason, lowest block and cell; the reference stops in cleanup_itd alone"""
    cfg, tcase, ncat, kitd, ktherm, ocnf = gen.STOP_RECORD
    st = np.load(os.path.join(gen.HERE, "ref_therm2_stop.npz"))["stop"]
    x = gen.t_input(cfg, tcase, ncat, stop=True)
    b = int(np.nonzero(st[:, 0, 3])[0][0])
    assert not st[:, 0, :3].any()
    got = step(contexts(cfg), x, outputs(x), kitd, ktherm, update_ocn_f=ocnf)
    assert got == (evpk.ITD_STOP, 3) + x["stop_expect"]
    assert got[3:] == (b + 1, int(st[b, 1, 3]), int(st[b, 2, 3]))
