"""evpk_step_radiation, evpk_step_radiation_dedd and evpk_step_radiation_dedd_lvl on the device, compared DIRECTLY with the reference's own
output (tests/golden/ref_sw_c_*.npz, ref_sw_d_*.npz, ref_sw_v_*.npz; tests/golden/make_ref_shortwave.py) on the physical ocean cells.  The
restatements are not consulted; tests/test_shortwave_ref.py holds them to the same fixtures on the CPU.  Reads tests/golden/ only.

The device computes exp and atan with its own fixed algorithm, so it differs from the reference in the last bits wherever those enter.
Per array the tolerance is FOUR TIMES make_ref_shortwave.SPREAD_MEASURED: the largest distance, over the records of the family, of the
restatement on the ports of the device's math from the reference record, relative to the array's largest magnitude in the record (at most
6.4e-14, measured on the CPU and recounted by tests/test_shortwave_ref.py; the device is held bit-equal to that restatement by
tests/test_rad_gpu.py, test_dedd_gpu.py and test_pondlvl_gpu.py, so this is the distance it shows).  An array without an entry is asserted
bit for bit, and so -- on their own -- are the arrays and cells through which no exp / atan flows: snowfracn, apeffn, apeff_ai, the
coszen the call returns and dhsn; under albedo_type = 'constant' the albedos and what is built from them alone; every output of the dEdd
calls and the radiation arrays of the ccsm3 call on night cells; every zero of the reference.

The dEdd calls are fed the coszen the reference's compute_coszen returned (coszen_in of the record): compute_coszen stays with the caller.
Still unpinned: see tests/test_shortwave_ref.py.
"""
import numpy as np
import pytest

try:
    import torch          # before libevpk: the process must end up with ONE HIP runtime (torch bundles its own)
    torch.cuda.is_available()
except ImportError:
    torch = None

from tests.golden import deddvec as dv
from tests.golden import make_ref_shortwave as gen
from tests.golden import radvec as rv
from tests.test_dedd_gpu import call as call_dedd
from tests.test_dedd_gpu import contexts          # noqa: F401  (the module-scoped fixture)
from tests.test_dedd_gpu import outputs as dedd_outputs
from tests.test_pondlvl_gpu import call_sw
from tests.test_pondlvl_host import SW_ALL
from tests.test_rad_gpu import call as call_ccsm3
from tests.test_rad_gpu import outputs as rad_outputs
from tests.test_shortwave_ref import C_IDS, D_IDS, V_IDS, count, night

pytestmark = pytest.mark.gpu

FACTOR = 4.0
_inputs = {}


def shared(key, make):
    """inputs computed once per case, shared, not modified"""
    if key not in _inputs:
        _inputs[key] = make()
    return _inputs[key]


def assert_equals_record(x, y, ref, keys, fam, exact, night_keys, what):
    dark = night(x)
    assert dark.sum() > 50
    for k in keys:
        got = gen.on_cells(y[k], x["ocean"])
        r = ref[k]
        bound = 0.0 if k in exact else gen.SPREAD_MEASURED[fam].get(k, 0.0)
        if bound == 0.0 or not r.any():
            assert gen.same(r, got), (what, k, "bit for bit", count(r, got))
        else:
            assert np.array_equal(np.isnan(r), np.isnan(got)), (what, k)
            scale = float(np.abs(r).max())
            err = float(np.abs(got - r).max())
            print(f"{what} {k}: {err / scale:.2e} of {FACTOR * bound:.2e}")
            assert err <= FACTOR * bound * scale, (what, k, err / scale, bound, int((np.abs(got - r) > FACTOR * bound * scale).sum()))
        if k in night_keys:
            assert gen.same(r[dark], got[dark]), (what, "night", k, count(r[dark], got[dark]))
        zero = r == 0.0
        assert not got[zero].any(), (what, "zeros", k, int((got[zero] != 0.0).sum()))


@pytest.mark.parametrize("cfg,tcase,ncat,atype", gen.C_RECORDS, ids=C_IDS)
def test_step_radiation_equals_the_reference_fixture(contexts, cfg, tcase, ncat, atype):
    x = shared(("C", cfg, tcase, ncat), lambda: gen.c_input(cfg, tcase, ncat))
    ref = np.load(gen.c_path(cfg, tcase, ncat, atype))
    y = rad_outputs(x)
    assert call_ccsm3(contexts(cfg), x, y, albedo_type=atype) is None
    exact = gen.EXACT_CONSTANT if atype == "constant" else []
    assert_equals_record(x, y, ref, gen.C_KEYS, "C", exact, rv.RADIATION, "step_radiation")


@pytest.mark.parametrize("cfg,tcase,pond,ncat,variant", gen.D_RECORDS, ids=D_IDS)
def test_step_radiation_dedd_equals_the_reference_fixture(contexts, cfg, tcase, pond, ncat, variant):
    from tests.test_dedd_host import VARIANTS
    x0 = shared(("D", cfg, tcase, pond, ncat), lambda: gen.d_input(cfg, tcase, pond, ncat))
    ref = np.load(gen.d_path(cfg, tcase, pond, ncat, variant))
    x = gen.with_coszen(x0, ref)
    y = dedd_outputs(x)
    assert call_dedd(contexts(cfg), x, y, **(VARIANTS[variant][0] if variant else {})) is None
    assert_equals_record(x, y, ref, gen.D_KEYS, "D", ["snowfracn", "apeffn", "apeff_ai", "coszen"], dv.WRITTEN, "step_radiation_dedd")


@pytest.mark.parametrize("cfg,tcase,linitonly", gen.V_RECORDS, ids=V_IDS)
def test_step_radiation_dedd_lvl_equals_the_reference_fixture(contexts, cfg, tcase, linitonly):
    x0 = shared(("V", cfg, tcase), lambda: gen.v_input(cfg, tcase))
    ref = np.load(gen.v_path(cfg, tcase, linitonly))
    x = gen.with_coszen(x0, ref)
    y = {k: x[k].copy() for k in SW_ALL}
    assert call_sw(contexts(cfg), x, y, linitonly) is None
    assert_equals_record(x, y, ref, gen.V_KEYS, "V", ["snowfracn", "apeffn", "apeff_ai", "coszen", "dhsn"], dv.WRITTEN, "step_radiation_dedd_lvl")
