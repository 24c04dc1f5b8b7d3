"""The committed fixtures tests/golden/ref_*.npz are what the generators make today: each tests/golden/make_ref_*.py writes its family
again, into a scratch directory, from the oracle/_ref programs that __graft_entry__.build() left, and every array has to come out with
the committed key, dtype, shape and bytes, with no file missing or extra.  CPU; skipped where the reference, amdflang or the oracle/_ref
programs are absent (the GPU box).  Only the programs and the committed fixtures are read, never the reference tree."""
import fnmatch
import importlib
import os

import numpy as np
import pytest

from tests import refcompile as R
from tests.golden import itdvec, make_ref_shortwave, make_ref_therm2, refrun, refvec, ridgevec

# generator -> (the names of its fixtures, the program it runs, the builds of that program)
FAMILIES = {
    "make_ref_golden": ([f"ref_{cfg}.npz" for cfg in refvec.CONFIGS], "ref_harness", refvec.CONFIGS),
    "make_ref_kernels": (["ref_dyn_*.npz"], "ref_kernels", refvec.KERNEL_CONFIGS),
    "make_ref_remap": (["ref_remap_*.npz"], "ref_remap", refvec.KERNEL_CONFIGS),
    "make_ref_ridge": (["ref_ridge_*.npz"], "ref_ridge", ridgevec.CONFIGS),
    "make_ref_itd": (["ref_itd_*.npz"], "ref_itd", itdvec.CONFIGS),
    "make_ref_therm2": (["ref_litd_*.npz", "ref_therm2_*.npz"], "ref_therm2", make_ref_therm2.BUILDS),
    "make_ref_shortwave": (["ref_sw_*.npz"], "ref_shortwave", make_ref_shortwave.BUILDS),
}
EXES = [refrun.exe(program, cfg) for _, program, cfgs in FAMILIES.values() for cfg in cfgs]
pytestmark = pytest.mark.skipif(not (os.path.isdir(R.REF) and os.path.exists(R.FC) and all(os.path.exists(e) for e in EXES)),
                                reason="needs /root/reference, amdflang and the oracle/_ref programs (this container only)")


def committed(name):
    return sorted(f for f in os.listdir(refrun.HERE) if any(fnmatch.fnmatch(f, pat) for pat in FAMILIES[name][0]))


def test_every_committed_fixture_belongs_to_one_generator():
    owned = [f for name in FAMILIES for f in committed(name)]
    assert sorted(owned) == sorted(f for f in os.listdir(refrun.HERE) if fnmatch.fnmatch(f, "ref_*.npz"))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_generator_reproduces_its_committed_fixtures(name, tmp_path, monkeypatch):
    monkeypatch.setattr(refrun, "build", lambda program, cfg, dims, ncat: refrun.exe(program, cfg))      # run what build() left: no make here
    importlib.import_module("tests.golden." + name).main(str(tmp_path))
    want = committed(name)
    assert want and sorted(os.listdir(tmp_path)) == want
    for f in want:
        with np.load(os.path.join(refrun.HERE, f)) as a, np.load(os.path.join(tmp_path, f)) as b:
            assert sorted(b.files) == sorted(a.files), f
            for k in a.files:
                assert (b[k].dtype, b[k].shape) == (a[k].dtype, a[k].shape) and b[k].tobytes() == a[k].tobytes(), (f, k)
