"""evpk_step_radiation_dedd on the device against the numpy restatement tests/npdedd.py -- bit for bit, on every cell of every output: the
call writes every cell (zeros where the cell is not listed), so ghost cells, land and the ice-free block are compared too; coszen is in /
out and keeps the caller's bits outside the listed, lit cells.  The kernel uses + - x /, sqrt, comparisons, selects and the fixed-algorithm
exp (dev_exp, whose array port the restatement runs on), and the library is built with -ffp-contract=off.  Parity with the reference:
tests/test_shortwave_ref.py holds the restatement, and tests/test_shortwave_ref_gpu.py the device, to reference-built records of run_dEdd and
below; step_radiation's call order, the aggregation lines of coupling_prep, aerosols and topographic ponds stay unpinned.  Inputs: tests/golden/deddvec.py (no shape larger than 26 x 18 cells); tests/test_dedd_host.py
shows that they take every branch.
"""
import os
import sys
import traceback
import uuid

import numpy as np
import pytest

try:
    import torch          # before libevpk: the process must end up with ONE HIP runtime (torch bundles its own)
    torch.cuda.is_available()
except ImportError:
    torch = None

from cice5_amd import evpk
from tests import nptherm1s
from tests.golden import deddvec as dv
from tests.golden import itdvec as iv
from tests.golden import radvec as rv
from tests.golden import therm1svec as sv
from tests.golden import therm1vec as tv
from tests.test_dedd_host import VARIANTS, restated
from tests.test_rad_host import AI, physical
from tests.test_therm1_gpu import cells, eq, geometry, params
from tests.test_therm1s_gpu import call as call_therm1
from tests.test_therm1s_host import arrays as therm1s_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = "g26x18_b8x5"
ALL = dv.WRITTEN + ["coszen"]


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(cfg):
        if cfg not in made:
            x = restated(cfg, "plain")[0]
            _, d, f = geometry(cfg)
            f["tmask"] = x["tmask"]                 # the land of the inputs
            made[cfg] = evpk.Context(d, f)
            made[cfg].set_params(params(x))
        return made[cfg]
    yield get
    for c in made.values():
        c.close()


def outputs(x, penl=True):
    y = {k: x[k].copy() for k in ALL}
    if not penl:
        y["fswpenln"] = None
    return y


def call(ctx, x, y, **kw):
    g = lambda k: y[k] if k in y else x.get(k)
    a = dict(ntrcr=x["ntrcr"], tracers=x["tracers"])
    a.update({k: x[k] for k in evpk.DEDD_SCALARS})
    a.update(kw)
    return ctx.step_radiation_dedd({k: g(k) for k in evpk.DEDD_STATE}, {k: g(k) for k in evpk.DEDD_FORCING}, g("coszen"),
                                   {k: g(k) for k in dv.WRITTEN}, **a)


def assert_equal(got, want):
    for k in ALL:
        if want.get(k) is None:
            assert got.get(k) is None, k
            continue
        assert eq(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def run_case(ctx, cfg, tcase, pond="cesm", ncat=5, penl=True, **kw):
    """one evpk_step_radiation_dedd against the restatement of the same case, every cell of every array; returns (x, y, want)"""
    x, want, _ = restated(cfg, tcase, pond, ncat, penl, **kw)
    y = outputs(x, penl)
    assert call(ctx, x, y, **kw) is None
    assert_equal(y, want)
    return x, y, want


@pytest.mark.parametrize("cfg", list(dv.CONFIGS))
@pytest.mark.parametrize("tcase", dv.TABLES)
@pytest.mark.parametrize("pond", dv.PONDS)
def test_equals_restatement_on_every_cell(contexts, cfg, tcase, pond):
    """both grids (the second block of each is ice-free), the plain table (k_shortwave_dedd<5, 4, 1>) and the deep one (7 + 2 layers, the
    generic kernel), with tr_pond_cesm and without a pond tracer: equal to the restatement on every cell of every output -- ghost cells,
    land and the ice-free block included -- over outputs pre-filled with non-zero draws; coszen keeps the caller's bits outside the listed
    lit cells and holds max(puny, coszen) on them"""
    x, y, want = run_case(contexts(cfg), cfg, tcase, pond)
    for k in dv.WRITTEN:
        assert (x[k] != 0.0).mean() > 0.99, k                       # (pre-filled with non-zero draws)
    listed = (x["aicen"] > dv.PUNY) & x["ocean"][:, None]
    S = x["swvdr"] + x["swidr"] + x["swvdf"] + x["swidf"]
    lit = listed.any(axis=1) & (S > dv.PUNY)
    assert (x["aicen"][1] == 0.0).all() and y["fswsfcn"][listed].any() and not y["fswsfcn"][~listed].any()
    assert not y["alvdrn"][~listed].any() and not y["snowfracn"][~listed].any()
    assert y["coszen"][~lit].tobytes() == x["coszen"][~lit].tobytes()
    assert eq(y["coszen"][lit], np.where(x["coszen"][lit] > dv.PUNY, x["coszen"][lit], dv.PUNY)) and (x["coszen"][lit] < 0.0).any()


@pytest.mark.parametrize("name", list(VARIANTS) + ["no_fswpenln"])
def test_namelist_and_argument_variants(contexts, name):
    """rsnw_mlt = 3000 and 4 (both ends of the snow table), R_snw = 2, R_ice = -1, R_pnd = -1, hs0 = 0, kalg = 0; fswpenln NULL with every
    other array identical"""
    if name == "no_fswpenln":
        x, y, want = run_case(contexts(CFG), CFG, "plain", penl=False)
        base = restated(CFG, "plain")[1]
        for k in ALL:
            if k != "fswpenln":
                assert eq(y[k], base[k]), k
        return
    x, y, want = run_case(contexts(CFG), CFG, "plain", **VARIANTS[name][0])
    base = restated(CFG, "plain")[1]
    assert any(not eq(y[k], base[k]) for k in dv.WRITTEN)


@pytest.mark.parametrize("ncat,tcase,pond", [(3, "plain", "cesm"), (1, "plain", "none"), (3, "deep", "cesm")])
def test_generic_kernel_with_fewer_categories(contexts, ncat, tcase, pond):
    run_case(contexts(CFG), CFG, tcase, pond, ncat)


def prep_arrays(x, y):
    """the arrays of one evpk_prep_radiation call behind y under the shortwave the step saw"""
    z = {k: (y[k].copy() if y[k] is not None else None) for k in rv.RADIATION + ["scale_factor"]}
    z["fswfac"] = x["fswfac"].copy()
    z.update(aice=x["aice"], aicen=x["aicen"])
    z.update({q: x[q] for q in rv.BANDS})
    z.update({k: y[v] for k, v in AI.items()})
    return z


@pytest.mark.parametrize("tcase", dv.TABLES)
def test_round_trip_with_prep_radiation_is_the_identity(contexts, tcase):
    """evpk_step_radiation_dedd, then evpk_prep_radiation under the same forcing with the aggregated albedos as alvdr_ai ..: netsw /
    scale_factor is exactly 1 wherever scale_factor > puny and aice > 0, and every radiation array is bit for bit unchanged"""
    ctx = contexts(CFG)
    x, want, _ = restated(CFG, tcase)
    y = outputs(x)
    assert call(ctx, x, y) is None
    phys = physical(x)
    acted = phys & (x["aice"] > 0.0) & (y["scale_factor"] > rv.PUNY)
    assert acted.sum() > 20
    z = prep_arrays(x, y)
    tr = x["tracers"]
    assert ctx.prep_radiation(z, nilyr=tr["nilyr"], nslyr=tr["nslyr"]) is None
    assert (z["scale_factor"][phys] == 1.0).all() and (z["fswfac"][phys] == 1.0).all()
    for k in rv.RADIATION:
        assert eq(z[k], y[k]), k
    assert y["Sswabsn"].any()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def test_device_tensors_and_pageable_arrays_agree(contexts):
    ctx = contexts(CFG)
    x, want, _ = restated(CFG, "plain")
    y = outputs(x)
    assert not evpk.host_is_mapped(y["fswsfcn"])
    assert call(ctx, x, y) is None
    dev = {k: _dev(x[k]) for k in dv.STATE + dv.FORCING + ALL}
    assert call(ctx, x, dev) is None
    torch.cuda.synchronize()
    for k in ALL:
        assert eq(dev[k].cpu().numpy(), y[k]), k
    assert_equal(y, want)


def test_chain_on_device_tensors_into_step_therm1(contexts):
    """evpk_step_radiation_dedd -> evpk_step_therm1 on device tensors that never visit the host (no pond tracer: the table of
    step_therm1's own tests), against npdedd -> nptherm1s: the state, the 22 merged planes and the radiation arrays"""
    ctx = contexts(CFG)
    x, w1, _ = restated(CFG, "plain", "none")
    w = therm1s_arrays(x)
    carried = ["fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn"]
    w.update({k: w1[k].copy() for k in carried})
    infos, stop, _ = nptherm1s.step(iv.blocks_of(x["d"]), x["tmask"], nptherm1s.params(x), w)
    assert stop is None
    names64 = sv.WRITTEN + sv.IN2D + ["flw", "potT", "Qa", "rhoa", "fsnow", "sss", "fswthrun"]
    dev = {k: _dev(x[k]) for k in set(names64 + dv.STATE + dv.FORCING + ALL)}
    dev.update({k: _dev(x[k]) for k in evpk.THERM1_MASKS})
    assert call(ctx, x, dev) is None
    assert call_therm1(ctx, x, dev) is None
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    m = x["ocean"]
    for k in tv.STATE + sv.MERGED + ["fswsfcn", "fswintn", "Sswabsn", "Iswabsn"]:
        assert eq(cells(got[k], m), cells(w[k], m)), (k, int((cells(got[k], m) != cells(w[k], m)).sum()))
    for k in ("fswthrun", "fswpenln", "scale_factor", "albpndn", "apeffn", "coszen"):
        assert eq(got[k], w1[k]), k
    assert not eq(got["fswabs"], x["fswabs"]) and not eq(got["vicen"], x["vicen"])            # (step_therm1 went on from there)


def _refused(ctx, x, y, match, **kw):
    with pytest.raises(evpk.EvpkError, match=match):
        call(ctx, x, y, **kw)
    return True


def test_refusals_leave_the_arrays_untouched(contexts):
    ctx = contexts(CFG)
    x, want, _ = restated(CFG, "plain")
    y = outputs(x)
    tr = x["tracers"]
    nb, ncat, ny, nx = x["aicen"].shape
    R = lambda match, xx=x, yy=y, **kw: _refused(ctx, xx, yy, match, **kw)
    R("calc_Tsfc", calc_Tsfc=False)
    R("heat_capacity", heat_capacity=False)
    R("tr_aero", tr_aero=True)
    R("tr_pond_lvl", tracers=dict(tr, tr_pond_cesm=0, tr_pond_lvl=1))
    R("tr_pond_topo", tracers=dict(tr, tr_pond_cesm=0, tr_pond_topo=1))
    R("tr_pond_cesm without nt_apnd", tracers=dict(tr, nt_apnd=0))
    R("tr_pond_cesm without nt_apnd", tracers=dict(tr, nt_hpnd=0))
    R("tr_pond_cesm without nt_apnd", tracers=dict(tr, nt_hpnd=x["ntrcr"] + 1))
    R("nilyr = 9", tracers=dict(tr, nilyr=9))
    R("nilyr = 0", tracers=dict(tr, nilyr=0))
    R("nslyr = 9", tracers=dict(tr, nslyr=9))
    R("nslyr = 0", tracers=dict(tr, nslyr=0))
    R("ncat = 17 not in", xx=dict(x, aicen=np.zeros((nb, 17, ny, nx))))
    R("ncat = 0 not in", xx=dict(x, aicen=np.zeros((nb, 0, ny, nx))))
    R("lies beyond ntrcr", tracers=dict(tr, nt_Tsfc=x["ntrcr"] + 1))
    R("lies beyond ntrcr", tracers=dict(tr, nt_Tsfc=0))
    R("puny = 1e-12", puny=1.0e-12)
    R("dT_mlt = 0", dT_mlt=0.0)
    R("dT_mlt = -1", dT_mlt=-1.0)
    for k in dv.STATE + dv.FORCING:
        R("a required argument is missing", xx=dict(x, **{k: None}))
    for k in ALL:
        if k != "fswpenln":
            R("a required argument is missing", yy=dict(y, **{k: None}))
    for k in ALL:
        assert eq(y[k], x[k]), k
    # evpk_step_radiation keeps refusing the scheme
    from tests.test_rad_gpu import call as call_ccsm3
    from tests.test_rad_host import restated as rad_restated
    xr = rad_restated(CFG, "plain")[0]
    with pytest.raises(evpk.EvpkError, match=r"evpk_step_radiation: shortwave = 'dEdd' \(run_dEdd\) is not supported"):
        call_ccsm3(ctx, xr, {k: xr[k].copy() for k in rv.WRITTEN}, shortwave="dEdd")


def test_refusal_on_more_than_one_rank_before_connect():
    x = restated(CFG, "plain")[0]
    _, d, f = geometry(CFG, nprocs=2, rank=0)
    ctx = evpk.Context(d, f, defer_connect=True)    # (the geometry says two ranks; nothing collective has happened)
    try:
        nb = d.nblocks
        assert nb > 0
        xx = {k: (np.ascontiguousarray(v[:nb]) if isinstance(v, np.ndarray) and v.ndim >= 3 and v.dtype == np.float64 else v) for k, v in x.items()}
        y = outputs(xx)
        with pytest.raises(evpk.EvpkError, match="nranks = 2"):
            call(ctx, xx, y)
        for k in ALL:
            assert eq(y[k], xx[k]), k
    finally:
        ctx.close()


# ---- x-slab ranks: one process per rank on one GPU (the harness of tests/test_rad_gpu.py) ----
def job_dedd(rank, world, tag, tcase):
    d1, d, f = geometry(CFG, world, rank)
    at = {b.block_id: n for n, b in enumerate(d1.local_blocks)}
    loc = [at[b.block_id] for b in d.local_blocks]
    x = dv.dedd_input(CFG, tcase)
    f["tmask"] = np.ascontiguousarray(x["tmask"][loc])
    cut = lambda a: np.ascontiguousarray(a[loc])
    ctx = evpk.Context(d, f, device=0, unique_id=(b"EVPKIPC:" + f"{tag}_0".encode()).ljust(128, b"\0"))
    try:
        ctx.set_params(params(x))
        xx = dict(x, **{k: cut(x[k]) for k in dv.STATE + dv.FORCING})
        y = {k: cut(x[k]) for k in ALL}
        call(ctx, xx, y)
    finally:
        ctx.close()
    return loc, y


def _worker(rank, world, tag, job, args, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["OMP_NUM_THREADS"] = "2"
        q.put((rank, None, globals()[job](rank, world, tag, *args)))
    except Exception:
        q.put((rank, traceback.format_exc(), None))


def _spawn(world, job, args=(), timeout=240):
    import multiprocessing as mp
    assert world <= 3                              # (+ the parent: at most 4 processes hold the GPU)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "evpk_dedd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, world, tag, job, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            rank, err, out = q.get(timeout=timeout)
            assert err is None, f"rank {rank}: {err}"
            res[rank] = out
    finally:
        for p in procs:
            p.join(timeout=1 if len(res) < world else 30)
            if p.is_alive():
                p.kill()
        try:
            os.unlink(f"/dev/shm/{tag}_0")
        except OSError:
            pass
    return [res[r] for r in range(world)]


def test_ranks_equal_the_restatement():
    """three rank processes on one GPU, of which two own block columns and the third owns none: put together, the ranks' blocks equal the
    restatement; the rank without a block column returns 0"""
    tcase = "plain"
    x, want, _ = restated(CFG, tcase)
    outs = _spawn(3, "job_dedd", (tcase,))
    assert [len(loc) > 0 for loc, _ in outs] == [True, True, False]
    seen = sorted(n for loc, _ in outs for n in loc)
    assert seen == list(range(x["aicen"].shape[0]))
    for loc, y in outs[:2]:
        assert_equal(y, {k: want[k][loc] for k in ALL})
    for k in ALL:                                   # the idle rank's (empty) arrays are what it passed
        assert outs[2][1][k].shape[0] == 0
