"""evpk_linear_itd on the device against the numpy restatement tests/nplitd.py -- bit for bit: the routines use only + - x / , comparisons
and selects, the library is built with -ffp-contract=off.  Parity with the reference is pinned: the restatement equals the reference's
own compiled linear_itd, fit_line and the boundary integrals included (tests/test_therm2_ref.py), and tests/test_therm2_ref_gpu.py
compares the device with those records directly; shift_ice / compute_tracers are pinned by tests/test_itd_ref.py as well.
Inputs: tests/golden/litdvec.py (no shape larger than 26 x 18 cells); tests/test_litd_host.py shows that they take every branch.

No stop case: linear_itd's own donor rules keep every transfer inside shift_ice's checks (tests/test_litd_host.py, include/evpk.h).
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

from cice5_amd import blocks, constants as C
from cice5_amd import dyn, evpk, synth
from tests import npitd
from tests.golden import itdvec as iv
from tests.golden import litdvec as lv
from tests.test_litd_host import OUT, restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
BCASE = "cyclic_open"


def geometry(cfg, nprocs=1, rank=0):
    """the context arguments of one rank and the whole-domain decomposition"""
    nx, ny, bx, by, _ = lv.CONFIGS[cfg]
    ew, ns, _ = iv.BOUNDS[BCASE]
    d1 = blocks.create_distrb_cart(nx, ny, bx, by, ew_boundary_type=ew, ns_boundary_type=ns)
    d = d1 if nprocs == 1 else blocks.create_distrb_cart(nx, ny, bx, by, nprocs=nprocs, rank=rank, ew_boundary_type=ew, ns_boundary_type=ns)
    f = synth.make_block_fields(synth.SynthCase(nx=nx, ny=ny, ew_boundary=C.BND_NAMES[ew], ns_boundary=C.BND_NAMES[ns]), d)
    return d1, d, f


def params():
    return dyn.set_evp_parameters(3600.0, 4, False, 1.0e4, ncat=5)


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(cfg):
        if cfg not in made:
            x = lv.litd_input(cfg, "plain", quiet=True)
            _, d, f = geometry(cfg)
            f["tmask"] = x["tmask"]                 # the land of the inputs
            made[cfg] = evpk.Context(d, f)
            made[cfg].set_params(params())
        return made[cfg]
    yield get
    for c in made.values():
        c.close()


_inputs = {}


def inputs(cfg, tcase, ncat=5):
    """(x, restated arrays, infos): computed once per case, shared, not modified"""
    key = (cfg, tcase, ncat)
    if key not in _inputs:
        x = lv.litd_input(cfg, tcase, ncat=ncat)
        y, infos, stop = restate(x)
        assert stop is None
        _inputs[key] = (x, y, infos)
    return _inputs[key]


def call(ctx, x, y, fpond=True, **kw):
    a = dict(ntrcr=x["ntrcr"], trcr_depend=x["trcr_depend"], tracers=x["tracers"], hin_max=x["hin_max"], hi_min=x["hi_min"], constants=x["k"])
    a.update(kw)
    return ctx.linear_itd(x["aicen_init"], x["vicen_init"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["aice0"], a["ntrcr"],
                          a["trcr_depend"], a["tracers"], a["hin_max"], a["hi_min"], a["constants"], y["fpond"] if fpond else None)


def eq(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def cells(a, m):
    """a[..., cells of m] with the block axis first"""
    return np.moveaxis(a, (0, -2, -1), (0, 1, 2))[m]


def assert_equals_restatement(x, got, want, topo):
    m = x["ocean"]
    for k in iv.STATE + (["fpond"] if topo else []):
        if got[k] is not None:
            assert eq(cells(got[k], m), cells(want[k], m)), (k, int((cells(got[k], m) != cells(want[k], m)).sum()))
    for k in ("aice", "aice0"):
        assert eq(got[k], want[k]), k


@pytest.mark.parametrize("cfg", list(lv.CONFIGS))
@pytest.mark.parametrize("tcase", list(lv.TRACER_CASES))
def test_equals_restatement_and_leaves_land_ghost_and_idle_blocks(contexts, cfg, tcase):
    """both grids, all pond tables, ncat = 5: physical ocean cells equal the restatement, aice / aice0 on every cell; land, ghost and
    padding cells of the state and every cell of the block without a listed cell keep a sentinel"""
    ctx = contexts(cfg)
    x, want, infos = inputs(cfg, tcase)
    y = {k: x[k].copy() for k in OUT}
    idle = np.array([not i["listed"] for i in infos])
    assert idle.any() and not idle.all()
    keep = ~x["ocean"] | idle[:, None, None]
    for k in ("trcrn",):                              # (aicen of the idle block is read by aggregate_area: it stays 0 there)
        cells(y[k], keep)[...] = SENTINEL
    for k in ("aicen", "vicen", "vsnon"):
        cells(y[k], ~x["ocean"] & ~idle[:, None, None])[...] = SENTINEL
    before = {k: y[k].copy() for k in iv.STATE}
    topo = bool(x["tracers"].get("tr_pond_topo"))
    assert call(ctx, x, y) is None
    live = x["ocean"] & ~idle[:, None, None]
    for k in iv.STATE + (["fpond"] if topo else []):
        assert eq(cells(y[k], live), cells(want[k], live)), (k, int((cells(y[k], live) != cells(want[k], live)).sum()))
    for k in iv.STATE:
        assert eq(cells(y[k], keep), cells(before[k], keep)), k
    if not topo:
        assert eq(y["fpond"], x["fpond"])
    # aice / aice0 on every cell: the sums of the aicen the call was given where it writes none
    a = np.zeros_like(y["aice"])
    for n in range(x["ncat"]):
        a = a + before["aicen"][:, n]
    a[live] = want["aice"][live]
    assert eq(y["aice"], a) and eq(y["aice0"], np.maximum(1.0 - a, 0.0))


@pytest.mark.parametrize("ncat", [3, 1])
def test_generic_path(contexts, ncat):
    ctx = contexts("g26x18_b8x5")
    x, want, infos = inputs("g26x18_b8x5", "lvl_ponds", ncat)
    assert sum(i["listed"] for i in infos) > 100 and (ncat == 1 or sum(i["up"] for i in infos) and sum(i["down"] for i in infos))
    y = {k: x[k].copy() for k in OUT}
    assert call(ctx, x, y) is None
    assert_equals_restatement(x, y, want, False)


def test_no_tracers_and_no_fpond(contexts):
    """ntrcr = 0 with trcrn = NULL, fpond = NULL without topo ponds"""
    ctx = contexts("g26x18_b8x5")
    x0, _, _ = inputs("g26x18_b8x5", "plain")
    x = dict(x0, ntrcr=0, trcr_depend=np.zeros(0, dtype=np.int32), tracers={}, trcrn=np.zeros(x0["trcrn"].shape[:2] + (0,) + x0["trcrn"].shape[3:]))
    want, infos, stop = restate(x)
    assert stop is None
    y = dict({k: x[k].copy() for k in ("aicen", "vicen", "vsnon", "aice", "aice0")}, trcrn=None, fpond=None)
    assert call(ctx, x, y, fpond=False) is None
    assert_equals_restatement(x, y, want, False)
    x1, want1, _ = inputs("g26x18_b8x5", "cesm_ponds")
    y = {k: x1[k].copy() for k in OUT}
    assert call(ctx, x1, y, fpond=False) is None
    assert_equals_restatement(x1, y, want1, False)


def test_device_pointers_and_pageable_arrays_agree(contexts):
    ctx = contexts("g26x18_b8x5")
    x, want, _ = inputs("g26x18_b8x5", "topo_ponds")
    y = {k: x[k].copy() for k in OUT}
    assert not evpk.host_is_mapped(y["aicen"])
    assert call(ctx, x, y) is None
    dev = {k: torch.from_numpy(x[k].copy()).cuda() for k in OUT + ["aicen_init", "vicen_init"]}
    assert call(ctx, dict(x, aicen_init=dev["aicen_init"], vicen_init=dev["vicen_init"]), dev) is None
    torch.cuda.synchronize()
    for k in OUT:
        assert eq(dev[k].cpu().numpy(), y[k]), k
    assert_equals_restatement(x, y, want, True)


def test_linear_itd_then_cleanup_itd_on_the_device(contexts):
    """the chain a host runs: linear_itd -> cleanup_itd without the state leaving the device equals nplitd -> npitd.cleanup_itd"""
    ctx = contexts("g26x18_b8x5")
    x, want, _ = inputs("g26x18_b8x5", "lvl_ponds")
    names = OUT + ["aicen_init", "vicen_init", "fresh", "fsalt", "fhocn", "first_ice"]
    dev = {k: torch.from_numpy(x[k].copy()).cuda() for k in names}
    assert call(ctx, dict(x, aicen_init=dev["aicen_init"], vicen_init=dev["vicen_init"]), dev) is None
    fl = {k: dev[k] for k in iv.FLUX}
    assert ctx.cleanup_itd(x["dt"], dev["aicen"], dev["vicen"], dev["vsnon"], dev["trcrn"], dev["aice0"], dev["aice"], x["ntrcr"], x["trcr_depend"],
                           x["tracers"], x["hin_max"], x["k"], fl, dev["first_ice"]) is None
    torch.cuda.synchronize()
    z = {k: want[k].copy() for k in OUT}
    z.update({k: x[k].copy() for k in ("fresh", "fsalt", "fhocn", "first_ice")})
    # (land: the reference zeroes the tracers of land cells in a block that shifts, the device leaves them: compare ocean cells)
    _, stop = npitd.cleanup_itd(iv.blocks_of(x["d"]), x["dt"], x["ntrcr"], x["trcr_depend"], x["tracers"], x["hin_max"], x["k"], z["aicen"],
                                z["vicen"], z["vsnon"], z["trcrn"], z["aice0"], z["aice"], {k: z[k] for k in iv.FLUX}, z["first_ice"])
    assert stop is None
    m = x["ocean"]
    for k in iv.STATE + iv.FLUX + ["aice", "aice0", "first_ice"]:
        g = dev[k].cpu().numpy()
        assert np.array_equal(cells(g, m), cells(z[k], m)), k


def test_refusals_leave_the_arrays_untouched(contexts):
    ctx = contexts("g26x18_b8x5")
    x, _, _ = inputs("g26x18_b8x5", "topo_ponds")
    y = {k: x[k].copy() for k in OUT}
    nb, ncat, nt, ny, nx = x["trcrn"].shape
    z = lambda *s: np.zeros(s)
    with pytest.raises(evpk.EvpkError, match="a required argument is missing"):
        call(ctx, x, dict(y, aice0=None))
    with pytest.raises(evpk.EvpkError, match="a required argument is missing"):
        call(ctx, x, dict(y, trcrn=None))
    with pytest.raises(evpk.EvpkError, match="a required argument is missing"):
        call(ctx, dict(x, vicen_init=None), y)
    with pytest.raises(evpk.EvpkError, match="ncat = 17 not in"):
        ctx.linear_itd(z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, 1, ny, nx),
                       z(nb, ny, nx), z(nb, ny, nx), 1, [0], dict(nt_Tsfc=1), np.zeros(18), 0.01)
    with pytest.raises(evpk.EvpkError, match="ntrcr = 33 exceeds 32"):
        call(ctx, x, dict(y, trcrn=z(nb, ncat, 33, ny, nx)), ntrcr=33, trcr_depend=np.zeros(33, dtype=np.int32))
    with pytest.raises(evpk.EvpkError, match="puny = 1e-12"):
        call(ctx, x, y, constants=dict(x["k"], puny=1.0e-12))
    with pytest.raises(evpk.EvpkError, match="tr_pond_topo needs fpond"):
        call(ctx, x, y, fpond=False)
    with pytest.raises(evpk.EvpkError, match="nt_Tsfc is required"):
        call(ctx, x, y, tracers=dict(x["tracers"], nt_Tsfc=0))
    for k in OUT:
        assert eq(y[k], x[k]), k


def test_refusal_on_more_than_one_rank_before_connect():
    _, d, f = geometry("g26x18_b8x5", nprocs=2, rank=0)
    ctx = evpk.Context(d, f, defer_connect=True)    # (the geometry says two ranks; nothing collective has happened)
    try:
        nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
        z = lambda *s: np.zeros(s)
        with pytest.raises(evpk.EvpkError, match="nranks = 2"):
            ctx.linear_itd(z(nb, 5, ny, nx), z(nb, 5, ny, nx), z(nb, 5, ny, nx), z(nb, 5, ny, nx), z(nb, 5, ny, nx), z(nb, 5, 1, ny, nx),
                           z(nb, ny, nx), z(nb, ny, nx), 1, [0], dict(nt_Tsfc=1), iv.ridgevec.HIN_MAX, 0.01)
    finally:
        ctx.close()


# ---- x-slab ranks: one process per rank on one GPU (the harness of tests/test_step_dyn_multirank_gpu.py) ----
CFG = "g26x18_b8x5"


def job_litd(rank, world, tag, tcase):
    d1, d, f = geometry(CFG, world, rank)
    at = {b.block_id: n for n, b in enumerate(d1.local_blocks)}
    loc = [at[b.block_id] for b in d.local_blocks]
    x = lv.litd_input(CFG, tcase)
    f["tmask"] = np.ascontiguousarray(x["tmask"][loc])
    cut = lambda a: np.ascontiguousarray(a[loc])
    ctx = evpk.Context(d, f, device=0, unique_id=(b"EVPKIPC:" + f"{tag}_0".encode()).ljust(128, b"\0"))
    try:
        ctx.set_params(params())
        y = {k: cut(x[k]) for k in OUT}
        stop = call(ctx, dict(x, aicen_init=cut(x["aicen_init"]), vicen_init=cut(x["vicen_init"])), y)
    finally:
        ctx.close()
    return loc, y, stop


def _worker(rank, world, tag, job, args, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["OMP_NUM_THREADS"] = "2"
        q.put((rank, None, globals()[job](rank, world, tag, *args)))
    except Exception:
        q.put((rank, traceback.format_exc(), None))


def _spawn(world, job, args=(), timeout=240):
    import multiprocessing as mp
    assert world <= 5                              # (+ the parent: at most 6 processes hold the GPU)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "evpk_litd_" + uuid.uuid4().hex[:12]
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


def test_ranks_equal_the_one_rank_result(contexts):
    """three rank processes on one GPU, of which two own block columns (16 and 10 columns wide) and the third owns none: put together,
    the ranks' blocks equal the one-rank device result on every element; the rank without a block column returns 0"""
    tcase = "topo_ponds"
    x, _, _ = inputs(CFG, tcase)
    one = {k: x[k].copy() for k in OUT}
    assert call(contexts(CFG), x, one) is None
    outs = _spawn(3, "job_litd", (tcase,))
    assert [len(loc) > 0 for loc, _, _ in outs] == [True, True, False] and all(stop is None for _, _, stop in outs)
    seen = sorted(n for loc, _, _ in outs for n in loc)
    assert seen == list(range(x["aicen"].shape[0]))
    for loc, y, _ in outs[:2]:
        for k in OUT:
            assert eq(y[k], one[k][loc]), k
    for k in OUT:                                   # the idle rank's (empty) arrays are what it passed
        assert outs[2][1][k].shape[0] == 0
