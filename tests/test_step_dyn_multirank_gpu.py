"""The second half of step_dynamics on x-slab ranks: evpk_bound_state in one exchange round (k_bound_pack -> one message per partner ->
k_bound_fill), evpk_ridge_ice / evpk_cleanup_itd / evpk_aggregate and the one-call evpk_step_dynamics on K processes that share one GPU
(or take one each where there are K), over the peer-mapped transport ("ipc"), the shared-memory relay ("shm") and, where the devices
suffice, RCCL.  The spawn harness is that of tests/test_multirank_gpu.py: one process per rank, a queue with a timeout, kill on exit, the
/dev/shm tags removed.  Workers send their block arrays back; the parent puts them together by block_id into whole-domain arrays, so that
the yardsticks are the ones of the one-rank tests: the one-rank device path (itself pinned to the reference's ghost cells), the plane-by-plane
path (EVPK_BOUND_DIRECT=0), and the reference's records tests/golden/ref_itd_*.npz.
"""
import os
import sys
import time
import traceback
import uuid

import numpy as np
import pytest

from tests.test_multirank_gpu import XPS, _device_count, _per_rank

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = "g26x18_b8x5"          # 26 x 18 in 8 x 5 blocks: 4 block columns of which the last is 2 wide, and a short last block row
STATE = ["aicen", "vicen", "vsnon", "trcrn"]


# ---- the harness ----
class _Rank:
    def __init__(self, rank, world, tag, xp, dev, uids):
        self.rank, self.world, self.tag, self.xp, self.dev, self.uids = rank, world, tag, xp, dev, uids

    def uid(self, k=0):
        """the unique id of the k-th context this job makes (every rank makes them in the same order)"""
        if self.xp == "rccl":
            return self.uids[k]
        return ({"shm": b"EVPKSHM:", "ipc": b"EVPKIPC:"}[self.xp] + f"{self.tag}_{k}".encode()).ljust(128, b"\0")


def _worker(rank, world, tag, xp, per_rank, job, args, uids, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ["OMP_NUM_THREADS"] = "2"
        dev = rank % max(1, _device_count()) if per_rank else 0
        q.put((rank, None, globals()[job](_Rank(rank, world, tag, xp, dev, uids), *args)))
    except Exception:
        q.put((rank, traceback.format_exc(), None))


def _spawn(world, xp, job, args=(), nctx=1, timeout=240):
    """job(rank info, *args) in `world` processes; what each returned, by rank"""
    import multiprocessing as mp
    per_rank = _per_rank(world)
    if xp == "rccl" and not per_rank:
        pytest.skip(f"RCCL refuses {world} ranks on {_device_count()} device(s)")
    assert world <= 5                              # (+ the parent: at most 6 processes hold the GPU)
    uids = None
    if xp == "rccl":
        from cice5_amd import evpk
        uids = [evpk.get_unique_id() for _ in range(nctx)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "evpk_sd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, world, tag, xp, per_rank, job, args, uids, q)) for r in range(world)]
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
        for k in range(nctx):
            try:
                os.unlink(f"/dev/shm/{tag}_{k}")
            except OSError:
                pass
    return [res[r] for r in range(world)]


def _loc(d1, d):
    """the rank's blocks as indices into the whole-domain block list"""
    at = {b.block_id: n for n, b in enumerate(d1.local_blocks)}
    return [at[b.block_id] for b in d.local_blocks]


def _cut(x, loc, nb1):
    return {k: (np.ascontiguousarray(v[loc]) if isinstance(v, np.ndarray) and v.ndim >= 3 and v.shape[0] == nb1 else v) for k, v in x.items()}


def _assemble(outs, like, names):
    """whole-domain arrays from what the ranks sent back: (loc, dict of block arrays) per rank; every block exactly once"""
    whole = {k: np.full_like(like[k], np.nan if like[k].dtype.kind == "f" else -99) for k in names}
    seen = []
    for loc, y in outs:
        seen += list(loc)
        for k in names:
            if len(loc):
                whole[k][loc] = y[k]
    assert sorted(seen) == list(range(like[names[0]].shape[0])), seen
    return whole


def _params():
    from cice5_amd import dyn
    from tests.golden import ridgevec as rv
    return dyn.set_evp_parameters(rv.DT, 4, False, 1.0e4, krdg_partic=1, krdg_redist=1, ncat=5, mu_rdg=rv.MU_RDG)


def _itd_context(R, bcase, k=0):
    """the rank's context on the fixtures' grid and land (tests/test_itd_gpu.geometry, cut into x-slabs)"""
    from cice5_amd import blocks, constants as C, evpk, synth
    from tests.golden import itdvec as iv
    nx, ny, bx, by, _ = iv.CONFIGS[CFG]
    ew, ns, _ = iv.BOUNDS[bcase]
    d1 = iv.decomp(CFG, bcase)
    d = blocks.create_distrb_cart(nx, ny, bx, by, nprocs=R.world, rank=R.rank, ew_boundary_type=ew, ns_boundary_type=ns)
    loc = _loc(d1, d)
    f = synth.make_block_fields(synth.SynthCase(nx=nx, ny=ny, ew_boundary=C.BND_NAMES[ew], ns_boundary=C.BND_NAMES[ns]), d)
    f["tmask"] = np.ascontiguousarray(iv.tmask(CFG, d1, bcase)[loc])
    ctx = evpk.Context(d, f, device=R.dev, unique_id=R.uid(k))
    ctx.set_params(_params())
    return ctx, d1, d, loc


# ---- 1. bound_state, every element ----
BOUND_CASES = [(ew, ns, land, ncat, ntrcr) for ew, ns, land in (("cyclic", "tripole", "landblock"), ("cyclic", "open", "landblock"), ("open", "open", "none"))
               for ncat, ntrcr in ((5, 3), (5, 0))]
NTRCR_DIM = 5


def _sentinels(case, nb, ncat, nyb, nxb):
    """every cell of every array of the WHOLE domain its own value in (-1, 1), none of them 0"""
    from tests.golden import refvec
    s = lambda k, shape: np.ascontiguousarray(2.0 * refvec.hash01(shape, refvec.seed_of(CFG, case, "bound_ranks", k)) - 1.0)
    return dict(aicen=s("a", (nb, ncat, nyb, nxb)), vicen=s("v", (nb, ncat, nyb, nxb)), vsnon=s("s", (nb, ncat, nyb, nxb)),
                trcrn=s("t", (nb, ncat, NTRCR_DIM, nyb, nxb)))


def _bound_decomp(ew, ns, land, nprocs=1, rank=0):
    from tests import test_ref_pins as P
    from tests.golden import refvec
    z = P.load(CFG)
    case = refvec.case_name(ew, ns, land)
    return case, P.decomp(CFG, z, ew, ns, case, nprocs=nprocs, rank=rank)


def _bound_context(ew, ns, d, device=0, unique_id=None):
    from cice5_amd import constants as C, evpk, synth
    from tests.golden import refvec
    nx, ny, _, _, _ = refvec.CONFIGS[CFG]
    f = synth.make_block_fields(synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[ns], ew_boundary=C.BND_NAMES[ew], land="none"), d)
    return evpk.Context(d, f, device=device, unique_id=unique_id)


def job_bound(R, cases):
    out = []
    for k, (ew, ns, land, ncat, ntrcr) in enumerate(cases):
        case, d1 = _bound_decomp(ew, ns, land)
        _, d = _bound_decomp(ew, ns, land, R.world, R.rank)
        loc = _loc(d1, d)
        inp = _cut(_sentinels(case, d1.nblocks, ncat, d1.ny_block, d1.nx_block), loc, d1.nblocks)
        ctx = _bound_context(ew, ns, d, R.dev, R.uid(k))
        try:
            got, st = {}, {}
            for path in ("packed", "planes"):
                os.environ["EVPK_BOUND_DIRECT"] = "1" if path == "packed" else "0"
                y = {n: inp[n].copy() for n in STATE}
                ctx.bound_state(y["aicen"], y["vicen"], y["vsnon"], y["trcrn"] if ntrcr else None, ntrcr)
                s = ctx.stats()
                got[path], st[path] = y, (int(s.bound_state_rounds), int(s.bound_state_planes), int(s.transport))
        finally:
            os.environ.pop("EVPK_BOUND_DIRECT", None)
            ctx.close()
        out.append((loc, got, st))
    return out


_ONE_RANK_BOUND = {}


def _one_rank_bound(ew, ns, land, ncat, ntrcr):
    """(a): the one-rank ctx.bound_state of the whole domain -- computed once per case, shared, not modified"""
    key = (ew, ns, land, ncat, ntrcr)
    if key not in _ONE_RANK_BOUND:
        case, d1 = _bound_decomp(ew, ns, land)
        inp = _sentinels(case, d1.nblocks, ncat, d1.ny_block, d1.nx_block)
        want = {n: inp[n].copy() for n in STATE}
        ctx = _bound_context(ew, ns, d1)
        try:
            ctx.bound_state(want["aicen"], want["vicen"], want["vsnon"], want["trcrn"] if ntrcr else None, ntrcr)
            s = ctx.stats()
            assert int(s.bound_state_rounds) == 0 and int(s.bound_state_planes) == ncat * (3 + ntrcr)
        finally:
            ctx.close()
        _ONE_RANK_BOUND[key] = (d1, inp, want)
    return _ONE_RANK_BOUND[key]


@pytest.mark.parametrize("xp", XPS)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_bound_state_across_slabs_equals_one_rank_on_every_element(world, xp):
    """Worlds 2 (slabs of 16 and 10 columns; on the cyclic ring west and east neighbour coincide), 3 (the third rank owns no block column)
    and 4 (slabs 8, 8, 8, 2: neighbour and mirror rank differ on both sides), each on cyclic / tripole and cyclic / open with an eliminated
    land block and on open / open, with 30 planes (ntrcr = 3 of 5 slots) and 15 (ntrcr = 0, trcrn = NULL).  Every cell a distinct non-zero
    sentinel.  The packed path equals (a) the one-rank bound_state of the whole domain and (b) the plane-by-plane path of the same ranks on
    every element; it takes ONE exchange round where the plane-by-plane path takes one per 14 planes."""
    from tests.golden import itdvec as iv
    outs = _spawn(world, xp, "job_bound", (BOUND_CASES,), nctx=len(BOUND_CASES))
    nown = min(world, 2) if world < 4 else 4                        # (4 block columns: ceil(4 / world) per rank)
    for k, (ew, ns, land, ncat, ntrcr) in enumerate(BOUND_CASES):
        d1, inp, want = _one_rank_bound(ew, ns, land, ncat, ntrcr)
        per = [o[k] for o in outs]
        for path in ("packed", "planes"):
            got = _assemble([(loc, g[path]) for loc, g, _ in per], inp, STATE)
            for n in STATE:
                assert np.array_equal(got[n], want[n]), (path, k, n, int((got[n] != want[n]).sum()), np.argwhere(got[n] != want[n])[:4])
            assert np.array_equal(got["trcrn"][:, :, ntrcr:], inp["trcrn"][:, :, ntrcr:])          # the spare tracer slots
        phys = iv.physical(d1)
        a, a0 = got["aicen"][:, 0][~phys], inp["aicen"][:, 0][~phys]
        assert (a != a0).sum() > 100 and (a == a0).sum() > 10       # ghost cells rewritten; cells that kept the caller's value
        assert np.array_equal(got["aicen"][:, 0][phys], inp["aicen"][:, 0][phys])
        planes = ncat * (3 + ntrcr)
        for r, (loc, _, st) in enumerate(per):
            if r < nown:
                assert st["packed"][:2] == (1, planes) and st["planes"][:2] == ((planes + 13) // 14, planes), (k, r, st)
                assert st["packed"][2] == {"shm": 2, "ipc": 3, "rccl": 1}[xp]
            else:
                assert len(loc) == 0 and st["packed"][0] == 0, (k, r, st)


# ---- 2. step_dynamics(advection = 0, ridge = 0) against the reference's chain records ----
# the records of the three boundary cases: lvl_ponds where the reference's record has it; the open / open record was made with "plain"
CHAIN_CASES = [("lvl_ponds", "cyclic_open"), ("lvl_ponds", "cyclic_tripole"), ("plain", "open_open")]


def job_chain(R, cases):
    from tests.golden import itdvec as iv
    from tests.test_step_dyn_gpu import _chain_arrays, _step
    from cice5_amd import evpk
    out = []
    for k, (tcase, bcase) in enumerate(cases):
        ctx, d1, d, loc = _itd_context(R, bcase, k)
        try:
            x = iv.itd_input(CFG, tcase, bcase)
            y = _cut(_chain_arrays(x), loc, d1.nblocks)
            assert not evpk.host_is_mapped(y["aicen"])
            assert _step(ctx, x, y, x["dt"], 1) is None
        finally:
            ctx.close()
        out.append((loc, y))
    return out


@pytest.mark.parametrize("xp", XPS)
@pytest.mark.parametrize("world", [2, 3])
def test_step_dynamics_across_slabs_equals_the_reference_chain(world, xp):
    """cleanup_itd(dt * ndtd) -> bound_state -> aggregate -> tendencies on the ranks' pageable arrays: put together, the cleanup record on
    the ocean cells, the ghost cells, c_*, the tendencies, the fluxes and first_ice of the reference's records of the three boundary cases
    (cyclic / open and cyclic / tripole with lvl_ponds; open / open with the tracer table its record was made with, plain)"""
    from tests.golden import itdvec as iv
    from tests.test_itd_gpu import assert_chain_record, assert_cleanup_record
    from tests.test_itd_ref import fixture
    from tests.test_step_dyn_gpu import _chain_arrays
    outs = _spawn(world, xp, "job_chain", (CHAIN_CASES,), nctx=len(CHAIN_CASES))
    for k, (tcase, bcase) in enumerate(CHAIN_CASES):
        x, ref = iv.itd_input(CFG, tcase, bcase), fixture(CFG, tcase, bcase)
        like = _chain_arrays(x)
        y = _assemble([o[k] for o in outs], like, list(like))
        assert_cleanup_record(y, ref, x["ocean"], iv.STATE + iv.FLUX + ["first_ice"])
        assert_chain_record(x, y, ref)


# ---- 3. / 6. ridging on two ranks: one call and the three separate calls; pageable, page-locked and device-resident arrays ----
def job_ridge(R, where, separate):
    from cice5_amd import evpk
    from tests.test_itd_gpu import aggregate, cleanup
    from tests.test_step_dyn_gpu import _diag, _ridge_case, _step
    ctx, d1, d, loc = _itd_context(R, "cyclic_open")
    try:
        r, x, h = _ridge_case()
        h = _cut(h, loc, d1.nblocks)
        if where == "pageable":
            y = {k: v.copy() for k, v in h.items()}
        elif where == "page_locked":
            y = {k: evpk.host_copy(v) for k, v in h.items()}
            assert evpk.host_is_mapped(y["trcrn"])
        else:
            import torch
            torch.cuda.set_device(R.dev)
            y = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
        assert _step(ctx, x, y, r["dt"], r["ndtd"], ridge=True, rdg_conv=y["rdg_conv"], rdg_shear=y["rdg_shear"], diag=_diag(y, False)) is None
        if where == "device":
            torch.cuda.synchronize()
            y = {k: v.cpu().numpy() for k, v in y.items()}
        y = {k: np.array(v) for k, v in y.items()}
        w = None
        if separate:          # ridge_ice(dt, ndtd) -> cleanup_itd(dt * ndtd) -> aggregate(bound = 1, dt) on copies
            w = {k: v.copy() for k, v in h.items()}
            assert ctx.ridge_ice(r["dt"], r["ndtd"], w["aice0"], w["aicen"], w["vicen"], w["vsnon"], w["trcrn"], r["ntrcr"], r["trcr_depend"],
                                 x["tracers"], r["hin_max"], w["rdg_conv"], w["rdg_shear"], _diag(w, True)) is None
            assert cleanup(ctx, dict(x, dt=r["dt"] * r["ndtd"]), w) is None
            aggregate(ctx, dict(x, dt=r["dt"]), w, bound=True)
    finally:
        ctx.close()
    return loc, y, w


@pytest.fixture(scope="module")
def ridge_one_rank():
    """evpk_step_dynamics(ridge = 1) of the whole domain on one rank: computed once, shared, not modified"""
    from cice5_amd import evpk
    from tests.test_itd_gpu import geometry
    from tests.test_step_dyn_gpu import _diag, _ridge_case, _step
    r, x, h = _ridge_case()
    d, f = geometry(CFG, "cyclic_open")
    ctx = evpk.Context(d, f)
    try:
        ctx.set_params(_params())
        y = {k: v.copy() for k, v in h.items()}
        assert _step(ctx, x, y, r["dt"], r["ndtd"], ridge=True, rdg_conv=y["rdg_conv"], rdg_shear=y["rdg_shear"], diag=_diag(y, False)) is None
    finally:
        ctx.close()
    assert not np.array_equal(y["aicen"], h["aicen"])
    return y


@pytest.mark.parametrize("xp", XPS)
def test_step_dynamics_with_ridging_across_slabs_equals_one_rank(ridge_one_rank, xp):
    """two ranks, rdg_conv / rdg_shear given: the state, the aggregates, the tendencies, the fluxes and the ridging diagnostics bit for
    bit those of the one-rank device run; and so are the three separate calls ridge_ice, cleanup_itd, aggregate(bound = 1) on the ranks"""
    from tests.test_itd_gpu import eq
    outs = _spawn(2, xp, "job_ridge", ("pageable", True))
    names = list(ridge_one_rank)
    y = _assemble([(loc, a) for loc, a, _ in outs], ridge_one_rank, names)
    w = _assemble([(loc, b) for loc, _, b in outs], ridge_one_rank, names)
    for k in names:
        assert eq(y[k], ridge_one_rank[k]), ("one call", k, int((y[k] != ridge_one_rank[k]).sum()))
        assert eq(w[k], ridge_one_rank[k]), ("separate calls", k, int((w[k] != ridge_one_rank[k]).sum()))


@pytest.mark.parametrize("where", ["page_locked", "device"])
def test_step_dynamics_across_slabs_on_page_locked_and_device_arrays(ridge_one_rank, where):
    """the arrays used in place: identical to pageable (which the test above ties to the one-rank run)"""
    from tests.test_itd_gpu import eq
    outs = _spawn(2, "ipc", "job_ridge", (where, False))
    names = list(ridge_one_rank)
    y = _assemble([(loc, a) for loc, a, _ in outs], ridge_one_rank, names)
    for k in names:
        assert eq(y[k], ridge_one_rank[k]), (where, k, int((y[k] != ridge_one_rank[k]).sum()))


# ---- 4. after evp, on the rates it leaves resident, with transport ----
def _transport_state(d, f, advection):
    """the arrays of tests/test_step_dyn_gpu._transport_case on a decomposition of ours"""
    from tests import test_parity_gpu as T
    from tests.golden import itdvec as iv
    from tests.golden import ridgevec as rv
    if advection == 2:
        ntrcr, ntrcr_dim = 6, 8
        dep = [0, 1, 1, 2, 2, 0]
        tracers = dict(nt_Tsfc=1, nt_qice=2, nilyr=2, nt_qsno=4, nslyr=2)
        state = list(T._ice_state(d, f, ntrcr, ntrcr_dim, 4, 2))
    else:
        state, kw = T._upwind_state(d, f, 11, "lvl_ponds")
        ntrcr, dep = kw["ntrcr"], kw["trcr_depend"]
        tracers = dict(nt_Tsfc=1, nt_qice=2, nilyr=1, nt_qsno=3, nslyr=1, nt_alvl=4, nt_vlvl=5, nt_apnd=6, nt_hpnd=7, nt_fbri=8, tr_pond_lvl=1,
                       tr_brine=1)
    nb, ncat, ntrcr_dim, nyb, nxb = state[4].shape
    h = dict(zip(rv.STATE, state))
    h.update(aice=np.zeros((nb, nyb, nxb)), vice=np.zeros((nb, nyb, nxb)), vsno=np.zeros((nb, nyb, nxb)), trcr=np.full((nb, ntrcr_dim, nyb, nxb), 555.0),
             daidtd=np.ascontiguousarray(f["aice"].copy()), dvidtd=np.ascontiguousarray(f["vice"].copy()), dagedtd=np.zeros((nb, nyb, nxb)),
             first_ice=np.zeros((nb, ncat, nyb, nxb), dtype=np.int32))
    for k in iv.FLUX:
        h[k] = np.zeros((nb, nyb, nxb))
    x = dict(ntrcr=ntrcr, trcr_depend=np.array(dep, dtype=np.int32), tracers=tracers, hin_max=rv.HIN_MAX.copy(), k=dict(iv.K))
    return x, h


def job_transport(R, ns, advection, nx, ny, bsx, bsy, ndte):
    from cice5_amd import blocks, constants as C, dyn, synth
    from tests.test_itd_gpu import eq
    from tests.test_step_dyn_gpu import _step
    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[ns], land="continents")
    xmin = synth.global_min_dx(case)
    # the whole domain on one rank, in this process
    d1 = blocks.create_distrb_cart(nx, ny, bsx, bsy, ns_boundary_type=ns)
    f1 = synth.make_block_fields(case, d1)
    synth.add_remap_grid(case, d1, f1)
    x, h1 = _transport_state(d1, f1, advection)
    s1 = dyn.EvpDynamics(d1, f1, ndte=ndte, xmin=xmin, device=R.dev)
    try:
        s1.init_evp(3600.0)
        s1.evp(3600.0)
        s1.ctx.remap_init(f1["dxu"], f1["dyu"], f1["hm"])
        dt = 0.4 * xmin / max(np.abs(f1["uvel"]).max(), np.abs(f1["vvel"]).max())
        y1 = {k: v.copy() for k, v in h1.items()}
        assert _step(s1.ctx, x, y1, dt, 1, ridge=True, advection=advection) is None
    finally:
        s1.close()
    # the rank's slab
    d = blocks.create_distrb_cart(nx, ny, bsx, bsy, nprocs=R.world, rank=R.rank, ns_boundary_type=ns)
    loc = _loc(d1, d)
    f = synth.make_block_fields(case, d)
    synth.add_remap_grid(case, d, f)
    s = dyn.EvpDynamics(d, f, ndte=ndte, xmin=xmin, device=R.dev, unique_id=R.uid())
    try:
        s.init_evp(3600.0)
        s.evp(3600.0)
        s.ctx.remap_init(f["dxu"], f["dyu"], f["hm"])
        y = _cut(h1, loc, d1.nblocks)
        assert _step(s.ctx, x, y, dt, 1, ridge=True, advection=advection) is None
        rounds = int(s.ctx.stats().bound_state_rounds)
    finally:
        s.close()
    bad = [(k, int((y[k] != y1[k][loc]).sum())) for k in h1 if not eq(y[k], y1[k][loc])]
    changed = sorted(k for k in h1 if not eq(y[k], h1[k][loc]))
    return bad, changed, rounds, len(loc)


@pytest.mark.parametrize("ns,world,xp,advection", [("tripole", 4, "ipc", 2), ("open", 3, "shm", 2), ("tripole", 2, "ipc", 2), ("tripole", 2, "ipc", 1)])
def test_step_dynamics_after_evp_with_transport_across_slabs(ns, world, xp, advection):
    """240 x 64 in 20 x 32 blocks: evp with a short ndte, then evpk_step_dynamics(advection, ridge = 1, rdg_conv = NULL) -- transport on
    the resident velocities, ridging on the rates evp left on the device, cleanup_itd, bound_state, aggregate -- on the ranks, and the same
    two calls on a one-rank context of the whole grid: every cell of aice0, aicen, vicen, vsnon, trcrn, aice, vice, vsno, trcr, the
    tendencies, the fluxes and first_ice is equal, and the state changed"""
    if xp not in XPS:
        pytest.skip(f"transport {xp} is not among EVPK_TEST_XPS")
    outs = _spawn(world, xp, "job_transport", (ns, advection, 240, 64, 20, 32, 12))
    for r, (bad, changed, rounds, nloc) in enumerate(outs):
        assert not bad, (r, bad)
        assert nloc > 0 and rounds == 1, (r, nloc, rounds)
        for k in ("aice0", "aicen", "vicen", "vsnon", "trcrn", "aice", "vice", "vsno", "trcr", "daidtd", "dvidtd"):
            assert k in changed, (r, k, changed)


# ---- 5. a stop on one rank hangs nobody ----
def _ridge_stop_cell(x):
    """a physical ocean cell (global block index, i, j; 1-based i, j) of the LAST block column, which rank 1 of 2 owns"""
    from tests.golden import itdvec as iv
    d1 = iv.decomp(CFG, "cyclic_open")
    for b, blk in enumerate(d1.local_blocks):
        if blk.iglob_lo > 16 and x["ocean"][b, 3, 2]:
            return b, 3, 4
    raise AssertionError("no ocean cell")


def job_stop(R, what, name):
    from tests.golden import itdvec as iv
    from tests.golden import ridgevec as rv
    from tests.test_step_dyn_gpu import _chain_arrays, _ridge_case, _step
    ctx, d1, d, loc = _itd_context(R, "cyclic_open")
    try:
        if what == "itd":
            # the failing cells of iv.STOPS lie in the global blocks 6 (rank 0) and 11 (rank 1): rank 1 takes the input without them
            x = iv.stop_input(name) if R.rank == 0 else iv.itd_input(CFG, "plain", tag="stop")
            y = _cut(_chain_arrays(x), loc, d1.nblocks)
            t0 = time.time()
            got = _step(ctx, x, y, x["dt"], 1)
        else:
            r, x, h = _ridge_case()
            b, i, j = _ridge_stop_cell(x)
            sp = rv.STOPS[name]
            h["aice0"][b, j - 1, i - 1] = sp["aice0"]
            for k in ("aicen", "vicen", "vsnon"):
                h[k][b, :, j - 1, i - 1] = 0.0
            h["aicen"][b, sp["n"] - 1, j - 1, i - 1] = sp["a"]
            h["vicen"][b, sp["n"] - 1, j - 1, i - 1] = sp["a"] * sp["h"]
            h["rdg_conv"][b, j - 1, i - 1] = 0.0
            h["rdg_shear"][b, j - 1, i - 1] = 0.0
            y = _cut(h, loc, d1.nblocks)
            t0 = time.time()
            got = _step(ctx, x, y, r["dt"], r["ndtd"], ridge=True, rdg_conv=y["rdg_conv"], rdg_shear=y["rdg_shear"])
        secs = time.time() - t0
        ctx.sync()
        # the transport is still in step: one more collective call on clean arrays goes through on both ranks
        z = {k: np.ones_like(y[k]) for k in STATE}
        ctx.bound_state(z["aicen"], z["vicen"], z["vsnon"], z["trcrn"], x["ntrcr"])
    finally:
        ctx.close()
    return loc, got, secs


@pytest.mark.parametrize("xp", XPS)
def test_a_cleanup_stop_on_one_rank_hangs_nobody(xp):
    """iv.STOPS "bounds" in rank 0's slab: rank 0 returns (EVPK_ITD_STOP, 3, reason, its LOCAL block, i, j) after posting aggregate's
    bound_state; rank 1 returns normally, well inside the 20 s after which a wait on a partner gives up, and the transport stays in step
    (a further bound_state passes on both ranks).  Ordinary return codes, no fault."""
    from cice5_amd import evpk
    from tests.golden import itdvec as iv
    from tests.test_itd_ref import GOLDEN
    name = "bounds"
    ref = np.load(os.path.join(GOLDEN, "ref_itd_stops.npz"))[name]
    b = int(np.nonzero(ref[0])[0][0])                  # the first whole-domain block that stops (0-based)
    outs = _spawn(2, xp, "job_stop", ("itd", name))
    (loc0, got0, secs0), (loc1, got1, secs1) = outs
    assert b in loc0 and b not in loc1
    assert got0 == (evpk.ITD_STOP, 3, iv.STOPS[name]["reason"], loc0.index(b) + 1, int(ref[1][b]), int(ref[2][b]))
    assert got1 is None
    assert max(secs0, secs1) < 10.0, (secs0, secs1)


@pytest.mark.parametrize("xp", XPS)
def test_a_ridge_stop_on_one_rank_hangs_nobody(xp):
    """the rv.STOPS "aice0_negative" cell placed in rank 1's slab: stage 2 with the cell and rank 1's local block; rank 0 returns normally"""
    from cice5_amd import evpk
    from tests.golden import ridgevec as rv
    from tests.test_step_dyn_gpu import _ridge_case
    name = "aice0_negative"
    b, i, j = _ridge_stop_cell(_ridge_case()[1])
    outs = _spawn(2, xp, "job_stop", ("ridge", name))
    (loc0, got0, secs0), (loc1, got1, secs1) = outs
    assert b in loc1 and b not in loc0
    assert got0 is None
    assert got1 == (evpk.RIDGE_STOP, 2, rv.STOPS[name]["reason"], loc1.index(b) + 1, i, j)
    assert max(secs0, secs1) < 10.0, (secs0, secs1)
