"""The one staging path of the host API (stage_in / stage_out, cice5_amd/csrc/evpk_api.hip): every entry point that takes the caller's block
arrays computes the same bits whether they are pageable (copied up into the call's pool and the outputs copied down again), page-locked or
device resident (used in place), or a mixture of the three within one call -- the choice is made array by array, and the staged ones are
packed one behind the other in the pool.  Pageable results are pinned to the reference or the oracle elsewhere (tests/test_ref_pins_gpu.py,
test_parity_gpu.py, test_ridge_gpu.py, test_itd_gpu.py); here the other kinds are compared with them bit for bit, input-only arrays must come
back unchanged, the shared pool grows and is reused across calls of different size, and a transport_remap that stops copies nothing back.
Shapes: g26x18_b8x5 (16 blocks, the last column and row padded; 15 with an eliminated land block) on cyclic / tripole and open / open.
Inputs: tests/golden/refvec.py, ridgevec.py, itdvec.py.
"""
import numpy as np
import pytest

try:
    import torch          # before libevpk: the process must end up with ONE HIP runtime (torch bundles its own)
    torch.cuda.is_available()
except ImportError:
    torch = None

from cice5_amd import constants as C
from cice5_amd import dyn, evpk, synth
from oracle import orc
from tests import test_ref_pins as P
from tests import util
from tests.golden import itdvec as iv
from tests.golden import make_ref_itd as gen
from tests.golden import refvec
from tests.golden import ridgevec as rv
from tests.test_itd_gpu import aggregate, cleanup, copies, eq, post_bound_state
from tests.test_itd_gpu import geometry as itd_geometry
from tests.test_itd_ref import fixture
from tests.test_ridge_gpu import device_run
from tests.test_ridge_gpu import geometry as ridge_geometry
from tests.test_ridge_ref import ARRAYS as RIDGE_ARRAYS

pytestmark = pytest.mark.gpu

CFG = "g26x18_b8x5"
BOUNDS = [("cyclic", "tripole", "landblock"), ("open", "open", "none")]
KINDS = ["pageable", "page_locked", "device", "mixed", "mixed_shifted"]
ROTATION = ["pageable", "page_locked", "device"]


class _Dev:
    """a device tensor with the members Context.transport_remap asks of an array"""

    def __init__(self, t):
        self.t, self.ndim, self.shape, self.dtype, self.flags = t, t.ndim, tuple(t.shape), t.dtype, {"C_CONTIGUOUS": t.is_contiguous()}

    def data_ptr(self):
        return self.t.data_ptr()

    def is_contiguous(self):
        return self.t.is_contiguous()

    def cpu(self):
        return self.t.cpu()


def held(x, kind):
    """copies of the arrays of x (None stays) in one kind of memory; mixed: alternately pageable, page-locked and device in the order of x"""
    y = {}
    for q, (k, a) in enumerate(x.items()):
        how = kind if kind in ROTATION else ROTATION[(q + (kind == "mixed_shifted")) % 3]
        if a is None:
            y[k] = None
        elif how == "pageable":
            y[k] = a.copy()
            assert not evpk.host_is_mapped(y[k])
        elif how == "page_locked":
            y[k] = evpk.host_copy(a)
            assert evpk.host_is_mapped(y[k])
        else:
            y[k] = _Dev(torch.from_numpy(a).cuda())
    return y


def to_host(y):
    torch.cuda.synchronize()
    return {k: None if v is None else (v.cpu().numpy() if isinstance(v, _Dev) else np.array(v)) for k, v in y.items()}


def check_kinds(x, call, input_only=(), writes=True, returns=None):
    """call(y) on copies of x in every kind of memory: what it returns and every array afterwards equal the pageable run's, bit for bit;
    the arrays of input_only are as they were.  writes: the call has to change some array; returns: what it has to return.  Returns the
    pageable results."""
    want = want_rc = None
    for kind in KINDS:
        y = held(x, kind)
        rc = call(y)
        got = to_host(y)
        for k in input_only:
            assert eq(got[k], x[k]), (kind, k, "an input was written")
        if kind == "pageable":
            want, want_rc = got, rc
            assert rc == returns, rc
            assert not writes or any(v is not None and not eq(v, x[k]) for k, v in got.items()), "the call changed nothing"
            continue
        assert rc == want_rc, (kind, rc, want_rc)
        for k, v in got.items():
            assert v is None or eq(v, want[k]), (kind, k, int((v != want[k]).sum()))
    return want


# ---- the contexts: with an eliminated land block on cyclic / tripole, all blocks on open / open; velocities uploaded, remap grid set ----
def _pins_geometry(ew, ns, land):
    nx, ny, _, _, _ = refvec.CONFIGS[CFG]
    case = refvec.case_name(ew, ns, land)
    d = P.decomp(CFG, P.load(CFG), ew, ns, case)
    sc = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[ns], ew_boundary=C.BND_NAMES[ew], land="none")
    f = synth.make_block_fields(sc, d)
    synth.add_remap_grid(sc, d, f)
    for k in ("uvel", "vvel"):                           # (the synthetic ice is at rest here) rough, up to 0.3 m/s: Courant numbers of 1e-3
        f[k] = np.ascontiguousarray(0.3 * (2.0 * refvec.hash01(f[k].shape, refvec.seed_of(CFG, case, "staging", k)) - 1.0))
    return case, sc, d, f


def _resident(d, f, xmin):
    ctx = evpk.Context(d, f)
    ctx.set_params(dyn.set_evp_parameters(3600.0, 2, False, xmin))
    ctx.upload(f)                                        # uvel, vvel resident, as after an evp
    ctx.remap_init(f["dxu"], f["dyu"], f["hm"])
    return ctx


@pytest.fixture(scope="module")
def pins():
    made = {}

    def get(ew, ns, land):
        if (ew, ns, land) not in made:
            case, sc, d, f = _pins_geometry(ew, ns, land)
            assert d.nblocks == (15 if land == "landblock" else 16)
            made[ew, ns, land] = (case, d, f, _resident(d, f, synth.global_min_dx(sc)))
        return made[ew, ns, land]
    yield get
    for m in made.values():
        m[3].close()


@pytest.fixture(scope="module")
def itd_contexts():
    made = {}

    def get(bcase):
        if bcase not in made:
            ctx = evpk.Context(*itd_geometry(CFG, bcase))
            ctx.set_params(dyn.set_evp_parameters(3600.0, 4, False, 1.0e4, ncat=5))
            made[bcase] = ctx
        return made[bcase]
    yield get
    for c in made.values():
        c.close()


def _ridge_context():
    ctx = evpk.Context(*ridge_geometry(CFG))
    ctx.set_params(dyn.set_evp_parameters(rv.DT, 4, False, 1.0e4, krdg_partic=1, krdg_redist=1, ncat=5, mu_rdg=rv.MU_RDG))
    return ctx


def _state(case, d, ntrcr_dim):
    """aice0, aicen, vicen, vsnon, trcrn of refvec.state_input: every cell its own value"""
    a, v, s, t = refvec.state_input(CFG, case, d.nblocks, d.ny_block, d.nx_block, ntrcr_dim)
    return dict(aice0=np.ascontiguousarray(1.0 - a.sum(axis=1)), aicen=a, vicen=v, vsnon=s, trcrn=np.ascontiguousarray(t[:, :, :ntrcr_dim]))


# ---- 1. halo_update, halo_update_stress ----
@pytest.mark.parametrize("ew,ns,land", BOUNDS)
@pytest.mark.parametrize("nz,loc,typ,fill", [(0, C.LOC_NECORNER, C.KIND_VECTOR, 0.0), (3, C.LOC_CENTER, C.KIND_SCALAR, -9.5)])
def test_halo_update(pins, ew, ns, land, nz, loc, typ, fill):
    case, d, f, ctx = pins(ew, ns, land)
    x = dict(a=refvec.halo_r8_input(CFG, case, f"staging{nz}", d.nblocks, d.ny_block, d.nx_block, nz))
    check_kinds(x, lambda y: ctx.halo_update(y["a"], loc, typ, fill))


@pytest.mark.parametrize("ew,ns,land", BOUNDS)
def test_halo_update_stress(pins, ew, ns, land):
    """[a1 | a2] in the pool when both are pageable; a2 is an input; next to the eliminated land block the coverage plane is built"""
    case, d, f, ctx = pins(ew, ns, land)
    x = {k: refvec.halo_r8_input(CFG, case, k, d.nblocks, d.ny_block, d.nx_block, 0) for k in ("stress1", "stress2")}
    check_kinds(x, lambda y: ctx.halo_update_stress(y["stress1"], y["stress2"]), input_only=["stress2"],
                writes=(ns == "tripole"))            # (without a fold there may be nothing to write)


# ---- 2. transport_upwind, transport_upwind_state ----
@pytest.mark.parametrize("ew,ns,land", BOUNDS)
def test_transport_upwind(pins, ew, ns, land):
    case, d, f, ctx = pins(ew, ns, land)
    s = _state(case, d, 1)
    x = dict(works=np.ascontiguousarray(np.concatenate([s["aice0"][:, None], s["aicen"], s["vicen"]], axis=1)))
    check_kinds(x, lambda y: ctx.transport_upwind(600.0, y["works"]))


@pytest.mark.parametrize("ew,ns,land", BOUNDS)
def test_transport_upwind_state(pins, ew, ns, land):
    """every tracer rule of state_to_work / compute_tracers; two tracer slots beyond ntrcr; the coverage plane next to the land block"""
    case, d, f, ctx = pins(ew, ns, land)
    dep, n_tsfc, n_alvl, n_apnd, n_fbri, pond = refvec.TRACER_CASES["lvl_ponds"]
    x = _state(case, d, len(dep) + 2)
    want = check_kinds(x, lambda y: ctx.transport_upwind_state(600.0, y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], len(dep), dep,
                                                               nt_Tsfc=n_tsfc, nt_alvl=n_alvl, nt_apnd=n_apnd, nt_fbri=n_fbri, ponds=pond))
    assert eq(want["trcrn"][:, :, len(dep):], x["trcrn"][:, :, len(dep):])


# ---- 3. transport_remap, transport_remap_state ----
@pytest.mark.parametrize("case", ["cyclic_tripole", "open_closed_rim", "areas_only"])
def test_transport_remap(case):
    """mm and tm, and mm alone (tm = NULL: a null device pointer, never staged)"""
    d, f, mm, tm, tables = refvec.remap_fields(CFG, case)
    order, midpt = refvec.REMAP_CASES[case][2][0]
    ctx = _resident(d, f, 1.0e4)
    try:
        x = dict(mm=mm, tm=tm if tm.shape[2] else None)
        check_kinds(x, lambda y: ctx.transport_remap(refvec.REMAP_DT, y["mm"], y["tm"], *tables, integral_order=order, l_dp_midpt=bool(midpt)),
                    returns=0)
    finally:
        ctx.close()


@pytest.mark.parametrize("ew,ns,land", BOUNDS)
def test_transport_remap_state(pins, ew, ns, land):
    """next to the eliminated land block the ice is at rest, as tests/test_ref_pins_gpu.py has it (the slab holds no grid lengths there, and a
    departure point next to it is out of bounds): the round trip through the tracer transforms still rewrites every array"""
    case, d, f, ctx = pins(ew, ns, land)
    if land == "landblock":
        f = dict(f, uvel=np.zeros_like(f["uvel"]), vvel=np.zeros_like(f["vvel"]))
        ctx = _resident(d, f, 1.0e4)
    ntrcr = 3
    x = _state(case, d, ntrcr + 1)
    tables = orc.remap_tables([0, 1, 2])
    try:
        want = check_kinds(x, lambda y: ctx.transport_remap_state(600.0, y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], ntrcr, 3, 1,
                                                                  330.0 * 3.34e5, *tables), returns=0)
    finally:
        if land == "landblock":
            ctx.close()
    assert eq(want["trcrn"][:, :, ntrcr:], x["trcrn"][:, :, ntrcr:])


def _unchanged_after_stop(ctx, dt, mm, tm, tables, order, midpt, code):
    mg, tg = mm.copy(), tm.copy()
    assert not evpk.host_is_mapped(mg) and not evpk.host_is_mapped(tg)
    assert ctx.transport_remap(dt, mg, tg, *tables, integral_order=order, l_dp_midpt=bool(midpt)) == code
    assert np.array_equal(mg, mm) and np.array_equal(tg, tm)


def test_a_transport_remap_that_stops_copies_nothing_back(pins):
    """the reference's two l_stop cases (its own records' inputs and test_transport_remap_reports_the_two_abort_cases'): the update has
    written the staged copies by then -- the caller's pageable arrays keep every bit; the same for the state arrays of transport_remap_state"""
    codes = {1: evpk.REMAP_BAD_DEPARTURE, 2: evpk.REMAP_NEGATIVE_MASS}
    for name, (rc, order, midpt) in refvec.REMAP_STOPS.items():
        d, f, mm, tm, tables = refvec.remap_fields(CFG, "cyclic_open", stop=name)
        ctx = _resident(d, f, 1.0e4)
        try:
            _unchanged_after_stop(ctx, refvec.REMAP_DT, mm, tm, tables, order, midpt, codes[rc])
        finally:
            ctx.close()
    case, d, f, mm, tm, tables = util.remap_case(48, 40, 24, 20)
    ctx = _resident(d, f, 1.0e4)
    try:
        _unchanged_after_stop(ctx, 3600.0 * 400, mm, tm, tables, 3, True, evpk.REMAP_BAD_DEPARTURE)
    finally:
        ctx.close()
    case, d, f, ctx = pins(*BOUNDS[1])
    x = _state(case, d, 4)
    y = held(x, "pageable")
    assert ctx.transport_remap_state(3600.0 * 4000, y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], 3, 3, 1, 330.0 * 3.34e5,
                                     *orc.remap_tables([0, 1, 2])) == evpk.REMAP_BAD_DEPARTURE
    for k in x:
        assert np.array_equal(y[k], x[k]), k


# ---- 4. ridge_ice, cleanup_itd, aggregate, bound_state ----
def test_ridge_ice():
    """all 23 arrays of a call; the rates are inputs"""
    r = rv.ridge_input(CFG, "lvl_ponds")
    x = copies(r, RIDGE_ARRAYS + ["rdg_conv", "rdg_shear"])
    ctx = _ridge_context()
    try:
        check_kinds(x, lambda y: device_run(ctx, dict(r, rdg_conv=y["rdg_conv"], rdg_shear=y["rdg_shear"]), y), input_only=["rdg_conv", "rdg_shear"])
    finally:
        ctx.close()


@pytest.mark.parametrize("tcase,bcase", [("lvl_ponds", "cyclic_tripole"), ("plain", "open_open")])
def test_cleanup_itd(itd_contexts, tcase, bcase):
    """ten arrays of doubles and first_ice, whose int32 elements end the pool on half a double"""
    ctx = itd_contexts(bcase)
    x = iv.itd_input(CFG, tcase, bcase)
    check_kinds(copies(x, iv.STATE + gen.CELL2 + ["first_ice"]), lambda y: cleanup(ctx, x, y))


@pytest.mark.parametrize("bound", [0, 1])
@pytest.mark.parametrize("tcase,bcase", [("lvl_ponds", "cyclic_tripole"), ("plain", "open_open")])
def test_aggregate(itd_contexts, tcase, bcase, bound):
    """bound = 0: the category arrays are inputs and are not copied back"""
    ctx = itd_contexts(bcase)
    x = iv.itd_input(CFG, tcase, bcase)
    z = post_bound_state(x, fixture(CFG, tcase, bcase), ghosts=not bound)
    check_kinds(z, lambda y: aggregate(ctx, x, y, bound=bool(bound)), input_only=[] if bound else iv.STATE)


@pytest.mark.parametrize("ew,ns,land", BOUNDS)
def test_bound_state(pins, ew, ns, land):
    case, d, f, ctx = pins(ew, ns, land)
    x = _state(case, d, 5)
    del x["aice0"]
    check_kinds(x, lambda y: ctx.bound_state(y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], 3))


# ---- 5. the pool of a context across calls: small -> large -> small ----
def test_the_pool_grows_and_is_reused():
    """halo_update of one 2-D array (the pool is made), ridge_ice with every diagnostic (it grows: the old one is freed), halo_update again
    (the larger pool is reused) on one context equal the same calls on a fresh context each"""
    d, _ = ridge_geometry(CFG)
    r = rv.ridge_input(CFG, "lvl_ponds")
    a = refvec.halo_r8_input(CFG, "cyclic_open", "pool", d.nblocks, d.ny_block, d.nx_block, 0)

    def halo(ctx):
        y = a.copy()
        ctx.halo_update(y, C.LOC_CENTER, C.KIND_SCALAR, 0.0)
        return dict(a=y)

    def ridge(ctx):
        y = copies(r, RIDGE_ARRAYS)
        assert device_run(ctx, r, y) is None
        return y

    got, want = [], []
    ctx = _ridge_context()
    try:
        for call in (halo, ridge, halo):
            got.append(call(ctx))
    finally:
        ctx.close()
    for call in (halo, ridge):
        ctx = _ridge_context()
        try:
            want.append(call(ctx))
        finally:
            ctx.close()
    assert not eq(want[0]["a"], a) and not eq(want[1]["aicen"], r["aicen"])
    for g, w in zip(got, want + want[:1]):
        for k in w:
            assert eq(g[k], w[k]), k
