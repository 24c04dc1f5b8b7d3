"""evpk_cleanup_itd and evpk_aggregate on the device against the reference fixtures tests/golden/ref_itd_*.npz -- bit for bit: the
routines use only + - x / and comparisons, the library is built with -ffp-contract=off -- and, where the reference build cannot go
(ncat = 3; ridge_ice in front), against the numpy restatement tests/npitd.py, which equals the fixtures bit for bit
(tests/test_itd_ref.py).  Inputs: tests/golden/itdvec.py (no shape larger than 26 x 18 cells).
"""
import os

import numpy as np
import pytest

try:
    import torch          # before libevpk: the process must end up with ONE HIP runtime (torch bundles its own)
    torch.cuda.is_available()
except ImportError:
    torch = None

from cice5_amd import constants as C
from cice5_amd import dyn, evpk, synth
from tests.golden import itdvec as iv
from tests.golden import make_ref_itd as gen
from tests.golden import ridgevec as rv
from tests.test_itd_ref import GOLDEN, RECORDS, fixture

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
CELL2 = gen.CELL2


def geometry(cfg, bcase):
    nx, ny, _, _, _ = iv.CONFIGS[cfg]
    ew, ns, _ = iv.BOUNDS[bcase]
    d = iv.decomp(cfg, bcase)
    case = synth.SynthCase(nx=nx, ny=ny, ew_boundary=C.BND_NAMES[ew], ns_boundary=C.BND_NAMES[ns])
    f = synth.make_block_fields(case, d)
    f["tmask"] = iv.tmask(cfg, d, bcase)          # the land of the fixtures
    return d, f


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(cfg, bcase="cyclic_open"):
        if (cfg, bcase) not in made:
            d, f = geometry(cfg, bcase)
            ctx = evpk.Context(d, f)
            ctx.set_params(dyn.set_evp_parameters(3600.0, 4, False, 1.0e4, ncat=5))
            made[cfg, bcase] = ctx
        return made[cfg, bcase]
    yield get
    for c in made.values():
        c.close()


def copies(x, names):
    return {k: x[k].copy() for k in names}


def cleanup(ctx, x, y, fluxes=True, first_ice=True, **kw):
    return ctx.cleanup_itd(x["dt"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice0"], y["aice"], x["ntrcr"], x["trcr_depend"],
                           x["tracers"], x["hin_max"], x["k"], {k: y[k] for k in iv.FLUX} if fluxes else None,
                           y["first_ice"] if first_ice else None, **kw)


def aggregate(ctx, x, z, bound, tend=True):
    ctx.aggregate(x["dt"], z["aicen"], z["vicen"], z["vsnon"], z["trcrn"], z["aice"], z["vice"], z["vsno"], z["aice0"], z["trcr"], x["ntrcr"],
                  x["trcr_depend"], x["tracers"], bound=bound, daidtd=z["daidtd"] if tend else None, dvidtd=z["dvidtd"] if tend else None,
                  dagedtd=z["dagedtd"] if tend else None, Tocnfrz=x["k"]["Tocnfrz"])


def eq(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all()) if a.dtype.kind == "f" else np.array_equal(a, b)


def assert_cleanup_record(y, ref, m, names):
    for k in names:
        a, b = gen.on_cells(y[k], m), ref[k]
        assert a.shape == b.shape and eq(a, b), (k, int((a != b).sum()))


def post_bound_state(x, ref, ghosts=True):
    """the state after cleanup_itd (+ bound_state) rebuilt from the record alone: ocean cells, ghost cells; land cells are empty"""
    z = {}
    for k in iv.STATE:
        a = np.zeros_like(x[k])
        v = np.moveaxis(a, (0, -2, -1), (0, 1, 2))
        v[x["ocean"]] = ref[k]
        if ghosts:
            v[~x["phys"]] = ref["g_" + k]
        z[k] = a
    nb, ncat, ntrcr, ny, nx = x["trcrn"].shape
    for k in ("aice", "vice", "vsno", "aice0"):
        z[k] = np.full((nb, ny, nx), SENTINEL)
    z["trcr"] = np.full((nb, ntrcr, ny, nx), SENTINEL)
    z.update(copies(x, iv.TEND))
    return z


def assert_chain_record(x, z, ref):
    for k in iv.STATE:
        assert eq(gen.on_cells(z[k], ~x["phys"]), ref["g_" + k]), "g_" + k
    for k in ("aice", "vice", "vsno", "aice0", "trcr"):
        assert eq(z[k], ref["c_" + k]), "c_" + k
    for k in iv.TEND:
        assert eq(gen.on_cells(z[k], x["phys"]), ref[k]), k


@pytest.mark.parametrize("cfg,tcase,bcase", RECORDS)
def test_cleanup_equals_the_reference_and_leaves_land_and_ghost_cells(contexts, cfg, tcase, bcase):
    """both grids, all pond tables: physical ocean cells equal the record; land, ghost and padding cells of aicen / vicen / vsnon / trcrn
    keep a sentinel"""
    ctx = contexts(cfg, bcase)
    x = iv.itd_input(cfg, tcase, bcase)
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    m = x["ocean"]
    for k in iv.STATE:
        np.moveaxis(y[k], (0, -2, -1), (0, 1, 2))[~m] = SENTINEL
    assert cleanup(ctx, x, y) is None
    assert_cleanup_record(y, fixture(cfg, tcase, bcase), m, iv.STATE + CELL2 + ["first_ice"])
    for k in iv.STATE:
        assert (np.moveaxis(y[k], (0, -2, -1), (0, 1, 2))[~m] == SENTINEL).all(), k


def test_quiet_input_leaves_trcrn_untouched(contexts):
    """no cell shifts and none is zapped: trcrn, the state and the fluxes are bitwise what they were (lvl_ponds: hin_max(0) = 0)"""
    ctx = contexts("g26x18_b8x5")
    x = iv.itd_input("g26x18_b8x5", "lvl_ponds", quiet=True)
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    assert cleanup(ctx, x, y) is None
    for k in iv.STATE + iv.FLUX + ["first_ice"]:
        assert eq(y[k], x[k]), k
    want, _, infos, _ = gen.restate(x, chain=False)
    assert not any(i["boundaries"] or i["zap1"] or i["zap2"] or i["zapT"] for i in infos)
    for k in ("aice0", "aice"):
        assert eq(y[k][x["ocean"]], want[k][x["ocean"]]), k


def test_generic_path_ncat3_equals_restatement(contexts):
    ctx = contexts("g26x18_b8x5")
    x = iv.itd_input("g26x18_b8x5", "lvl_ponds", ncat=3, tag="ncat3")
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    assert cleanup(ctx, x, y) is None
    want, chain, infos, stop = gen.restate(x)
    assert stop is None and sum(len(i["boundaries"]) for i in infos) >= 3 and sum(len(i["zap1"]) for i in infos) >= 1
    for k in iv.STATE + CELL2 + ["first_ice"]:
        assert eq(gen.on_cells(y[k], x["ocean"]), gen.on_cells(want[k], x["ocean"])), k
    z = dict(copies(y, iv.STATE), **copies(x, iv.TEND))
    nb, ncat, ntrcr, ny, nx = x["trcrn"].shape
    for k in ("aice", "vice", "vsno", "aice0"):
        z[k] = np.full((nb, ny, nx), SENTINEL)
    z["trcr"] = np.full((nb, ntrcr, ny, nx), SENTINEL)
    for k in iv.STATE:                                  # (land cells: the reference zeroes their tracers in a block that shifts)
        np.moveaxis(z[k], (0, -2, -1), (0, 1, 2))[x["phys"] & ~x["ocean"]] = np.moveaxis(chain[k], (0, -2, -1), (0, 1, 2))[x["phys"] & ~x["ocean"]]
    aggregate(ctx, x, z, bound=True)
    for k in iv.STATE + ["aice", "vice", "vsno", "aice0", "trcr"] + iv.TEND:
        assert eq(z[k], chain[k]), k


def test_aggregate_without_bound(contexts):
    """bound = 0 on a state whose ghost cells are current: every cell of every block, and the tendencies; the state is not written"""
    cfg, tcase, bcase = "g26x18_b8x5", "cesm_ponds", "cyclic_open"
    ctx = contexts(cfg, bcase)
    x, ref = iv.itd_input(cfg, tcase, bcase), fixture(cfg, tcase, bcase)
    z = post_bound_state(x, ref)
    before = copies(z, iv.STATE)
    aggregate(ctx, x, z, bound=False)
    assert_chain_record(x, z, ref)
    for k in iv.STATE:
        assert eq(z[k], before[k]), k


@pytest.mark.parametrize("cfg,tcase,bcase", [("g26x18_b8x5", "lvl_ponds", "cyclic_open"), ("g26x18_b8x5", "lvl_ponds", "cyclic_tripole"),
                                             ("g26x18_b8x5", "plain", "open_open"), ("g24x16_b24x16", "topo_ponds", "cyclic_open")])
def test_aggregate_with_bound_state(contexts, cfg, tcase, bcase):
    """bound = 1 on cyclic, tripole and open boundaries: the ghost cells of the state, aggregate on every cell, the tendencies"""
    ctx = contexts(cfg, bcase)
    x, ref = iv.itd_input(cfg, tcase, bcase), fixture(cfg, tcase, bcase)
    z = post_bound_state(x, ref, ghosts=False)
    aggregate(ctx, x, z, bound=True)
    assert_chain_record(x, z, ref)


def test_null_optional_arguments(contexts):
    cfg, tcase, bcase = "g26x18_b8x5", "topo_ponds", "cyclic_open"
    ctx = contexts(cfg, bcase)
    x, ref = iv.itd_input(cfg, tcase, bcase), fixture(cfg, tcase, bcase)
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    assert cleanup(ctx, x, y, fluxes=False, first_ice=False) is None
    assert_cleanup_record(y, ref, x["ocean"], iv.STATE + ["aice0", "aice"])
    for k in iv.FLUX + ["first_ice"]:
        assert eq(y[k], x[k]), k
    z = post_bound_state(x, ref)
    aggregate(ctx, x, z, bound=False, tend=False)
    for k in ("aice", "vice", "vsno", "aice0", "trcr"):
        assert eq(z[k], ref["c_" + k]), k
    for k in iv.TEND:
        assert eq(z[k], x[k]), k


def test_chain_on_device_resident_arrays(contexts):
    """cleanup_itd -> aggregate(bound = 1) on tensors in device memory, against the chain record"""
    cfg, tcase, bcase = "g26x18_b8x5", "lvl_ponds", "cyclic_tripole"
    ctx = contexts(cfg, bcase)
    x, ref = iv.itd_input(cfg, tcase, bcase), fixture(cfg, tcase, bcase)
    nb, ncat, ntrcr, ny, nx = x["trcrn"].shape
    h = copies(x, iv.STATE + CELL2 + iv.TEND + ["first_ice"])
    h.update(vice=np.zeros((nb, ny, nx)), vsno=np.zeros((nb, ny, nx)), trcr=np.zeros((nb, ntrcr, ny, nx)))
    dev = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    assert cleanup(ctx, x, dev) is None
    one = {k: dev[k].cpu().numpy() for k in iv.STATE + CELL2 + ["first_ice"]}
    assert_cleanup_record(one, ref, x["ocean"], iv.STATE + CELL2 + ["first_ice"])
    aggregate(ctx, x, dev, bound=True)
    torch.cuda.synchronize()
    assert_chain_record(x, {k: v.cpu().numpy() for k, v in dev.items()}, ref)


def test_ridge_ice_cleanup_aggregate_on_device_resident_arrays(contexts):
    """ridge_ice -> cleanup_itd -> aggregate(bound = 1) without the state leaving the device: equal to the restatement of the last two
    fed with the state ridge_ice left (the reference's record starts after ridging)"""
    cfg = "g26x18_b8x5"
    ctx = contexts(cfg)
    r = rv.ridge_input(cfg, "lvl_ponds")
    x = iv.itd_input(cfg, "lvl_ponds")
    tr = dict(r["tracers"], nt_Tsfc=1, nt_qice=2, nilyr=1, tr_brine=1)
    x.update(ntrcr=r["ntrcr"], trcr_depend=r["trcr_depend"], tracers=tr, hin_max=r["hin_max"])
    assert np.array_equal(rv.listed(x["d"], x["tmask"]), x["ocean"])
    nb, ncat, ntrcr, ny, nx = r["trcrn"].shape
    h = dict({k: r[k].copy() for k in rv.STATE + ["rdg_conv", "rdg_shear"]}, **copies(x, ["aice"] + iv.FLUX + iv.TEND + ["first_ice"]))
    h.update(vice=np.zeros((nb, ny, nx)), vsno=np.zeros((nb, ny, nx)), trcr=np.zeros((nb, ntrcr, ny, nx)))
    for k in iv.STATE:                                  # land and ghost cells are empty, as the model keeps them (the device leaves land cells alone)
        np.moveaxis(h[k], (0, -2, -1), (0, 1, 2))[~x["ocean"]] = 0.0
    dev = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    ctx.set_params(dyn.set_evp_parameters(rv.DT, 4, False, 1.0e4, krdg_partic=1, krdg_redist=1, ncat=5, mu_rdg=rv.MU_RDG))
    assert ctx.ridge_ice(r["dt"], r["ndtd"], dev["aice0"], dev["aicen"], dev["vicen"], dev["vsnon"], dev["trcrn"], r["ntrcr"], r["trcr_depend"],
                         r["tracers"], r["hin_max"], dev["rdg_conv"], dev["rdg_shear"], None) is None
    ridged = {k: dev[k].cpu().numpy() for k in rv.STATE}
    assert not np.array_equal(ridged["aicen"], h["aicen"])
    assert cleanup(ctx, x, dev) is None
    aggregate(ctx, x, dev, bound=True)
    torch.cuda.synchronize()
    xr = dict(x, **ridged)
    y, z, infos, stop = gen.restate(xr)
    assert stop is None
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    for k in iv.FLUX + ["first_ice"]:
        assert eq(gen.on_cells(got[k], x["ocean"]), gen.on_cells(y[k], x["ocean"])), k
    for k in iv.STATE:
        sel = x["ocean"] | ~x["phys"]
        assert eq(gen.on_cells(got[k], sel), gen.on_cells(z[k], sel)), k
    for k in ("aice", "vice", "vsno", "aice0", "trcr"):
        assert eq(got[k], z[k]), k
    for k in iv.TEND:
        assert eq(gen.on_cells(got[k], x["phys"]), gen.on_cells(z[k], x["phys"])), k


@pytest.mark.parametrize("name", list(iv.STOPS))
def test_stop_reason_block_and_cell(contexts, name):
    ref = np.load(os.path.join(GOLDEN, "ref_itd_stops.npz"))[name]
    ctx = contexts("g26x18_b8x5")
    x = iv.stop_input(name)
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    b = int(np.nonzero(ref[0])[0][0])
    assert cleanup(ctx, x, y) == (iv.STOPS[name]["reason"], b + 1, int(ref[1][b]), int(ref[2][b]))


def test_refusals(contexts):
    ctx = contexts("g26x18_b8x5")
    x = iv.itd_input("g26x18_b8x5", "plain")
    y = copies(x, iv.STATE + CELL2 + ["first_ice"])
    with pytest.raises(evpk.EvpkError, match="aerosol tracers"):
        cleanup(ctx, x, y, tr_aero=True)
    with pytest.raises(evpk.EvpkError, match="nbtrcr = 2"):
        cleanup(ctx, x, y, nbtrcr=2)
    with pytest.raises(evpk.EvpkError, match="heat_capacity = .false."):
        cleanup(ctx, x, y, heat_capacity=False)
    nb, ncat, _, ny, nx = x["trcrn"].shape
    x33 = dict(x, ntrcr=33, trcr_depend=np.zeros(33, dtype=np.int32))
    y33 = dict(y, trcrn=np.zeros((nb, ncat, 33, ny, nx)))
    with pytest.raises(evpk.EvpkError, match="ntrcr = 33 exceeds 32"):
        cleanup(ctx, x33, y33)
    z33 = dict(copies(x, iv.TEND), **{k: np.zeros((nb, ny, nx)) for k in ("aice", "vice", "vsno", "aice0")}, trcr=np.zeros((nb, 33, ny, nx)),
               **copies(y33, iv.STATE))
    with pytest.raises(evpk.EvpkError, match="ntrcr = 33 exceeds 32"):
        aggregate(ctx, x33, z33, bound=False)
    z = lambda *s: np.zeros(s)
    with pytest.raises(evpk.EvpkError, match="ncat = 17 not in"):
        ctx.cleanup_itd(3600.0, z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, ny, nx), z(nb, 17, 1, ny, nx), z(nb, ny, nx), z(nb, ny, nx), 1, [0],
                        dict(nt_Tsfc=1), np.zeros(18))
    for k in iv.STATE + CELL2 + ["first_ice"]:          # a refused call touches nothing
        assert eq(y[k], x[k]), k


def test_refusal_on_more_than_one_rank():
    from tests import util
    nx, ny, bx, by, _ = iv.CONFIGS["g26x18_b8x5"]
    _, d, f = util.make_case(nx, ny, bx, by, nprocs=2, rank=0)
    ctx = evpk.Context(d, f, defer_connect=True)    # (the geometry says two ranks; nothing collective has happened)
    try:
        nb, ny_, nx_ = d.nblocks, d.ny_block, d.nx_block
        z = lambda *s: np.zeros(s)
        with pytest.raises(evpk.EvpkError, match="nranks = 2"):
            ctx.cleanup_itd(3600.0, z(nb, 5, ny_, nx_), z(nb, 5, ny_, nx_), z(nb, 5, ny_, nx_), z(nb, 5, 1, ny_, nx_), z(nb, ny_, nx_), z(nb, ny_, nx_),
                            1, [0], dict(nt_Tsfc=1), iv.ridgevec.HIN_MAX)
        with pytest.raises(evpk.EvpkError, match="nranks = 2"):
            ctx.aggregate(3600.0, z(nb, 5, ny_, nx_), z(nb, 5, ny_, nx_), z(nb, 5, ny_, nx_), z(nb, 5, 1, ny_, nx_), z(nb, ny_, nx_), z(nb, ny_, nx_),
                          z(nb, ny_, nx_), z(nb, ny_, nx_), z(nb, 1, ny_, nx_), 1, [0], dict(nt_Tsfc=1))
    finally:
        ctx.close()
