"""Seeded random configurations of the single-rank path against the oracle, bit for bit: grid and block shapes (blocks that
do not divide the grid, i.e. padded edge blocks), boundary types, ndte parity, classic / revised EVP, ocean turning angle,
ice cover (polar / full / wandering patches / isolated cells), library modes.  Cheap cases, many of them: the point is
the corners nobody thought of writing a test for."""
import os

import numpy as np
import pytest

from cice5_amd import blocks, constants as C, dyn, synth
from oracle import orc
from tests import util

pytestmark = pytest.mark.gpu

# ({"EVPK_TILE": "1", "EVPK_STRIP_ROWS": "13"}: the sixteen-wave tile; the slot once held {"EVPK_PREFETCH": "0"}, then {"EVPK_TILE": "2"},
#  whose kernels were retired and are refused -- it stays a slot: the list's length and order decide every seed's draw)
MODES = [{}, {"EVPK_FORCE_EXCHANGE": "1"}, {"EVPK_DOUBLE": "0"}, {"EVPK_TILE": "1", "EVPK_STRIP_ROWS": "13"},
         {"EVPK_FORCE_EXCHANGE": "1", "EVPK_ZONE_M": "2"},
         {"EVPK_COMPACT_METRICS": "0"}, {"EVPK_STRIP_ROWS": "3"}, {"EVPK_FORCE_EXCHANGE": "1", "EVPK_OVERLAP": "0"},
         {"EVPK_FORCE_EXCHANGE": "2"}, {"EVPK_FORCE_EXCHANGE": "2", "EVPK_ZONE_M": "1"},
         {"EVPK_TILE": "1"}, {"EVPK_TILE": "1", "EVPK_FORCE_EXCHANGE": "1"}, {"EVPK_TILE": "1", "EVPK_STRIP_ROWS": "2"}, {"EVPK_TILE": "0"}]


def _config(seed):
    rng = np.random.default_rng(1000 + seed + int(os.environ.get("EVPK_FUZZ_BASE", "0")))
    if os.environ.get("EVPK_FUZZ_BIG"):          # many strip columns / rows: the strip-height tuner, several rounds of workgroups
        nx = int(rng.choice([733, 1000, 1464, 2048]))
        ny = int(rng.choice([257, 400, 701]))
    else:
        nx = int(rng.choice([8, 24, 61, 62, 64, 96, 122, 123, 130, 200, 371, 733]))
        ny = int(rng.choice([10, 12, 23, 40, 57, 64, 131, 257]))
    ns = str(rng.choice(["open", "open", "tripole", "closed"]))
    ew = str(rng.choice(["cyclic", "cyclic", "open", "closed"]))
    if ns == "tripole":
        ew = "cyclic"
        nx += nx & 1                                   # the fold needs an even nx_global
    bsx = int(rng.choice([nx, max(3, nx // 2), max(3, nx // 3 + 1), 7, 20]))
    bsy = int(rng.choice([ny, max(3, ny // 2), max(3, ny // 3 + 1), 5]))
    bsx, bsy = min(bsx, nx), min(bsy, ny)
    if ns == "tripole" and ny % bsy == 1 and bsy < ny:
        bsy += 1           # a one-row top block is rejected (the reference's own result then depends on the decomposition)
    return dict(nx=nx, ny=ny, bsx=bsx, bsy=bsy, ns=ns, ew=ew, ndte=int(rng.choice([1, 2, 5, 8, 13, 20])),
                revised=bool(rng.random() < 0.3), turn=bool(rng.random() < 0.3), ice=str(rng.choice(["polar", "full", "patches", "dots"])),
                land=str(rng.choice(["rows", "continents"])), mode=MODES[int(rng.integers(len(MODES)))], ncalls=int(rng.choice([1, 2, 3])),
                resident=bool(rng.random() < 0.5), pin=bool(rng.random() < 0.2), sparse=bool(rng.random() < 0.25),
                tilt=bool(rng.random() < 0.2), ugrid_wind=bool(rng.random() < 0.2), dt=float(rng.choice([3600.0, 900.0, 7200.0])),
                strength=(None if rng.random() < 0.6 else dict(kstrength=int(rng.integers(0, 2)), krdg_partic=int(rng.integers(0, 2)),
                                                                 krdg_redist=int(rng.integers(0, 2)))), rng=rng)


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVPK_FUZZ_N", "40"))))
def test_random_configuration(seed, monkeypatch):
    k = _config(seed)
    k["sparse"] = k["sparse"] and k["resident"] and not k["ugrid_wind"]      # sparse transfers: resident state, page-locked arrays
    k["pin"] = k["pin"] or k["sparse"] or bool(os.environ.get("EVPK_FUZZ_PIN"))      # (EVPK_FUZZ_PIN=1: every draw through page-locked arrays)
    for name, v in k["mode"].items():
        monkeypatch.setenv(name, v)
    case = synth.SynthCase(nx=k["nx"], ny=k["ny"], ns_boundary=C.BND_NAMES[k["ns"]], ew_boundary=C.BND_NAMES[k["ew"]],
                           land=k["land"], ice="full" if k["ice"] != "polar" else "polar")
    d = blocks.create_distrb_cart(k["nx"], k["ny"], k["bsx"], k["bsy"], ew_boundary_type=k["ew"], ns_boundary_type=k["ns"])
    f = synth.make_block_fields(case, d)
    base = util.clone(f)
    xmin = synth.global_min_dx(case)
    cosw, sinw = (np.cos(0.4), np.sin(0.4)) if k["turn"] else (1.0, 0.0)
    fo, fg = util.clone(f), util.clone(f)
    skw = dict(strength_mode=1, **k["strength"]) if k["strength"] else {}
    dt = k["dt"]
    p = orc.make_params(dt, k["ndte"], xmin, revised_evp=k["revised"], cosw=cosw, sinw=sinw, tilt_from_slope=k["tilt"],
                        wind_on_ugrid=k["ugrid_wind"], **skw)
    s = dyn.EvpDynamics(d, fg, ndte=k["ndte"], revised_evp=k["revised"], xmin=xmin, cosw=cosw, sinw=sinw,
                        tilt_from_slope=k["tilt"], wind_on_ugrid=k["ugrid_wind"], device_strength=k["strength"], pin_host=k["pin"],
                        sparse_io=k["sparse"])
    s.init_evp(dt)
    I, J = blocks.block_index_windows(d)
    nxg, nyg = d.nx_global, d.ny_global
    rng = k["rng"]
    for call in range(k["ncalls"]):
        if k["ice"] in ("patches", "dots"):
            kx, ky, ph = rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5), rng.uniform(0, 6.28)
            for ff in (fo, fg):
                for n in range(d.nblocks):
                    Ig = np.broadcast_to(I[n][None, :], (d.ny_block, d.nx_block)).copy()
                    Jg = np.broadcast_to(J[n][:, None], (d.ny_block, d.nx_block)).copy()
                    if k["ew"] == "cyclic":
                        Ig = (Ig - 1) % nxg + 1
                    if k["ns"] == "tripole":
                        top = Jg > nyg
                        Ig[top] = nxg - Ig[top] + 1
                        Jg = np.minimum(Jg, nyg)
                    w = np.sin(kx * Ig + ph) * np.cos(ky * Jg - ph)
                    keep = (w > (0.97 if k["ice"] == "dots" else 0.2)).astype(np.float64)
                    for name in ("aice", "vice", "vsno", "aice_init", "strength"):
                        ff[name][n] = base[name][n] * keep
        elif call:
            for ff in (fo, fg):
                ff["aice"] *= 0.9
                ff["vice"] *= 0.9
        if k["strength"]:
            for ff in (fo, fg):
                synth.add_thickness_distribution(ff)
        if k["sparse"]:                        # its precondition: no T-grid forcing where there is no ice
            for ff in (fo, fg):
                for name in ("strairxT", "strairyT"):
                    ff[name][...] = np.where(ff["aice"] > 0.0, base[name], 0.0)
        fin = util.clone(fo) if call == 0 else None        # (kept for the second runs below, should this draw differ)
        nt, nu, _ = orc.evp(d, p, fo)
        if k["resident"] and call:             # the state stays on the device: inputs only, then the staged calls
            s.ctx.upload_inputs(fg)
            s.ctx.prep(); s.ctx.subcycle(k["ndte"]); s.ctx.finish(); s.ctx.download(fg)
        else:
            s.evp(dt)
        st = s.ctx.stats()
        desc = {a: b for a, b in k.items() if a != "rng"}
        assert (st.icellt, st.icellu) == (nt, nu), (desc, call)
        bad = util.compare(d, fg, fo)
        if bad and call == 0:
            # One draw in ~17 000 differed in round 4 and never again (profiles/r04_v6/fuzz.txt): say which side moves, should it recur
            # -- the oracle once more from the same inputs, the device once more in a fresh context, then where the values differ
            f2 = util.clone(fin)
            orc.evp(d, p, f2)
            f3 = util.clone(fin)
            s3 = dyn.EvpDynamics(d, f3, ndte=k["ndte"], revised_evp=k["revised"], xmin=xmin, cosw=cosw, sinw=sinw, tilt_from_slope=k["tilt"],
                                 wind_on_ugrid=k["ugrid_wind"], device_strength=k["strength"], pin_host=k["pin"], sparse_io=k["sparse"])
            s3.init_evp(dt); s3.evp(dt); s3.close()
            where = [(n, [tuple(int(v) for v in ix) for ix in np.argwhere(fg[n] != fo[n])[:4]]) for n, _, _ in bad[:4]]
            bad = bad[:4] + [("oracle repeats itself", not util.compare(d, f2, fo)), ("device repeats itself", not util.compare(d, f3, fg)),
                             ("second device run equals the oracle", not util.compare(d, f3, fo)), ("where (block, j, i)", where)]
        assert not bad, (desc, call, bad)
    s.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVPK_FUZZ_R_N", "24"))))
def test_random_remap_configuration(seed, monkeypatch):
    """horizontal_remap (row f-3) on random grids / decompositions / boundaries / tracer trees / options, one rank, also through
    the general halo path: bit-identical with the oracle"""
    from cice5_amd import evpk
    k = _config(seed + 500)
    rng = k["rng"]
    if rng.random() < 0.4:
        monkeypatch.setenv("EVPK_FORCE_EXCHANGE", "1")
    nx, ny = max(k["nx"], 12), max(k["ny"], 12)
    nx += (k["ns"] == "tripole") and (nx & 1)
    trees = [(0, 1, 2 + 1), (0, 1, 2 + 1, 2 + 2), (1, 1, 2), (0,), (), (0, 2 + 1, 2 + 2, 1, 2 + 4)]
    dep = trees[int(rng.integers(len(trees)))]
    case, d, f, mm, tm, tables = util.remap_case(nx, ny, min(k["bsx"], nx), min(k["bsy"], ny), ns=k["ns"], ew=k["ew"], land=k["land"],
                                                 ncat=int(rng.integers(1, 5)), trcr_depend=dep)
    order, midpt = int(rng.integers(1, 4)), bool(rng.random() < 0.5)
    umax = max(np.abs(f["uvel"]).max(), np.abs(f["vvel"]).max(), 1e-9)
    dt = float(rng.uniform(0.05, 0.45)) * synth.global_min_dx(case) / umax
    mo, to, mg, tg = mm.copy(), tm.copy(), mm.copy(), tm.copy()
    rco = orc.horizontal_remap(d, dt, f, mo, to, *tables, integral_order=order, l_dp_midpt=midpt)
    s = dyn.EvpDynamics(d, f, ndte=10, xmin=1.0e4)
    s.set_evp_parameters(3600.0)
    s.ctx.upload(f)
    s.ctx.remap_init(f["dxu"], f["dyu"], f["hm"])
    rcg = s.ctx.transport_remap(dt, mg, tg if tg.shape[2] else None, *tables, integral_order=order, l_dp_midpt=midpt)
    if rng.random() < 0.5 and rco == 0:
        # ... and transport_remap whole (state_to_tracers / tracers_to_state / bound_state on the device too), same context
        from tests.test_parity_gpu import _ice_state
        ntrcr = int(rng.integers(0, 5)); ntrcr_dim = ntrcr + int(rng.integers(0, 3))
        nt_qsno, nslyr = (int(rng.integers(1, ntrcr + 1)), 1) if ntrcr else (1, 0)
        tb2 = orc.remap_tables([int(rng.choice([0, 1, 2])) for _ in range(ntrcr)])
        st = _ice_state(d, f, ntrcr, max(ntrcr_dim, 1), nt_qsno, nslyr)
        so, sg = [a.copy() for a in st], [a.copy() for a in st]
        r1 = orc.transport_remap_state(d, dt, f, *so, ntrcr, nt_qsno, nslyr, 1.1e8, *tb2, integral_order=order, l_dp_midpt=midpt)
        r2 = s.ctx.transport_remap_state(dt, *sg, ntrcr, nt_qsno, nslyr, 1.1e8, *tb2, integral_order=order, l_dp_midpt=midpt)
        assert {0: 0, 1: evpk.REMAP_BAD_DEPARTURE, 2: evpk.REMAP_NEGATIVE_MASS}[r1] == r2
        if r1 == 0:
            every = util.cell_mask(d, "all")
            for name, a, b_ in zip(("aice0", "aicen", "vicen", "vsnon", "trcrn"), sg, so):
                m = np.broadcast_to(every if a.ndim == 3 else (every[:, None] if a.ndim == 4 else every[:, None, None]), a.shape)
                assert np.array_equal(a[m], b_[m]), (name, {n: v for n, v in k.items() if n != "rng"})
    s.close()
    assert {0: 0, 1: evpk.REMAP_BAD_DEPARTURE, 2: evpk.REMAP_NEGATIVE_MASS}[rco] == rcg, (rco, rcg, k)
    if rco == 0:
        assert np.array_equal(mg, mo) and np.array_equal(tg, to), {n: v for n, v in k.items() if n != "rng"}


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVPK_FUZZ_E_N", "20"))))
def test_random_eap_configuration(seed, monkeypatch):
    """eap(dt) (row f-4) on random grids / decompositions / boundaries / ndte / classic and revised relaxation / turning angle,
    one to three calls, also as a forced exchange: bit-identical with the oracle"""
    from cice5_amd.eap_tables import eap_tables
    k = _config(seed + 900)
    rng = k["rng"]
    if rng.random() < 0.4:
        monkeypatch.setenv("EVPK_FORCE_EXCHANGE", "1")
    case = synth.SynthCase(nx=k["nx"], ny=k["ny"], ns_boundary=C.BND_NAMES[k["ns"]], ew_boundary=C.BND_NAMES[k["ew"]],
                           land=k["land"], ice="full" if k["ice"] != "polar" else "polar")
    d = blocks.create_distrb_cart(k["nx"], k["ny"], k["bsx"], k["bsy"], ew_boundary_type=k["ew"], ns_boundary_type=k["ns"])
    f = synth.make_block_fields(case, d)
    synth.add_eap_state(f)
    T = eap_tables()
    xmin = synth.global_min_dx(case)
    cosw, sinw = (np.cos(0.4), np.sin(0.4)) if k["turn"] else (1.0, 0.0)
    ndte = int(rng.choice([1, 2, 9, 10, 11, 21, 32]))
    fo, fg = util.clone(f), util.clone(f)
    p = orc.make_params(k["dt"], ndte, xmin, revised_evp=k["revised"], cosw=cosw, sinw=sinw, tilt_from_slope=k["tilt"])
    s = dyn.EvpDynamics(d, fg, ndte=ndte, revised_evp=k["revised"], xmin=xmin, cosw=cosw, sinw=sinw, tilt_from_slope=k["tilt"],
                        resident=k["resident"])
    s.init_eap(k["dt"], T)
    ne = util.cell_mask(d, "ne")
    for call in range(k["ncalls"]):
        if call:
            for ff in (fo, fg):
                ff["aice"] *= 0.8; ff["vice"] *= 0.8
                ff["strairxT"], ff["strairyT"] = ff["strairyT"].copy(), -ff["strairxT"]
        orc.eap(d, p, fo, T)
        s.eap(k["dt"])
        bad = util.compare(d, fg, fo)
        for n in synth.EAP_STATE + synth.EAP_HISTORY:
            if not np.array_equal(fg[n][ne], fo[n][ne]):
                bad.append((n, int((fg[n][ne] != fo[n][ne]).sum())))
        assert not bad, (call, bad[:6], {n: v for n, v in k.items() if n != "rng"})
    s.close()

