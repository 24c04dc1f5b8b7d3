#!/usr/bin/env python3
"""Time everything of step_dynamics behind evp on one MI355X, separate entry points against evpk_step_dynamics:
  (a) transport_remap_state -> ridge_ice -> cleanup_itd -> aggregate(bound = 1) as four calls from PAGEABLE host arrays
      (each call stages the category state up and down by itself);
  (b) evpk_step_dynamics from the same arrays (the union staged once);
  (c) both from device arrays;
  (d) evpk_aggregate with bound = 1 on the direct path (one launch of k_bound_state), with EVPK_BOUND_DIRECT=0 (plane by plane
      through the slab) and with bound = 0, from device arrays.

    python scripts/step_bench.py --grid 3600x2700 --ns tripole --ncat 5
    EVPK_LIB=/path/to/parent/libevpk.so python scripts/step_bench.py --only a          # the same arrays under another build

A library without evpk_step_dynamics (the parent commit's) runs (a) and the separate half of (c) and (d) only.  If the full
sequence stops in a stage on the synthetic state (the line says where), the run falls back to cleanup_itd -> aggregate alone
(advection = 0, ridge = 0), where the separate path is two calls.  State and tracers as scripts/itd_bench.py (12 tracers, nothing
shifts).  pcie_GB_model: the bytes the calls copy up and down, counted from the array sizes (not measured).
Prints one JSON line; min / median / max over --reps timed calls after one warm-up call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STATE = ["aice0", "aicen", "vicen", "vsnon", "trcrn"]
FLUX = ["fpond", "fresh", "fsalt", "fhocn"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="abcd", help="which of a, b, c, d to run")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import itd_bench as ib
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    import ctypes as ct
    have_step = hasattr(ct.CDLL(evpk.LIB_PATH), "evpk_step_dynamics")
    if not have_step:
        # an older build under EVPK_LIB: evpk.lib() binds every symbol of THIS tree's header, so the ones that build lacks get a stand-in
        # that takes the argtypes / restype assignments; calling one fails
        class _Absent:
            def __call__(self, *args):
                raise evpk.EvpkError("this build of libevpk.so does not export the symbol")

        class _OlderBuild(ct.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("evpk_"):
                        raise
                    fn = _Absent()
                    setattr(self, name, fn)
                    return fn
        real, ct.CDLL = ct.CDLL, _OlderBuild
        try:
            evpk.lib()
        finally:
            ct.CDLL = real
    nx, ny = (int(v) for v in a.grid.split("x"))
    DEP, TR, HIN = ib.DEP, dict(ib.TR), ib.HIN_MAX[:a.ncat + 1]
    ntrcr, ncat = len(DEP), a.ncat
    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[a.ns], land="continents")
    d = blocks.create_distrb_cart(nx, ny, nx // a.xblocks, ny, ns_boundary_type=a.ns)
    f = synth.make_block_fields(case, d)
    synth.add_remap_grid(case, d, f)
    xmin = synth.global_min_dx(case)
    s = dyn.EvpDynamics(d, f, ndte=120, xmin=xmin)
    s.init_evp(3600.0)
    s.evp(3600.0)                       # the velocities and the deformation rates transport and ridging read, resident on the device
    ctx = s.ctx
    ctx.remap_init(f["dxu"], f["dyu"], f["hm"])
    umax = max(float(np.abs(f["uvel"]).max()), float(np.abs(f["vvel"]).max()), 1e-9)
    dt = min(3600.0, 0.4 * xmin / umax)
    I, J = blocks.block_index_windows(d)
    nb, nyb, nxb = d.nblocks, d.ny_block, d.nx_block
    dev = torch.device("cuda")
    X = torch.from_numpy(2 * np.pi * ((I - 1) % nx + 1) / nx).to(dev)[:, None, :].expand(nb, nyb, nxb)
    Y = torch.from_numpy(np.pi * J / ny).to(dev)[:, :, None].expand(nb, nyb, nxb)
    ocean = torch.from_numpy(f["tmask"] > 0).to(dev)
    an, vn, sn, t = ib.state(torch, X, Y, ocean, ncat, ntrcr, False, C)
    D0 = dict(aicen=torch.stack(an, dim=1).contiguous(), vicen=torch.stack(vn, dim=1).contiguous(), vsnon=torch.stack(sn, dim=1).contiguous(),
              trcrn=torch.stack([torch.stack(q, dim=1) for q in t], dim=1).contiguous())
    del an, vn, sn, t
    D0["aice0"] = torch.where(ocean, 1.0 - D0["aicen"].sum(dim=1), torch.zeros_like(X)).contiguous()
    z2 = lambda: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev)
    for k in ["aice", "vice", "vsno", "daidtd", "dvidtd"] + FLUX:
        D0[k] = z2()
    D0["trcr"] = torch.zeros((nb, ntrcr, nyb, nxb), dtype=torch.float64, device=dev)
    cells = nb * nyb * nxb
    planes = {k: int(v.numel() // cells) for k, v in D0.items()}
    tables = evpk.remap_tracer_tables(DEP) if hasattr(evpk, "remap_tracer_tables") else None
    if tables is None:
        from oracle import orc
        tables = orc.remap_tables(list(DEP))
    rt = {k: TR.get(k, 0) for k in evpk.RIDGE_TRACER_FIELDS}
    out = {"what": "step_dynamics behind evp: separate entry points vs evpk_step_dynamics", "label": a.label, "lib": evpk.LIB_PATH, "grid": a.grid,
           "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "blocks": nb, "block_array_cells": cells, "dt": dt, "reps": a.reps,
           "state_GB": 8 * cells * ((3 + ntrcr) * ncat + 1) / 1e9, "has_step_dynamics": bool(have_step)}

    def separate(y, full):
        if full:
            rc = ctx.transport_remap_state(dt, *[y[k] for k in STATE], ntrcr, TR["nt_qsno"], TR["nslyr"], C.rhos * C.Lfresh, *tables)
            if rc:
                return ("transport", rc)
            st = ctx.ridge_ice(dt, 1, *[y[k] for k in STATE], ntrcr, DEP, rt, HIN, None, None, {k: y[k] for k in ("fpond", "fresh", "fhocn")})
            if st:
                return ("ridge_ice",) + st
        st = ctx.cleanup_itd(dt, y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice0"], y["aice"], ntrcr, DEP, TR, HIN, None,
                             {k: y[k] for k in FLUX}, None)
        if st:
            return ("cleanup_itd",) + st
        ctx.aggregate(dt, y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["vice"], y["vsno"], y["aice0"], y["trcr"], ntrcr, DEP, TR,
                      bound=True, daidtd=y["daidtd"], dvidtd=y["dvidtd"])
        return None

    def one_call(y, full):
        return ctx.step_dynamics(dt, 1, y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["vice"], y["vsno"], y["trcr"], ntrcr,
                                 DEP, TR, HIN, advection=2 if full else 0, ridge=full, fluxes={k: y[k] for k in FLUX}, daidtd=y["daidtd"],
                                 dvidtd=y["dvidtd"], tracer_type=tables[0], depend=tables[1], has_dependents=tables[2])

    def timed(fn, restore, reps):
        ts = []
        for _ in range(reps + 1):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
            if r is not None:
                return {"stopped": [str(v) for v in r]}
        w = ts[1:]
        return {"ms_min": round(min(w), 3), "ms_median": round(statistics.median(w), 3), "ms_max": round(max(w), 3), "first_call_ms": round(ts[0], 1)}

    # does the whole sequence run on this state?  (device arrays: cheap to find out)
    Dw = {k: v.clone() for k, v in D0.items()}
    stop = separate(Dw, True)
    full = stop is None
    out["sequence"] = "transport_remap_state, ridge_ice, cleanup_itd, aggregate" if full else "cleanup_itd, aggregate"
    if not full:
        out["full_sequence_stopped"] = [str(v) for v in stop]

    def restore_dev():
        for k in D0:
            Dw[k].copy_(D0[k])

    gb = lambda names: 8 * cells * sum(planes[k] for k in names) / 1e9
    if full:
        up_sep = gb(STATE) + gb(STATE + ["fpond", "fresh", "fhocn"]) + gb(STATE[1:] + ["aice0", "aice"] + FLUX) + gb(STATE[1:] + ["aice0", "aice", "vice", "vsno", "trcr", "daidtd", "dvidtd"])
    else:
        up_sep = gb(STATE[1:] + ["aice0", "aice"] + FLUX) + gb(STATE[1:] + ["aice0", "aice", "vice", "vsno", "trcr", "daidtd", "dvidtd"])
    out["pcie_GB_model"] = {"separate_each_way": up_sep, "step_dynamics_each_way": gb(list(D0))}

    if "c" in a.only:
        out["c_device_separate"] = timed(lambda: separate(Dw, full), restore_dev, max(a.reps, 5))
        if have_step:
            out["c_device_step_dynamics"] = timed(lambda: one_call(Dw, full), restore_dev, max(a.reps, 5))
    if "d" in a.only:
        restore_dev()
        if not full:
            separate(Dw, False)

        def agg(bound):
            ctx.aggregate(dt, Dw["aicen"], Dw["vicen"], Dw["vsnon"], Dw["trcrn"], Dw["aice"], Dw["vice"], Dw["vsno"], Dw["aice0"], Dw["trcr"], ntrcr, DEP,
                          TR, bound=bound, daidtd=Dw["daidtd"], dvidtd=Dw["dvidtd"])
        out["d_aggregate_bound0"] = timed(lambda: agg(False), lambda: None, 10)
        out["d_aggregate_bound1"] = timed(lambda: agg(True), lambda: None, 10)
        os.environ["EVPK_BOUND_DIRECT"] = "0"
        out["d_aggregate_bound1_plane_by_plane"] = timed(lambda: agg(True), lambda: None, 10)
        del os.environ["EVPK_BOUND_DIRECT"]
        if have_step:
            out["d_bound_state_alone"] = timed(lambda: ctx.bound_state(Dw["aicen"], Dw["vicen"], Dw["vsnon"], Dw["trcrn"], ntrcr), lambda: None, 10)
    if "a" in a.only or "b" in a.only:
        H0 = {k: v.cpu().numpy() for k, v in D0.items()}
        del Dw
        torch.cuda.empty_cache()
        Hw = {k: v.copy() for k, v in H0.items()}
        assert not evpk.host_is_mapped(Hw["trcrn"])

        def restore_host():
            for k in H0:
                Hw[k][...] = H0[k]
        if "a" in a.only:
            out["a_pageable_separate"] = timed(lambda: separate(Hw, full), restore_host, a.reps)
        if "b" in a.only and have_step:
            out["b_pageable_step_dynamics"] = timed(lambda: one_call(Hw, full), restore_host, a.reps)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
