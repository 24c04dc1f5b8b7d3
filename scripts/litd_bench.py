#!/usr/bin/env python3
"""Time evpk_linear_itd (the thermodynamic remapping of the thickness distribution, first part of step_therm2) on one MI355X with the ice
state resident in HBM (the caller's arrays are device arrays), on the state scripts/itd_bench.py builds:
  (a) vicen = vicen_init: no boundary moves -- but unlike cleanup_itd there is no "nothing shifts" fast path: the reference rewrites the
      tracers of every listed cell on every call;
  (b) a growth / melt mix: every category's thickness changes by up to +-12 %, so that ice moves up and down at every boundary.
The yardstick, re-measured in the same run: evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py.

    python scripts/litd_bench.py --grid 3600x2700 --ns tripole --ncat 5

Compulsory bytes, fp64, each array element once: aicen_init, vicen_init and every state plane read on every cell of the block arrays;
every state plane written on the listed cells; aice, aice0 written on every cell.  Prints one JSON line.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("itd_bench", os.path.join(ROOT, "scripts", "itd_bench.py"))
ib = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ib)

HI_MIN = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    nx, ny = (int(v) for v in a.grid.split("x"))
    DEP, TR, HIN_MAX = ib.DEP, ib.TR, ib.HIN_MAX
    ntrcr, ncat = len(DEP), a.ncat
    dt = 3600.0
    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[a.ns], land="continents")
    d = blocks.create_distrb_cart(nx, ny, nx // a.xblocks, ny, ns_boundary_type=a.ns)
    f = synth.make_block_fields(case, d)
    s = dyn.EvpDynamics(d, f, ndte=120, xmin=synth.global_min_dx(case))
    s.set_evp_parameters(dt)
    ctx = s.ctx
    I, J = blocks.block_index_windows(d)
    nb, nyb, nxb = d.nblocks, d.ny_block, d.nx_block
    dev = torch.device("cuda")
    X = torch.from_numpy(2 * np.pi * ((I - 1) % nx + 1) / nx).to(dev)[:, None, :].expand(nb, nyb, nxb)
    Y = torch.from_numpy(np.pi * J / ny).to(dev)[:, :, None].expand(nb, nyb, nxb)
    ocean = torch.from_numpy(f["tmask"] > 0).to(dev)
    lm = np.zeros(f["tmask"].shape, dtype=bool)
    for n, b in enumerate(d.local_blocks):
        lm[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = f["tmask"][n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] > 0
    physical_ocean = torch.from_numpy(lm).to(dev)
    cells = nb * nyb * nxb
    z2 = lambda: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev)
    aice0, aice = z2(), z2()
    state_planes = (3 + ntrcr) * ncat
    out = {"what": "evpk_linear_itd, state resident in HBM", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "cells": nx * ny,
           "block_array_cells": cells, "state_GB": 8 * cells * (state_planes + 1) / 1e9, "hi_min": HI_MIN}

    def timed(fn, restore):
        times = []
        for _ in range(a.reps + 1):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return 1e3 * min(times[1:]), 1e3 * times[0]

    def stacked(shifting):
        an, vn, sn, t = ib.state(torch, X, Y, ocean, ncat, ntrcr, shifting, C)
        AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
        TN = torch.stack([torch.stack(q, dim=1) for q in t], dim=1).contiguous()          # (nb, ncat, ntrcr, ny, nx)
        return AN, VN, SN, TN

    AN, VN, SN, TN = stacked(False)
    AI, VI = AN.clone(), VN.clone()
    listed = int((physical_ocean & (AN.sum(dim=1) > 1.0e-11)).sum().item())
    out["listed_cells"] = listed
    gb = 8 * (cells * (2 * ncat + state_planes + 2) + listed * state_planes) / 1e9
    keep = [q.clone() for q in (AN, VN, SN, TN)]
    cat = torch.arange(1, ncat + 1, dtype=torch.float64, device=dev)[None, :, None, None]
    mix = 1.0 + 0.12 * torch.sin(5 * X[:, None] + 3 * Y[:, None] + 1.7 * cat)
    for name, fac in (("a_no_thickness_change", None), ("b_growth_melt_mix", mix)):
        if fac is not None:
            keep[1] = VI * fac

        def restore():
            for q, k in zip((AN, VN, SN, TN), keep):
                q.copy_(k)

        def call():
            stop = ctx.linear_itd(AI, VI, AN, VN, SN, TN, aice, aice0, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], HI_MIN)
            assert stop is None, stop
        ms, first = timed(call, restore)
        moved = int(((AN != keep[0]).any(dim=1) & physical_ocean).sum().item())
        out[name] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": gb, "GBps_of_compulsory": gb / (ms * 1e-3),
                     "listed_cells": listed, "cells_whose_aicen_changed": moved}
    del AN, VN, SN, TN, AI, VI, keep, mix
    torch.cuda.empty_cache()

    # the yardstick: cleanup_itd where every block shifts (scripts/itd_bench.py, case b), same session, same box
    AN, VN, SN, TN = stacked(True)
    keep = [q.clone() for q in (AN, VN, SN, TN)]
    fl = {k: z2() for k in ("fpond", "fresh", "fsalt", "fhocn")}
    nlisted = int(lm.sum())

    def restore():
        for q, k in zip((AN, VN, SN, TN), keep):
            q.copy_(k)

    def call():
        assert ctx.cleanup_itd(dt, AN, VN, SN, TN, aice0, aice, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], None, fl, None) is None
    ms, first = timed(call, restore)
    cgb = 8 * nlisted * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9 + 2 * 8 * nlisted * state_planes / 1e9
    out["cleanup_itd_b_every_block_shifts"] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": cgb,
                                               "GBps_of_compulsory": cgb / (ms * 1e-3)}
    for name in ("a_no_thickness_change", "b_growth_melt_mix"):
        out[name]["GBps_ratio_to_cleanup_itd_b"] = out[name]["GBps_of_compulsory"] / out["cleanup_itd_b_every_block_shifts"]["GBps_of_compulsory"]
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
