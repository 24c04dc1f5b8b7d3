#!/usr/bin/env python3
"""Time evpk_cleanup_itd and evpk_aggregate (the rest of step_ridge / step_dynamics) on one MI355X with the ice state resident in HBM
(the caller's arrays are device arrays):
  (a) a state in which nothing shifts and nothing is zapped -- the common case;
  (b) the same state with one cell in a few hundred thicker than its category bound, so that every block shifts and shift_ice rewrites
      the tracers of every cell with ice;
  aggregate alone (bound = 0) and with bound_state (bound = 1).

    python scripts/itd_bench.py --grid 3600x2700 --ns tripole --ncat 5

Tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl -- 12 (nilyr = 4, nslyr = 1).  Compulsory bytes, fp64, each array element once:
  (a) read aicen, vicen, vsnon, the snow enthalpies and aice0, write aice and aice0, on the listed cells;
  (b) (a) + every state plane read and written once;
  aggregate: every state plane read, aice, vice, vsno, aice0, trcr written, the two tendencies read and written, on every cell.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIN_MAX = np.array([0.0, 0.64, 1.39, 2.47, 4.57, 9.0])
DEP = np.array([0, 1, 1, 1, 1, 2, 1, 1, 1, 1, 0, 1], dtype=np.int32)
TR = dict(nt_Tsfc=1, nt_qice=2, nilyr=4, nt_qsno=6, nslyr=1, nt_alvl=11)


def state(xp, x, y, ocean, ncat, ntrcr, shifting, C):
    ice = ocean & (xp.sin(3 * x + 0.5) * xp.cos(2 * y) > -0.3)
    zero = 0.0 * (x + y)
    a = [xp.where(ice, 0.12 * (1 + 0.5 * xp.sin(n * x + y)), zero) for n in range(1, ncat + 1)]
    thick = ice & (xp.sin(211 * x) * xp.sin(173 * y) > 0.99) if shifting else (ice & False)
    v = []
    for n in range(ncat):
        h = float(HIN_MAX[n]) + (0.2 + 0.6 * (0.5 + 0.5 * xp.cos(x + n))) * float(HIN_MAX[n + 1] - HIN_MAX[n])
        if n == 1:
            h = xp.where(thick, zero + 1.2 * float(HIN_MAX[2]), h)
        v.append(a[n] * h)
    sn = [a[n] * 0.2 * (1 + 0.5 * xp.sin(2 * x - y)) for n in range(ncat)]
    t = [[(k + 1.0) * (0.5 + 0.3 * xp.cos(2 * x - y + k + n)) for k in range(ntrcr)] for n in range(ncat)]
    for n in range(ncat):
        t[n][TR["nt_qsno"] - 1] = -C.rhos * (C.Lfresh + C.cp_ice * (5.0 + 4.0 * xp.sin(x + n)))
        for k in range(TR["nilyr"]):
            t[n][TR["nt_qice"] - 1 + k] = -C.rhoi * (0.9 * C.Lfresh + C.cp_ice * (5.0 + 4.0 * xp.cos(y + n + k)))
    return a, v, sn, t


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
    listed, cells = int(lm.sum()), nb * nyb * nxb
    z2 = lambda: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev)
    aice0, aice, vice, vsno, daidtd, dvidtd = (z2() for _ in range(6))
    fl = {k: z2() for k in ("fpond", "fresh", "fsalt", "fhocn")}
    trcr = torch.zeros((nb, ntrcr, nyb, nxb), dtype=torch.float64, device=dev)
    state_planes = (3 + ntrcr) * ncat
    out = {"what": "evpk_cleanup_itd / evpk_aggregate, state resident in HBM", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr,
           "cells": nx * ny, "listed_cells": listed, "block_array_cells": cells, "state_GB": 8 * cells * (state_planes + 1) / 1e9}
    quiet_gb = 8 * listed * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9

    def timed(fn, restore):
        times = []
        for _ in range(a.reps + 1):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return 1e3 * min(times[1:]), 1e3 * times[0]

    for name, shifting in (("a_nothing_shifts", False), ("b_every_block_shifts", True)):
        an, vn, sn, t = state(torch, X, Y, ocean, ncat, ntrcr, shifting, C)
        AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
        TN = torch.stack([torch.stack(q, dim=1) for q in t], dim=1).contiguous()          # (nb, ncat, ntrcr, ny, nx)
        del an, vn, sn, t
        keep = [q.clone() for q in (AN, VN, SN, TN)]

        def restore():
            for q, k in zip((AN, VN, SN, TN), keep):
                q.copy_(k)

        def call():
            stop = ctx.cleanup_itd(dt, AN, VN, SN, TN, aice0, aice, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], None, fl, None)
            assert stop is None, stop
        ms, first = timed(call, restore)
        changed = int((TN != keep[3]).sum().item())
        gb = quiet_gb + (2 * 8 * listed * state_planes / 1e9 if shifting else 0.0)
        out[name] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": gb, "GBps_of_compulsory": gb / (ms * 1e-3),
                     "trcrn_values_changed": changed}
        if not shifting:
            assert changed == 0
            for bound in (0, 1):
                def agg():
                    ctx.aggregate(dt, AN, VN, SN, TN, aice, vice, vsno, aice0, trcr, ntrcr, DEP, TR, bound=bool(bound), daidtd=daidtd, dvidtd=dvidtd)
                ms, first = timed(agg, lambda: None)
                gb = 8 * cells * (state_planes + 4 + ntrcr + 4) / 1e9
                out[f"aggregate_bound{bound}"] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": gb,
                                                   "GBps_of_compulsory": gb / (ms * 1e-3)}
        del AN, VN, SN, TN, keep
        torch.cuda.empty_cache()
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
