#!/usr/bin/env python3
"""Time evpk_ridge_ice (ridge_ice) on one MI355X with the ice state resident in HBM (the caller's arrays are
device arrays), once on a state that converges in one ridging iteration and once on one whose blocks need two.

    python scripts/ridge_bench.py --grid 3600x2700 --ns tripole --ncat 5 --trcr 0,1,1,1,1,2,1,1,1,1,0,1

--trcr: trcr_depend of the tracers (0 area, 1 ice volume, 2 snow volume): the default is Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl --
12 tracers (nilyr = 4, nslyr = 1).  The number of iterations of each state is taken from the numpy restatement (tests/npridge.py) on a
small grid with the same state per (x, y).  Prints one JSON line.
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIN_MAX = np.array([0.0, 0.64, 1.39, 2.47, 4.57, 9.0])
HARD_ASUM, HARD_THIN = 1.08, 0.3       # the cells of the "strong" state that make their block repeat
DIAG_2D = ["dardg1dt", "dardg2dt", "dvirdgdt", "opening", "fpond", "fresh", "fhocn"]
DIAG_3D = ["dardg1ndt", "dardg2ndt", "dvirdgndt", "aparticn", "krdgn", "araftn", "vraftn", "aredistn", "vredistn"]


def state(xp, x, y, ocean, ncat, ntrcr, strong):
    """the state after "transport" as a function of (x, y) in [0, 2 pi) x [0, pi): areas that sum to 1.03 (mild: plenty of open water
    and thin ice to close, one iteration) or, on a few cells of the strong state, to 1.08 with no open water and little thin ice (the
    closing is cut back to what the thinnest categories hold, the block repeats).  xp: numpy or torch"""
    ice = ocean & (xp.sin(3 * x + 0.5) * xp.cos(2 * y) > -0.3)
    hard = ice & (xp.sin(11 * x) * xp.sin(7 * y) > 0.97) if strong else (ice & False)
    zero = 0.0 * (x + y)
    a = []
    for n in range(1, ncat + 1):
        w = 0.16 * (1 + 0.5 * xp.sin(n * x + y))
        w = xp.where(hard, w * (HARD_THIN if n <= 2 else 1.9), w)
        a.append(xp.where(ice, w, zero))
    tot = sum(a)
    a = [xp.where(hard, q * HARD_ASUM / xp.where(hard, tot, zero + 1.0), q) for q in a]          # hard cells: no open water, areas sum to HARD_ASUM
    a0 = xp.where(ocean & ~hard, 1.03 - tot, zero)
    a0 = xp.where(a0 > 0, a0, zero)
    hi = [float(0.5 * (HIN_MAX[n] + HIN_MAX[n + 1])) * (1 + 0.2 * xp.cos(x + n)) for n in range(ncat)]
    v = [a[n] * hi[n] for n in range(ncat)]
    sn = [a[n] * 0.2 * (1 + 0.5 * xp.sin(2 * x - y)) for n in range(ncat)]
    t = [[(k + 1.0) * (0.5 + 0.3 * xp.cos(2 * x - y + k + n)) for k in range(ntrcr)] for n in range(ncat)]
    conv = xp.where(ice, 2.0e-6 * (1 + xp.sin(x) * xp.cos(y)), zero)
    shear = xp.where(ice, 4.0e-6 * (1 + xp.cos(2 * x)), zero)
    return a0, a, v, sn, t, conv, shear


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--trcr", default="0,1,1,1,1,2,1,1,1,1,0,1")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--cpu-grid", default="48x36", help="grid of the restatement sample that counts the iterations (0 = skip)")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    nx, ny = (int(v) for v in a.grid.split("x"))
    dep = np.array([int(v) for v in a.trcr.split(",")], dtype=np.int32)
    ntrcr, ncat = len(dep), a.ncat
    tr = dict(nt_qsno=6, nslyr=1, nt_alvl=11, nt_vlvl=12) if ntrcr == 12 else {}
    dt, ndtd = 3600.0, 1

    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[a.ns], land="continents")
    d = blocks.create_distrb_cart(nx, ny, nx // a.xblocks, ny, ns_boundary_type=a.ns)
    f = synth.make_block_fields(case, d)
    s = dyn.EvpDynamics(d, f, ndte=120, xmin=synth.global_min_dx(case))
    s.set_evp_parameters(dt)
    I, J = blocks.block_index_windows(d)
    nb, nyb, nxb = d.nblocks, d.ny_block, d.nx_block
    dev = torch.device("cuda")
    X = torch.from_numpy(2 * np.pi * ((I - 1) % nx + 1) / nx).to(dev)[:, None, :].expand(nb, nyb, nxb)
    Y = torch.from_numpy(np.pi * J / ny).to(dev)[:, :, None].expand(nb, nyb, nxb)
    ocean = torch.from_numpy(f["tmask"] > 0).to(dev)
    lm = np.zeros(f["tmask"].shape, dtype=bool)                   # step_ridge's list: physical cells with tmask
    for n, b in enumerate(d.local_blocks):
        lm[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = f["tmask"][n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] > 0
    listed = int(lm.sum())
    lmask = torch.from_numpy(lm).to(dev)
    rt = evpk.RidgeTracers(**{k: int(tr.get(k, 0)) for k in evpk.RIDGE_TRACER_FIELDS})
    p64, p32 = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32)
    ptr = lambda t_: ct.cast(t_.data_ptr(), p64)
    L, ctx = s.ctx._L, s.ctx._ctx
    diag2 = {k: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev) for k in DIAG_2D}
    diag3 = {k: torch.zeros((nb, ncat, nyb, nxb), dtype=torch.float64, device=dev) for k in DIAG_3D}
    rd = evpk.RidgeDiag(**{k: ptr(v) for k, v in {**diag2, **diag3}.items()})
    stop = np.zeros(4, dtype=np.int32)
    out = {"what": "evpk_ridge_ice, state resident in HBM", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "cells": nx * ny,
           "listed_cells": listed}
    # (3 + ntrcr) * ncat + 1 planes read and written, two deformation planes read, the diagnostics written (three of them read too)
    planes = 2 * ((3 + ntrcr) * ncat + 1) + 2 + (len(DIAG_2D) + 3) + len(DIAG_3D) * ncat
    out["compulsory_GB"] = 8 * listed * planes / 1e9
    for name, strong in (("mild", False), ("strong", True)):
        a0, an, vn, sn, t, conv, shear = state(torch, X, Y, ocean, ncat, ntrcr, strong)
        A0 = a0.contiguous()
        AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
        TN = torch.stack([torch.stack(q, dim=1) for q in t], dim=1).contiguous()          # (nb, ncat, ntrcr, ny, nx)
        CV, SH = conv.contiguous(), shear.contiguous()
        del a0, an, vn, sn, t
        keep = [q.clone() for q in (A0, AN, VN, SN, TN)]
        times = []
        for r in range(a.reps + 1):
            for q, k in zip((A0, AN, VN, SN, TN), keep):
                q.copy_(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = L.evpk_ridge_ice(ctx, dt, ndtd, ncat, ntrcr, ntrcr, dep.ctypes.data_as(p32), ct.byref(rt), HIN_MAX[:ncat + 1].ctypes.data_as(p64),
                                  ptr(CV), ptr(SH), ptr(A0), ptr(AN), ptr(VN), ptr(SN), ptr(TN), ct.byref(rd), stop.ctypes.data_as(p32))
            times.append(time.perf_counter() - t0)
            assert rc == 0, (rc, stop, L.evpk_last_error(ctx))
        asum = A0 + AN.sum(dim=1)
        worst = float(((asum - 1.0).abs() * lmask).max())
        ms = 1e3 * min(times[1:])
        rec = {"ms_per_call": round(ms, 3), "first_call_ms": round(1e3 * times[0], 1), "max_abs_asum_minus_1_on_listed_cells": worst,
               "GBps_of_compulsory": out["compulsory_GB"] / (ms * 1e-3)}
        if a.cpu_grid != "0":
            from tests import npridge
            cx, cy = (int(v) for v in a.cpu_grid.split("x"))
            xs = (2 * np.pi * np.arange(1, cx + 1) / cx)[None, :] + np.zeros((cy, 1))
            ys = (np.pi * np.arange(1, cy + 1) / cy)[:, None] + np.zeros((1, cx))
            b0, bn, bv, bs, bt, bc, bsh = state(np, xs, ys, np.ones((cy, cx), dtype=bool), ncat, ntrcr, strong)
            res = npridge.ridge_ice_block(dt, ndtd, 1, 3.0, C.rhos, HIN_MAX[:ncat + 1], np.ones((cy, cx), dtype=np.int32), 1, cx, 1, cy, bc, bsh,
                                          b0, np.stack(bn), np.stack(bv), np.stack(bs), np.stack([np.stack(q) for q in bt]), ntrcr, dep, tr,
                                          None, npridge.dev_exp)
            rec["iterations_of_the_restatement_sample"] = 1 + res["repeats"]
        out[name] = rec
        del A0, AN, VN, SN, TN, CV, SH, keep
        torch.cuda.empty_cache()
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
