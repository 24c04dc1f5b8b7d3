#!/usr/bin/env python3
"""Time evpk_bound_state on K x-slab ranks: the packed path (k_bound_pack -> one message per partner -> k_bound_fill) against the
plane-by-plane path (EVPK_BOUND_DIRECT=0), ALTERNATING in the same run after a warm-up, the state resident in HBM.

    python scripts/bound_ranks_bench.py --shape cfg4            # 1440 x 1080 tripole in 30 x 27 blocks on 4 ranks
    python scripts/bound_ranks_bench.py --shape wide            # 3600 x 300 tripole in 450 x 150 blocks on 4 ranks

It starts the K rank processes itself: one per GPU where there are K GPUs, otherwise all on GPU 0 -- which times ranks SHARING one
GPU (the exchange is then a copy inside one HBM), not an exchange between GPUs.  5 categories x 12 tracers = 75 planes.  Every rank
synchronises its device around each call; a call's time is the slowest rank's.  One JSON line per setting: the median, the quartiles
(spread = p75 - p25) and the extremes over the repetitions, the exchange rounds and the planes the library reports.
"""
import argparse
import json
import os
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg4": (1440, 1080, 30, 27), "wide": (3600, 300, 450, 150)}
NCAT, NTRCR = 5, 12
SETTINGS = (("packed", "1"), ("plane_by_plane", "0"))


def worker(rank, world, dev, uid, shape, ns, reps, warmup, q):
    try:
        import torch
        from cice5_amd import blocks, constants as C, evpk, synth
        nx, ny, bx, by = shape
        d = blocks.create_distrb_cart(nx, ny, bx, by, nprocs=world, rank=rank, ns_boundary_type=ns)
        f = synth.make_block_fields(synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[ns], land="none"), d)
        ctx = evpk.Context(d, f, device=dev, unique_id=uid)
        torch.cuda.set_device(dev)
        g = torch.Generator(device="cuda").manual_seed(1 + rank)
        r = lambda *s: torch.rand(s, dtype=torch.float64, device="cuda", generator=g)
        nb, nyb, nxb = d.nblocks, d.ny_block, d.nx_block
        a, v, s, t = r(nb, NCAT, nyb, nxb), r(nb, NCAT, nyb, nxb), r(nb, NCAT, nyb, nxb), r(nb, NCAT, NTRCR, nyb, nxb)
        times = {name: [] for name, _ in SETTINGS}
        info = {}
        for k in range(warmup + reps):
            for name, knob in SETTINGS:
                os.environ["EVPK_BOUND_DIRECT"] = knob
                torch.cuda.synchronize()
                ctx.sync()
                t0 = time.perf_counter()
                ctx.bound_state(a, v, s, t, NTRCR)
                ctx.sync()
                dt = time.perf_counter() - t0
                if k >= warmup:
                    times[name].append(dt)
                st = ctx.stats()
                info[name] = (int(st.bound_state_rounds), int(st.bound_state_planes), int(st.transport))
        ctx.close()
        q.put((rank, None, times, info, nb))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc(), None, None, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg4", choices=sorted(SHAPES))
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xp", default="ipc", choices=["ipc", "shm", "rccl"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import multiprocessing as mp
    import torch
    from cice5_amd import evpk
    ngpu = int(torch.cuda.device_count())
    per_rank = ngpu >= a.ranks
    if a.xp == "rccl":
        assert per_rank, "RCCL refuses several ranks on one device"
        uid = evpk.get_unique_id()
    tag = "evpk_brb_" + uuid.uuid4().hex[:12]
    if a.xp != "rccl":
        uid = ({"shm": b"EVPKSHM:", "ipc": b"EVPKIPC:"}[a.xp] + tag.encode()).ljust(128, b"\0")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, a.ranks, r if per_rank else 0, uid, SHAPES[a.shape], a.ns, a.reps, a.warmup, q)) for r in range(a.ranks)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=900))
            if res[-1][1]:
                raise SystemExit(f"rank {res[-1][0]}: {res[-1][1]}")
    finally:
        for p in procs:
            p.join(timeout=1 if len(res) < a.ranks or res[-1][1] else 60)
            if p.is_alive():
                p.kill()
        try:
            os.unlink("/dev/shm/" + tag)
        except OSError:
            pass
    res.sort()
    nx, ny, bx, by = SHAPES[a.shape]
    for name, _ in SETTINGS:
        per_call = np.max(np.array([r[2][name] for r in res if r[4]]), axis=0) * 1e3          # the slowest rank of each call
        p25, med, p75 = (float(np.percentile(per_call, p)) for p in (25, 50, 75))
        rounds, planes, xp = res[0][3][name]
        print(json.dumps({"what": "evpk_bound_state on x-slab ranks, state resident in HBM", "setting": name, "shape": a.shape, "grid": f"{nx}x{ny}",
                          "blocks": f"{bx}x{by}", "ns": a.ns, "ranks": a.ranks, "gpus": a.ranks if per_rank else 1,
                          "ranks_share_one_gpu": not per_rank, "transport": a.xp, "ncat": NCAT, "ntrcr": NTRCR, "planes": planes,
                          "exchange_rounds": rounds, "reps": a.reps, "warmup": a.warmup, "median_ms": round(med, 3), "p25_ms": round(p25, 3),
                          "p75_ms": round(p75, 3), "spread_ms": round(p75 - p25, 3), "min_ms": round(float(per_call.min()), 3),
                          "max_ms": round(float(per_call.max()), 3)}))


if __name__ == "__main__":
    main()
