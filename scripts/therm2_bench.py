#!/usr/bin/env python3
"""Time evpk_new_ice_lateral_melt (add_new_ice + lateral_melt of step_therm2, one launch: k_therm2_leads) on one MI355X with the ice state
resident in HBM, on the state scripts/itd_bench.py builds (12 tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl), ktherm = 1:
  (a) no frazil and no melt: frzmlt = -10, rside = 0 everywhere;
  (b) a winter mix: frzmlt = 20 .. 80 W/m2 on four ice cells in five -- thin frazil, all of it into category 1, no surplus -- and
      rside = 0.01 .. 0.05 on one ocean cell in five.
The yardstick, re-measured in the same run: evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py.
Then evpk_step_therm2 (kitd = 1) on PAGEABLE numpy arrays against the only way to run the same step without it: evpk_linear_itd and
evpk_cleanup_itd as two calls on the same pageable arrays (which stages the state twice and still leaves the two routines to the host).

    python scripts/therm2_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--no-pageable]

Compulsory bytes of k_therm2_leads, fp64, each array element once, per physical ocean cell:
  every cell          frzmlt, rside read, frazil written                                                               3
  a growing cell      aice0 read and written, aice, Tf read; aicen(1), vicen(1) read and written; Tsfc, qice x 4, sice x 4, alvl, vlvl of
                      category 1 read and written; salinz(1:4) read                                                    2 + 2 + 4 + 22 + 4 = 34
  a melting cell      aicen, vicen, vsnon of every category read and written (category 1's aicen, vicen once if it also grows);
                      qice x 4, qsno of every category read; fresh, fsalt, fhocn, meltl read and written               6 ncat + 5 ncat + 8
(surplus cells do not occur in these workloads; the script checks that.)  Prints one JSON line.
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
    ap.add_argument("--no-pageable", action="store_true", help="skip the evpk_step_therm2 comparison on pageable arrays")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, synth
    nx, ny = (int(v) for v in a.grid.split("x"))
    DEP, HIN_MAX = ib.DEP, ib.HIN_MAX
    TR = dict(ib.TR, nt_sice=7, nt_vlvl=12)
    ntrcr, ncat = len(DEP), a.ncat
    nilyr = TR["nilyr"]
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
    po = torch.from_numpy(lm).to(dev)
    cells = nb * nyb * nxb
    z2 = lambda: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev)
    state_planes = (3 + ntrcr) * ncat
    out = {"what": "evpk_new_ice_lateral_melt (k_therm2_leads), state resident in HBM; evpk_step_therm2 on pageable arrays", "grid": a.grid,
           "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "ktherm": 1, "cells": nx * ny, "block_array_cells": cells, "physical_ocean_cells": int(lm.sum()),
           "state_GB": 8 * cells * (state_planes + 1) / 1e9}

    def timed(fn, restore):
        times = []
        for _ in range(a.reps + 1):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return 1e3 * min(times[1:]), 1e3 * times[0]

    def stacked(shifting):
        an, vn, sn, t = ib.state(torch, X, Y, ocean, ncat, ntrcr, shifting, C)
        AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
        TN = torch.stack([torch.stack(q, dim=1) for q in t], dim=1).contiguous()          # (nb, ncat, ntrcr, ny, nx)
        return AN, VN, SN, TN

    AN, VN, SN, TN = stacked(False)
    AI, VI = AN.clone(), VN.clone()
    aice = AN.sum(dim=1)
    aice0 = torch.clamp(1.0 - aice, min=0.0)
    ice = aice > 1.0e-11
    prof = torch.tensor([2.0 + 1.2 * k for k in range(nilyr + 1)], dtype=torch.float64, device=dev)
    forcing = {"frzmlt": z2(), "rside": z2(), "Tf": z2() - 1.8, "sss": z2() + 34.0,
               "salinz": prof[None, :, None, None].expand(nb, nilyr + 1, nyb, nxb).contiguous()}
    fluxes = {k: z2() for k in ("frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn")}
    keep = [q.clone() for q in (AN, VN, SN, TN, aice0)]
    state = dict(aicen_init=AI, vicen_init=VI, aicen=AN, vicen=VN, vsnon=SN, trcrn=TN, aice=aice, aice0=aice0)
    grow_mask = po & ice & (torch.sin(37 * X) * torch.cos(29 * Y) > -0.8)                # four ice cells in five
    melt_mask = po & (torch.sin(53 * X + 1.0) * torch.cos(41 * Y) > 0.55)
    frz_b = torch.where(grow_mask, 50.0 + 30.0 * torch.sin(3 * X + Y), z2() - 10.0)
    rs_b = torch.where(melt_mask, 0.03 + 0.02 * torch.sin(5 * X - Y), z2())
    nocean = int(po.sum().item())

    def restore():
        for q, k in zip((AN, VN, SN, TN, aice0), keep):
            q.copy_(k)

    def call():
        ctx.new_ice_lateral_melt(dt, state, forcing, fluxes, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], ktherm=1)

    for name, frz, rs in (("a_no_frazil_no_melt", z2() - 10.0, z2()), ("b_winter_mix", frz_b, rs_b)):
        forcing["frzmlt"].copy_(frz)
        forcing["rside"].copy_(rs)
        ngrow = int((po & (frz > 0) & (aice0 > 1.0e-11)).sum().item())
        nmelt = int((po & (rs > 0)).sum().item())
        nboth = int((po & (frz > 0) & (rs > 0)).sum().item())
        gb = 8 * (3 * nocean + 34 * ngrow + (11 * ncat + 8) * nmelt - 4 * nboth) / 1e9
        ms, first = timed(call, restore)
        surplus = int((((VN[:, 1:] != keep[1][:, 1:]).any(dim=1)) & po & ~(rs > 0)).sum().item())
        assert surplus == 0, surplus
        out[name] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": gb, "GBps_of_compulsory": gb / (ms * 1e-3),
                     "ocean_cells": nocean, "growing_cells": ngrow, "melting_cells": nmelt,
                     "cells_whose_state_changed": int(((AN != keep[0]).any(dim=1) & po).sum().item())}
    del AN, VN, SN, TN, AI, VI, keep, state
    torch.cuda.empty_cache()

    # the yardstick: cleanup_itd where every block shifts (scripts/itd_bench.py, case b), same session, same box
    AN, VN, SN, TN = stacked(True)
    keep = [q.clone() for q in (AN, VN, SN, TN)]
    fl = {k: z2() for k in ("fpond", "fresh", "fsalt", "fhocn")}
    nlisted = int(lm.sum())
    a0, a1 = z2(), z2()

    def restore():
        for q, k in zip((AN, VN, SN, TN), keep):
            q.copy_(k)

    def call():
        assert ctx.cleanup_itd(dt, AN, VN, SN, TN, a0, a1, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], None, fl, None) is None
    ms, first = timed(call, restore)
    cgb = 8 * nlisted * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9 + 2 * 8 * nlisted * state_planes / 1e9
    out["cleanup_itd_b_every_block_shifts"] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": cgb,
                                               "GBps_of_compulsory": cgb / (ms * 1e-3)}
    for name in ("a_no_frazil_no_melt", "b_winter_mix"):
        out[name]["GBps_ratio_to_cleanup_itd_b"] = out[name]["GBps_of_compulsory"] / out["cleanup_itd_b_every_block_shifts"]["GBps_of_compulsory"]

    if not a.no_pageable:
        # one call on pageable arrays against linear_itd + cleanup_itd as two calls on the same pageable arrays (winter mix forcing)
        restore()
        torch.cuda.synchronize()
        H = {k: q.cpu().numpy() for k, q in (("aicen", AN), ("vicen", VN), ("vsnon", SN), ("trcrn", TN))}
        del AN, VN, SN, TN, keep
        torch.cuda.empty_cache()
        H["aicen_init"], H["vicen_init"] = H["aicen"].copy(), H["vicen"].copy()
        H["aice"], H["aice0"] = np.zeros((nb, nyb, nxb)), np.zeros((nb, nyb, nxb))
        fo = {k: v.cpu().numpy() for k, v in forcing.items()}
        fo["frain"] = np.zeros((nb, nyb, nxb))
        fx = {k: np.zeros((nb, nyb, nxb)) for k in fluxes}
        base = {k: H[k].copy() for k in ("aicen", "vicen", "vsnon")}

        def reset():
            for k in base:
                H[k][...] = base[k]

        def one():
            assert ctx.step_therm2(dt, H, fo, fx, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], kitd=1, ktherm=1, hi_min=HI_MIN) is None

        def two():
            assert ctx.linear_itd(H["aicen_init"], H["vicen_init"], H["aicen"], H["vicen"], H["vsnon"], H["trcrn"], H["aice"], H["aice0"], ntrcr, DEP, TR,
                                  HIN_MAX[:ncat + 1], HI_MIN) is None
            assert ctx.cleanup_itd(dt, H["aicen"], H["vicen"], H["vsnon"], H["trcrn"], H["aice0"], H["aice"], ntrcr, DEP, TR, HIN_MAX[:ncat + 1], None,
                                   {k: fx[k] for k in ("fpond", "fresh", "fsalt", "fhocn")}, None) is None
        t1, t2 = [], []
        for _ in range(3):                                  # alternating, the first round is the warm-up (it sizes the staging pools)
            for fn, acc in ((one, t1), (two, t2)):
                reset()
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        out["pageable"] = {"step_therm2_one_call_ms": round(1e3 * min(t1[1:]), 1), "linear_itd_plus_cleanup_itd_two_calls_ms": round(1e3 * min(t2[1:]), 1),
                           "first_round_ms": [round(1e3 * t1[0], 1), round(1e3 * t2[0], 1)],
                           "staged_up_GB_one_call": 8 * cells * (state_planes + 2 * ncat + 14 + nilyr + 1) / 1e9}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
