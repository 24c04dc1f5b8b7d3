#!/usr/bin/env python3
"""Time evpk_thermo_vertical (thermo_vertical, BL99, one launch: k_thermo_vertical<5, 4, 1>) on one MI355X with the ice state resident in
HBM, on the areas and thicknesses scripts/itd_bench.py builds (12 tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl) under a vertical
state and a forcing of this script's own:
  (a) a cold winter mix: air at 243 .. 263 K, no shortwave, 5 .. 25 cm of snow on four columns in five, ice at -5 .. -20 C;
  (b) a melting mix: air at 271 .. 277 K, 40 .. 150 W m-2 of shortwave, ice at -0.5 .. -3 C under a surface at 0 C on half the cells.
The yardstick, re-measured in the same run: evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py.
Iteration counts: the library does not return them, so the numpy restatement (tests/nptherm1.py) is run on a sample -- `--sample-rows`
rows of `--sample-waves` x 64 consecutive cells of one block, every category -- which is also compared bit for bit with what the device
returned there.  Reported: the histogram of the iteration count per (cell, category), and the mean over (wave, category) of the largest
count among the wave's 64 lanes, which is what a wave pays.
Then the same call on PAGEABLE numpy arrays against the cost of the state round trip it replaces (aicen, vicen, vsnon, trcrn down to
pageable memory and up again).

    python scripts/therm1_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--no-pageable]

Compulsory bytes, fp64, each array element once:
  a listed (cell, category)     aicen, vicen, vsnon read, vicen, vsnon written; Tsfc, qice x 4, qsno read and written, sice x 4 read; shcoef,
                                lhcoef read; fswsfcn, fswintn, Sswabsn, Iswabsn x 4 read and written; fifteen outputs written      52
  any other (cell, category)    fifteen zeros written, on ocean cells aicen read                                                    15 | 16
  a physical ocean cell         flw, potT, Qa, rhoa, fsnow, fbot, Tbot, mlt_onset, frz_onset read; with a listed category the two
                                onsets written                                                                                       9 | 11
Prints one JSON line.
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

CP_OCN, DEPRESST = 4218.0, 0.054
OUT15 = ["flwoutn", "evapn", "freshn", "fsaltn", "fhocnn", "fsensn", "flatn", "fsurfn", "fcondtopn", "melttn", "meltsn", "meltbn", "congeln",
         "snoicen", "dsnown"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--sample-rows", type=int, default=4)
    ap.add_argument("--sample-waves", type=int, default=3)
    ap.add_argument("--no-pageable", action="store_true", help="skip the call on pageable arrays")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    from tests import nptherm1
    nx, ny = (int(v) for v in a.grid.split("x"))
    DEP, HIN_MAX = ib.DEP, ib.HIN_MAX
    TR = dict(ib.TR, nt_sice=7, nt_vlvl=12)
    K = dict(Tocnfrz=C.Tocnfrz, ice_ref_salinity=C.ice_ref_salinity, hs_min=C.hs_min, cp_ice=C.cp_ice, Lfresh=C.Lfresh, Tmin=C.Tmin, puny=C.puny)
    ntrcr, ncat = len(DEP), a.ncat
    nilyr, nslyr = TR["nilyr"], TR["nslyr"]
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
    z2 = lambda v=0.0: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev) + v
    z3 = lambda v=0.0: torch.zeros((nb, ncat, nyb, nxb), dtype=torch.float64, device=dev) + v
    state_planes = (3 + ntrcr) * ncat
    out = {"what": "evpk_thermo_vertical (k_thermo_vertical<5, 4, 1>), state resident in HBM; the same call on pageable arrays", "grid": a.grid,
           "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "cells": nx * ny, "block_array_cells": cells, "physical_ocean_cells": int(lm.sum()),
           "state_GB": 8 * cells * state_planes / 1e9}

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
    nocean = int(po.sum().item())
    listed = (AN > C.puny) & po[:, None]
    nlisted = int(listed.sum().item())
    ncell_listed = int(listed.any(dim=1).sum().item())
    gb = 8 * (52 * nlisted + 15 * (cells * ncat - nlisted) + (nocean * ncat - nlisted) + 9 * nocean + 2 * ncell_listed) / 1e9
    Xn = X[:, None].expand(nb, ncat, nyb, nxb)
    Yn = Y[:, None].expand(nb, ncat, nyb, nxb)
    cat = torch.arange(ncat, dtype=torch.float64, device=dev)[None, :, None, None]
    forcing = {k: z2() for k in ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "sss")}
    forcing["shcoef"], forcing["lhcoef"] = z3(), z3()
    inout = {"fswsfcn": z3(), "fswintn": z3(), "Sswabsn": torch.zeros((nb, ncat, nslyr, nyb, nxb), dtype=torch.float64, device=dev),
             "Iswabsn": torch.zeros((nb, ncat, nilyr, nyb, nxb), dtype=torch.float64, device=dev), "fpond": z2(), "mlt_onset": z2(),
             "frz_onset": z2()}
    outp = {k: z3() for k in OUT15}
    state = dict(aicen=AN, vicen=VN, vsnon=SN, trcrn=TN)

    def workload(melting):
        """the vertical state and the forcing of one workload, written into the arrays above"""
        r = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * Xn + ph + cat) * torch.cos(q * Yn + 0.7 * cat)
        r2 = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * X + ph) * torch.cos(q * Y)
        forcing["rhoa"].fill_(1.3); forcing["Tbot"].fill_(-1.8); forcing["sss"].fill_(34.0)
        forcing["fsnow"].copy_(torch.where(r2(19, 23) > 0.5, 2.0e-5 * r2(7, 5), z2()))
        forcing["shcoef"].copy_(8.5 * (0.5 + r(13, 11)))
        forcing["lhcoef"].copy_(2.4e4 * (0.5 + r(17, 7, 1.0)))
        for k in ("Sswabsn", "Iswabsn", "fswsfcn", "fswintn"):
            inout[k].zero_()
        if melting:
            forcing["potT"].copy_(271.0 + 6.0 * r2(31, 37)); forcing["flw"].copy_(280.0 + 50.0 * r2(41, 29, 2.0))
            forcing["Qa"].copy_(3.0e-3 + 1.0e-3 * r2(11, 13)); forcing["fbot"].copy_(-5.0 - 35.0 * r2(9, 17))
            sw = 40.0 + 110.0 * r(23, 19)
            inout["fswsfcn"].copy_(0.5 * sw)
            inout["fswintn"].copy_(0.25 * sw)
            wl = [0.5 ** k for k in range(nilyr)]
            for k in range(nilyr):
                inout["Iswabsn"][:, :, k] = 0.25 * sw * wl[k] / sum(wl)
            Ttop = -0.5 - 2.5 * r(43, 47)
            hs = torch.where(r(53, 59) > 0.6, 0.02 + 0.1 * r(5, 3), z3())
        else:
            forcing["potT"].copy_(243.0 + 20.0 * r2(31, 37)); forcing["flw"].copy_(150.0 + 70.0 * r2(41, 29, 2.0))
            forcing["Qa"].copy_(3.0e-4 + 7.0e-4 * r2(11, 13)); forcing["fbot"].fill_(-2.0)
            Ttop = -5.0 - 15.0 * r(43, 47)
            hs = torch.where(r(53, 59) > 0.2, 0.05 + 0.2 * r(5, 3), z3())
        SN.copy_(AN * hs)
        Tsfc = torch.where(r(61, 67) > 0.5, z3(), Ttop - 0.3) if melting else Ttop - 1.0
        TN[:, :, TR["nt_Tsfc"] - 1] = Tsfc
        TN[:, :, TR["nt_qsno"] - 1] = -C.rhos * (C.Lfresh - C.cp_ice * torch.clamp(0.5 * (Tsfc + Ttop), max=0.0))
        for k in range(nilyr):
            S = 2.0 + 3.0 * r(3, 2, 0.3 * k) + 2.0 * (k + 0.5) / nilyr
            Tm = -S * DEPRESST
            T = torch.minimum(Ttop + (-1.9 - Ttop) * (k + 0.5) / nilyr, Tm - 0.05)
            TN[:, :, TR["nt_sice"] - 1 + k] = S
            TN[:, :, TR["nt_qice"] - 1 + k] = -C.rhoi * (C.cp_ice * (Tm - T) + C.Lfresh * (1.0 - Tm / T) - CP_OCN * Tm)

    def call():
        stop = ctx.thermo_vertical(dt, state, forcing, inout, outp, ntrcr, TR, yday=100.0, constants=K)
        assert stop is None, stop

    def sample(keep, rows, waves):
        """the restatement on rows x waves x 64 consecutive cells of block nb // 2; returns the iteration counts (rows, waves, ncat, 64) and
        whether the device result equals the restatement there"""
        b = nb // 2
        w = 64 * waves
        its_all, same = [], True
        blk = d.local_blocks[b]
        for r_ in range(rows):
            j = blk.jlo - 1 + int((r_ + 0.5) / rows * (blk.jhi - blk.jlo))
            lmj = lm[b, j]
            run = [i for i in range(nxb - w) if lmj[i:i + w].all()]
            if not run:
                continue
            i0 = run[len(run) // 2]
            cut = lambda q: np.ascontiguousarray(q[b:b + 1, ..., j:j + 1, i0:i0 + w].cpu().numpy())
            y = {k: cut(v) for k, v in list(keep.items()) + list(forcing.items())}
            y.update({k: np.zeros((1, ncat, 1, w)) for k in OUT15})
            x = dict(dt=dt, yday=100.0, min_salin=0.1, rhow=C.rhow, k=dict(K, rhoi=C.rhoi, rhos=C.rhos), tracers=TR)
            its = []
            infos, stop = nptherm1.step([(1, w, 1, 1)], np.ones((1, 1, w), dtype=np.int32), nptherm1.params(x), y, its)
            assert stop is None, stop
            cnt = np.zeros((waves, ncat, 64), dtype=np.int64)
            for _, n, _, i, it in its:
                cnt[i // 64, n, i % 64] = it
            its_all.append(cnt)
            for k, q in list(state.items()) + list(inout.items()) + list(outp.items()):
                if k != "fpond":
                    same = same and bool(np.array_equal(cut(q), y[k]))
        return np.array(its_all), same

    for name, melting in (("a_cold_winter_mix", False), ("b_melting_mix", True)):
        workload(melting)
        keep = {k: q.clone() for k, q in list(state.items()) + list(inout.items())}

        def restore():
            for k, q in list(state.items()) + list(inout.items()):
                q.copy_(keep[k])
        ms, first = timed(call, restore)
        its, same = sample(keep, a.sample_rows, a.sample_waves)
        done = its[its > 0]
        wmax = its.max(axis=-1) if its.size else its           # per (row, wave, category); 0: no listed cell in it
        hist = {str(int(v)): int(c) for v, c in zip(*np.unique(done, return_counts=True))}
        out[name] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": gb, "GBps_of_compulsory": gb / (ms * 1e-3),
                     "listed_cell_categories": nlisted, "sample_columns": int(done.size), "sample_equals_restatement": same,
                     "iterations_histogram": hist, "iterations_mean": float(done.mean()) if done.size else None,
                     "mean_of_per_wave_maximum": float(wmax[wmax > 0].mean()) if done.size else None,
                     "vanished": int(((state["aicen"] == 0.0) & listed).sum().item())}
    keep = None
    torch.cuda.empty_cache()

    if not a.no_pageable:
        # the same call on pageable arrays (melting mix) against the state round trip it replaces
        workload(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H = {k: q.cpu().numpy() for k, q in state.items()}
        down = time.perf_counter() - t0
        t0 = time.perf_counter()
        up = [torch.from_numpy(v).to(dev) for v in H.values()]
        torch.cuda.synchronize()
        up_s = time.perf_counter() - t0
        del up
        torch.cuda.empty_cache()
        Hf = {k: q.cpu().numpy() for k, q in forcing.items()}
        Hi = {k: q.cpu().numpy() for k, q in inout.items()}
        Ho = {k: q.cpu().numpy() for k, q in outp.items()}
        base = {k: v.copy() for k, v in list(H.items()) + list(Hi.items())}
        t1 = []
        for _ in range(3):                                  # the first round is the warm-up (it sizes the staging pool)
            for k, v in list(H.items()) + list(Hi.items()):
                v[...] = base[k]
            t0 = time.perf_counter()
            assert ctx.thermo_vertical(dt, H, Hf, Hi, Ho, ntrcr, TR, yday=100.0, constants=K) is None
            t1.append(time.perf_counter() - t0)
        out["pageable"] = {"thermo_vertical_one_call_ms": round(1e3 * min(t1[1:]), 1), "first_call_ms": round(1e3 * t1[0], 1),
                           "state_round_trip_down_and_up_ms": round(1e3 * (down + up_s), 1),
                           "staged_up_GB": 8 * cells * (state_planes + (2 + 2 + nslyr + nilyr) * ncat + 10) / 1e9,
                           "staged_down_GB": 8 * cells * (state_planes + (2 + nslyr + nilyr + 15) * ncat + 3) / 1e9}
    del AN, VN, SN, TN, state
    torch.cuda.empty_cache()

    # the yardstick: cleanup_itd where every block shifts (scripts/itd_bench.py, case b), same session, same box
    AN, VN, SN, TN = stacked(True)
    keep = [q.clone() for q in (AN, VN, SN, TN)]
    fl = {k: z2() for k in ("fpond", "fresh", "fsalt", "fhocn")}
    a0, a1 = z2(), z2()

    def restore():
        for q, k in zip((AN, VN, SN, TN), keep):
            q.copy_(k)

    def call():
        assert ctx.cleanup_itd(dt, AN, VN, SN, TN, a0, a1, ntrcr, DEP, TR, HIN_MAX[:ncat + 1], None, fl, None) is None
    ms, first = timed(call, restore)
    nl = int(lm.sum())
    cgb = 8 * nl * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9 + 2 * 8 * nl * state_planes / 1e9
    out["cleanup_itd_b_every_block_shifts"] = {"ms_per_call": round(ms, 3), "first_call_ms": round(first, 1), "compulsory_GB": cgb,
                                               "GBps_of_compulsory": cgb / (ms * 1e-3)}
    for name in ("a_cold_winter_mix", "b_melting_mix"):
        out[name]["GBps_ratio_to_cleanup_itd_b"] = out[name]["GBps_of_compulsory"] / out["cleanup_itd_b_every_block_shifts"]["GBps_of_compulsory"]
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
