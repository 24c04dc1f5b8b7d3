#!/usr/bin/env python3
"""Time evpk_step_therm1 (k_therm1_open, k_thermo_vertical, k_therm1_merge: step_therm1 in one call) on one MI355X with the ice state
resident in HBM, on the state and the two forcings of scripts/therm1_bench.py (a cold winter mix, a melting mix; 12 tracers: Tsfc, 4 x qice,
qsno, 4 x sice, alvl, vlvl -- neither iage nor FY nor ponds), with the further forcing of step_therm1: frzmlt < 0 on about half the
ocean, sst up to 2 K above Tf, an ice-ocean stress of 1e-4 .. 0.1 N m-2, wind of 0.5 .. 15 m/s, zlvl = 10 m.
In the same run: evpk_thermo_vertical alone (the parent's routine) on the coefficients the one call produced, and the yardstick,
evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py.  Every figure is the minimum, the median and the maximum over
`--reps` timed calls behind one warm-up call: the spread of this script within one session.
The two new launches are not timed from the host: `--only one` / `--only alone` restrict the run to the one call / to
evpk_thermo_vertical alone, so that a `rocprofv3 --kernel-trace --stats` run of either gives the kernels' own times, k_thermo_vertical's
inside the one call and alone among them; `--kernel-ms open,vertical,merge` then adds the GB/s rows from those times.
Then the one call on PAGEABLE numpy arrays against what a host does today around evpk_thermo_vertical on pageable arrays (the fifteen
per-category planes down for merge_fluxes, shcoef and lhcoef up).

    python scripts/therm1s_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--no-pageable] [--only one|alone]

Compulsory bytes, fp64, each array element once:
  k_therm1_open    a listed (cell, category): aicen, vicen, Tsfc read; aicen_init, vicen_init and the eight planes written        13
                   any other (cell, category): aicen, vicen read; aicen_init, vicen_init and eight zeros written                  12
                   a cell of the block arrays: aice, Tf, frzmlt read; aice_init, rside, Tbot, fbot written                         7
                   a physical ocean cell: potT, Qa, rhoa, uatm, vatm, wind, zlvl read                                              7
                   a melting cell (aice > puny, frzmlt < 0): sst, strocnxT, strocnyT, and per category vsnon, qsno, 4 x qice    3 + 6 ncat
                   a cell with a listed category: Cdn_atm written                                                                  1
  k_therm1_merge   a listed (cell, category): aicen, aicen_init, fswthrun, fswsfcn, fswintn, six planes of the opener, fourteen
                   of k_thermo_vertical read                                                                                      25
                   any other (cell, category) of a physical ocean cell: aicen, aicen_init read                                     2
                   a cell with a listed category: flw read, the 22 cumulative planes read and written                             45
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--only", choices=["all", "one", "alone"], default="all")
    ap.add_argument("--no-pageable", action="store_true", help="skip the calls on pageable arrays")
    ap.add_argument("--kernel-ms", default="", help="open,vertical,merge: kernel times of the melting mix from a kernel trace of `--only one`")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
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
    out = {"what": "evpk_step_therm1 (k_therm1_open, k_thermo_vertical<5, 4, 1>, k_therm1_merge), state resident in HBM; evpk_thermo_vertical "
                   "alone; the same on pageable arrays", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "cells": nx * ny,
           "block_array_cells": cells, "physical_ocean_cells": int(lm.sum()), "reps": a.reps, "only": a.only}

    def timed(fn, restore):
        times = []
        for _ in range(a.reps + 1):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        t = sorted(times[1:])
        return {"ms_min": round(t[0], 3), "ms_median": round(t[len(t) // 2], 3), "ms_max": round(t[-1], 3), "first_call_ms": round(times[0], 1)}

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
    Xn = X[:, None].expand(nb, ncat, nyb, nxb)
    Yn = Y[:, None].expand(nb, ncat, nyb, nxb)
    cat = torch.arange(ncat, dtype=torch.float64, device=dev)[None, :, None, None]
    r2 = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * X + ph) * torch.cos(q * Y)
    forcing = {k: z2() for k in ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "sss", "aice", "frzmlt", "sst", "Tf", "strocnxT", "strocnyT",
                                 "uatm", "vatm", "wind", "zlvl")}
    forcing["shcoef"], forcing["lhcoef"], forcing["fswthrun"] = z3(), z3(), z3()
    inout = {"fswsfcn": z3(), "fswintn": z3(), "Sswabsn": torch.zeros((nb, ncat, nslyr, nyb, nxb), dtype=torch.float64, device=dev),
             "Iswabsn": torch.zeros((nb, ncat, nilyr, nyb, nxb), dtype=torch.float64, device=dev), "fpond": z2(), "mlt_onset": z2(),
             "frz_onset": z2()}
    outp = {k: z3() for k in evpk.THERMO_OUT + ["aicen_init", "vicen_init"]}
    outp.update({k: z2() for k in ("rside", "aice_init")})
    merged = {k: z2() for k in ["Cdn_atm"] + evpk.THERM1_MERGED}
    state = dict(aicen=AN, vicen=VN, vsnon=SN, trcrn=TN)
    # the further forcing of step_therm1
    forcing["aice"].copy_(AN.sum(dim=1))
    forcing["Tf"].fill_(-1.8)
    forcing["frzmlt"].copy_(torch.where(r2(3, 5, 0.4) > 0.5, -20.0 - 200.0 * r2(7, 3), 30.0 * r2(5, 7)))
    forcing["sst"].copy_(-1.8 + 2.0 * r2(11, 9, 1.3))
    tau = 10.0 ** (-4.0 + 3.0 * r2(13, 17))
    forcing["strocnxT"].copy_(tau * torch.cos(9 * X)); forcing["strocnyT"].copy_(tau * torch.sin(9 * X))
    forcing["wind"].copy_(0.5 + 14.5 * r2(15, 21, 0.9))
    forcing["uatm"].copy_(forcing["wind"] * torch.cos(5 * Y)); forcing["vatm"].copy_(forcing["wind"] * torch.sin(5 * Y))
    forcing["zlvl"].fill_(10.0)
    melting_cells = int((po & (forcing["aice"] > C.puny) & (forcing["frzmlt"] < 0.0)).sum().item())
    gb_open = 8 * (13 * nlisted + 12 * (cells * ncat - nlisted) + 7 * cells + 7 * nocean + (3 + (2 + nilyr) * ncat) * melting_cells + ncell_listed) / 1e9
    gb_merge = 8 * (25 * nlisted + 2 * (nocean * ncat - nlisted) + 45 * ncell_listed) / 1e9
    out.update(listed_cell_categories=nlisted, melting_cells=melting_cells, compulsory_GB_k_therm1_open=gb_open, compulsory_GB_k_therm1_merge=gb_merge)

    def workload(melting):
        """the vertical state and the forcing of one workload of scripts/therm1_bench.py, written into the arrays above"""
        r = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * Xn + ph + cat) * torch.cos(q * Yn + 0.7 * cat)
        forcing["rhoa"].fill_(1.3); forcing["sss"].fill_(34.0)
        forcing["fsnow"].copy_(torch.where(r2(19, 23) > 0.5, 2.0e-5 * r2(7, 5), z2()))
        for k in ("Sswabsn", "Iswabsn", "fswsfcn", "fswintn"):
            inout[k].zero_()
        forcing["fswthrun"].zero_()
        if melting:
            forcing["potT"].copy_(271.0 + 6.0 * r2(31, 37)); forcing["flw"].copy_(280.0 + 50.0 * r2(41, 29, 2.0))
            forcing["Qa"].copy_(3.0e-3 + 1.0e-3 * r2(11, 13))
            sw = 40.0 + 110.0 * r(23, 19)
            inout["fswsfcn"].copy_(0.5 * sw)
            inout["fswintn"].copy_(0.25 * sw)
            forcing["fswthrun"].copy_(0.05 * sw)
            wl = [0.5 ** k for k in range(nilyr)]
            for k in range(nilyr):
                inout["Iswabsn"][:, :, k] = 0.25 * sw * wl[k] / sum(wl)
            Ttop = -0.5 - 2.5 * r(43, 47)
            hs = torch.where(r(53, 59) > 0.6, 0.02 + 0.1 * r(5, 3), z3())
        else:
            forcing["potT"].copy_(243.0 + 20.0 * r2(31, 37)); forcing["flw"].copy_(150.0 + 70.0 * r2(41, 29, 2.0))
            forcing["Qa"].copy_(3.0e-4 + 7.0e-4 * r2(11, 13))
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

    def one(st=state, fo=forcing, io=inout, ou=outp, me=merged):
        stop = ctx.step_therm1(dt, st, fo, io, ou, me, ntrcr, TR, yday=100.0, constants=K, ustar_min=0.005)
        assert stop is None, stop

    def alone(st=state, fo=forcing, io=inout, ou=outp):
        stop = ctx.thermo_vertical(dt, st, fo, io, ou, ntrcr, TR, yday=100.0, constants=K)
        assert stop is None, stop

    for name, melting in (("a_cold_winter_mix", False), ("b_melting_mix", True)):
        workload(melting)
        keep = {k: q.clone() for k, q in list(state.items()) + list(inout.items())}

        def restore():
            for k, q in list(state.items()) + list(inout.items()):
                q.copy_(keep[k])
        row = {}
        if a.only in ("all", "one"):
            row["step_therm1_one_call"] = timed(one, restore)      # (it leaves shcoef, lhcoef, fbot, Tbot in `forcing` for the call alone)
        else:
            restore(); one()
        if a.only in ("all", "alone"):
            row["thermo_vertical_alone"] = timed(alone, restore)
        if a.only == "all":
            row["one_call_minus_alone_ms_median"] = round(row["step_therm1_one_call"]["ms_median"] - row["thermo_vertical_alone"]["ms_median"], 3)
        out[name] = row
    keep = None
    torch.cuda.empty_cache()

    if not a.no_pageable and a.only == "all":
        workload(True)
        torch.cuda.synchronize()
        H, Hf, Hi, Ho, Hm = ({k: q.cpu().numpy() for k, q in src.items()} for src in (state, forcing, inout, outp, merged))
        base = {k: v.copy() for k, v in list(H.items()) + list(Hi.items())}
        t1, t2 = [], []
        for _ in range(3):                                  # the first round is the warm-up (it sizes the staging pool)
            for fn, ts in ((one, t1), (alone, t2)):
                for k, v in list(H.items()) + list(Hi.items()):
                    v[...] = base[k]
                t0 = time.perf_counter()
                fn(H, Hf, Hi, Ho, Hm) if fn is one else fn(H, Hf, Hi, Ho)
                ts.append(time.perf_counter() - t0)
        out["pageable"] = {"step_therm1_one_call_ms": round(1e3 * min(t1[1:]), 1), "thermo_vertical_as_today_ms": round(1e3 * min(t2[1:]), 1),
                           "as_today_moves": "the fifteen per-category planes down, shcoef and lhcoef up, beside the state both calls move",
                           "not_counted_for_today": "merge_fluxes, frzmlt_bottom_lateral and atmo_boundary_layer on the host"}
        del H, Hf, Hi, Ho, Hm, base
    del AN, VN, SN, TN, state
    torch.cuda.empty_cache()

    if a.only == "all":
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
        row = timed(call, restore)
        nl = int(lm.sum())
        cgb = 8 * nl * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9 + 2 * 8 * nl * state_planes / 1e9
        row.update(compulsory_GB=cgb, GBps_of_compulsory=cgb / (row["ms_min"] * 1e-3))
        out["cleanup_itd_b_every_block_shifts"] = row
        if a.kernel_ms:
            ko, kv, km = (float(v) for v in a.kernel_ms.split(","))
            y = row["GBps_of_compulsory"]
            out["kernels_b_melting_mix_from_trace"] = {
                "k_therm1_open_ms": ko, "k_therm1_open_GBps": gb_open / (ko * 1e-3), "k_therm1_open_GBps_ratio_to_cleanup_itd_b": gb_open / (ko * 1e-3) / y,
                "k_thermo_vertical_ms": kv,
                "k_therm1_merge_ms": km, "k_therm1_merge_GBps": gb_merge / (km * 1e-3), "k_therm1_merge_GBps_ratio_to_cleanup_itd_b": gb_merge / (km * 1e-3) / y}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
