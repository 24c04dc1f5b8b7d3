#!/usr/bin/env python3
"""Time evpk_step_radiation (k_shortwave_ccsm3: step_radiation on its ccsm3 branch and the albedo lines of coupling_prep, one launch) and
evpk_prep_radiation (k_prep_radiation) on one MI355X with the ice state and every output resident in HBM, on the thickness distribution
of scripts/itd_bench.py (12 tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl) under two mixes:
  a_cold_winter_mix   Tsfc of -6 .. -21 C, snow on four categories in five, shortwave on a third of the cells (the low sun)
  b_melting_mix       Tsfc at 0 C on half the categories and -0.5 .. -3 C on the others, snow on two in five, shortwave everywhere
In the same run the yardstick, evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py, so that the fraction of its rate on
the compulsory bytes comes from one session.  Every figure is the minimum, the median and the maximum over `--reps` timed calls behind one
warm-up call: the spread of this script within one session.
Then the same call on PAGEABLE numpy arrays against the transfer it replaces: aicen, vicen, vsnon and Tsfcn down to the host and the 40
planes evpk_step_therm1 reads (fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn at 5 x (4 + 1)) up again, as plain copies.

    python scripts/rad_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--no-pageable]

Compulsory bytes, fp64, each array element once:
  k_shortwave_ccsm3   a (cell, category) of the block arrays: aicen read; the nine per-category planes, nslyr + nilyr layers and the
                      nilyr + 1 planes of fswpenln written                                                     1 + 9 + nslyr + 2 nilyr + 1
                      a listed one besides: vicen, vsnon, Tsfc read                                                                  3
                      a cell of the block arrays: the four sw* and ocn_albedo2D read, eight planes written                           13
  k_prep_radiation    a physical cell: aice, four sw*, four al*_ai, scale_factor read; scale_factor, fswfac written                  12
                      a (cell, category) of a physical ocean cell: aicen read                                                        1
                      a listed one besides: 3 + nslyr + 2 nilyr + 1 planes read and written                       2 (4 + nslyr + 2 nilyr)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="3600x2700")
    ap.add_argument("--ns", default="tripole")
    ap.add_argument("--xblocks", type=int, default=8)
    ap.add_argument("--ncat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--no-pageable", action="store_true", help="skip the calls on pageable arrays")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    nx, ny = (int(v) for v in a.grid.split("x"))
    DEP, HIN_MAX = ib.DEP, ib.HIN_MAX
    TR = dict(ib.TR, nt_sice=7, nt_vlvl=12)
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
    ph = np.zeros(f["tmask"].shape, dtype=bool)
    for n, b in enumerate(d.local_blocks):
        lm[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = f["tmask"][n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] > 0
        ph[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    po = torch.from_numpy(lm).to(dev)
    cells = nb * nyb * nxb
    z2 = lambda v=0.0: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev) + v
    z3 = lambda v=0.0: torch.zeros((nb, ncat, nyb, nxb), dtype=torch.float64, device=dev) + v
    zl = lambda nl: torch.zeros((nb, ncat, nl, nyb, nxb), dtype=torch.float64, device=dev)
    out = {"what": "evpk_step_radiation (k_shortwave_ccsm3<5, 4, 1>) and evpk_prep_radiation (k_prep_radiation<5, 4, 1>), state and outputs "
                   "resident in HBM; the same on pageable arrays", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "cells": nx * ny,
           "block_array_cells": cells, "physical_ocean_cells": int(lm.sum()), "reps": a.reps}

    def timed(fn, restore=lambda: None):
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
    state = dict(aicen=AN, vicen=VN, vsnon=SN, trcrn=TN)
    listed = (AN > C.puny) & po[:, None]
    nlisted, nocean, nphys = int(listed.sum().item()), int(lm.sum()), int(ph.sum())
    Xn = X[:, None].expand(nb, ncat, nyb, nxb)
    Yn = Y[:, None].expand(nb, ncat, nyb, nxb)
    cat = torch.arange(ncat, dtype=torch.float64, device=dev)[None, :, None, None]
    r2 = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * X + ph) * torch.cos(q * Y)
    r = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * Xn + ph + cat) * torch.cos(q * Yn + 0.7 * cat)
    forcing = {k: z2() for k in evpk.RAD_FORCING}
    forcing["ocn_albedo2D"].copy_(0.069 - 0.011 * torch.cos(2.0 * (Y - 0.5 * np.pi)))
    outp = {k: z3() for k in evpk.RAD_OUT}
    outp.update(Sswabsn=zl(nslyr), Iswabsn=zl(nilyr), fswpenln=zl(nilyr + 1))
    outp.update({k: z2() for k in evpk.RAD_OUT2D})
    fswfac = z2()
    per = 1 + 9 + nslyr + 2 * nilyr + 1
    gb_rad = 8 * (per * cells * ncat + 3 * nlisted + 13 * cells) / 1e9
    gb_prep = 8 * (12 * nphys + nocean * ncat + 2 * (4 + nslyr + 2 * nilyr) * nlisted) / 1e9
    out.update(listed_cell_categories=nlisted, compulsory_GB_k_shortwave_ccsm3=gb_rad, compulsory_GB_k_prep_radiation=gb_prep)

    def workload(melting):
        if melting:
            Ttop = -0.5 - 2.5 * r(43, 47)
            TN[:, :, TR["nt_Tsfc"] - 1] = torch.where(r(61, 67) > 0.5, z3(), Ttop)
            SN.copy_(AN * torch.where(r(53, 59) > 0.6, 0.02 + 0.1 * r(5, 3), z3()))
            sw = 40.0 + 110.0 * r2(23, 19)
        else:
            TN[:, :, TR["nt_Tsfc"] - 1] = -6.0 - 15.0 * r(43, 47)
            SN.copy_(AN * torch.where(r(53, 59) > 0.2, 0.05 + 0.2 * r(5, 3), z3()))
            sw = torch.where(r2(7, 11) > 0.67, 5.0 + 30.0 * r2(23, 19), z2())
        for k, w in (("swvdr", 0.28), ("swvdf", 0.24), ("swidr", 0.31), ("swidf", 0.17)):
            forcing[k].copy_(w * sw)

    def rad(st=state, fo=forcing, ou=outp):
        ctx.step_radiation(st, fo, ou, ntrcr, TR)

    def prep_args(ou, fo, aice, aicen, fac):
        z = {k: ou[k] for k in evpk.PREP_RAD_INOUT}
        z.update({k: fo[k] for k in ("swvdr", "swvdf", "swidr", "swidf")})
        z.update(aice=aice, aicen=aicen, fswfac=fac, alvdr_ai=ou["alvdr"], alvdf_ai=ou["alvdf"], alidr_ai=ou["alidr"], alidf_ai=ou["alidf"])
        return z

    aice = AN.sum(dim=1).contiguous()
    for name, melting in (("a_cold_winter_mix", False), ("b_melting_mix", True)):
        workload(melting)
        row = {"step_radiation": timed(rad)}
        row["step_radiation"].update(GBps_of_compulsory=gb_rad / (row["step_radiation"]["ms_min"] * 1e-3))
        z = prep_args(outp, forcing, aice, AN, fswfac)
        row["prep_radiation"] = timed(lambda: ctx.prep_radiation(z, nilyr, nslyr), rad)     # (each timed call behind a fresh step_radiation)
        row["prep_radiation"].update(GBps_of_compulsory=gb_prep / (row["prep_radiation"]["ms_min"] * 1e-3))
        out[name] = row

    if not a.no_pageable:
        workload(True)
        torch.cuda.synchronize()
        H, Hf, Ho = ({k: q.cpu().numpy() for k, q in src.items()} for src in (state, forcing, outp))
        t1 = []
        for _ in range(3):                                  # the first round is the warm-up (it sizes the staging pool)
            t0 = time.perf_counter()
            rad(H, Hf, Ho)
            t1.append(time.perf_counter() - t0)
        # the transfer the call replaces: aicen, vicen, vsnon, Tsfcn down, the 40 planes step_therm1 reads up -- plain copies, pageable
        down = [AN, VN, SN, TN[:, :, TR["nt_Tsfc"] - 1].contiguous()]
        up = [outp[k] for k in ("fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn")]
        hd = [torch.from_numpy(np.empty(tuple(q.shape))) for q in down]
        hu = [torch.from_numpy(Ho[k]) for k in ("fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn")]
        t2 = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for h, q in zip(hd, down):
                h.copy_(q)
            for h, q in zip(hu, up):
                q.copy_(h)
            torch.cuda.synchronize()
            t2.append(time.perf_counter() - t0)
        planes = sum(int(np.prod(q.shape[1:-2])) for q in down), sum(int(np.prod(q.shape[1:-2])) for q in up)
        out["pageable"] = {"step_radiation_ms": round(1e3 * min(t1[1:]), 1), "transfer_it_replaces_ms": round(1e3 * min(t2[1:]), 1),
                           "transfer_planes_down_up": planes,
                           "not_counted_for_the_transfer": "shortwave_ccsm3 and the albedo aggregation on the host"}
        del H, Hf, Ho, hd, hu, down, up
    del AN, VN, SN, TN, state, outp
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
    row = timed(call, restore)
    state_planes = (3 + ntrcr) * ncat
    cgb = 8 * nocean * (3 * ncat + ncat * TR["nslyr"] + 1 + 2) / 1e9 + 2 * 8 * nocean * state_planes / 1e9
    row.update(compulsory_GB=cgb, GBps_of_compulsory=cgb / (row["ms_min"] * 1e-3))
    out["cleanup_itd_b_every_block_shifts"] = row
    for name in ("a_cold_winter_mix", "b_melting_mix"):
        for k in ("step_radiation", "prep_radiation"):
            out[name][k]["GBps_ratio_to_cleanup_itd_b"] = out[name][k]["GBps_of_compulsory"] / row["GBps_of_compulsory"]
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
