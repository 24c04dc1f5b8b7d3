#!/usr/bin/env python3
"""Time evpk_step_radiation_dedd (k_shortwave_dedd<5, 4, 1>: step_radiation on its Delta-Eddington branch and the albedo lines of
coupling_prep, one launch) on one MI355X with the ice state and every output resident in HBM, on the thickness distribution of
scripts/itd_bench.py (12 tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl, and apnd, hpnd behind them for tr_pond_cesm) in three cases:
  a_polar_night    no shortwave anywhere: the call writes its zeros and the 2-D sums, no column is solved
  b_winter_mix     snow of 5 .. 25 cm on every category (fs = 1: one surface type), no ponds, a low sun, Tsfc of -6 .. -21 C
  c_melting_mix    snow of 5 .. 25 mm (fs < 1), ponds of 10 .. 40 % and 5 .. 40 cm on every category, Tsfc at 0 C on half of them: all three
                   surface types on every listed column
Unlike the CCSM3 scheme the cost is arithmetic, not bytes: ten exp per layer that the trmin cut-off lets through.  Each case reports
  ms per call            minimum, median and maximum over `--reps` timed calls behind one warm-up call
  exp per second         the restatement's counter (tests/npdedd.py, info["exp_calls"]: ten per layer solved) on every `--stride`-th cell in
                         x and y of the same input, scaled by the number of listed lit columns; beside it the bound without the cut-off,
                         10 (nslyr + nilyr + 2) x 3 bands x the surface types present, counted on the whole input
  evpk_step_radiation    the CCSM3 scheme on the same state and shortwave, timed in the same run
  pageable               the same call on pageable numpy arrays
Prints one JSON line per case.

    python scripts/dedd_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--no-pageable]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=24, help="the restatement counts exp on every stride-th cell in x and y")
    ap.add_argument("--no-pageable", action="store_true", help="skip the calls on pageable arrays")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    from tests import npdedd
    nx, ny = (int(v) for v in a.grid.split("x"))
    TR = dict(ib.TR, nt_sice=7, nt_vlvl=12)
    ntr0, ncat = len(ib.DEP), a.ncat
    TRP = dict(TR, tr_pond_cesm=1, nt_apnd=ntr0 + 1, nt_hpnd=ntr0 + 2)
    ntrcr = ntr0 + 2
    nilyr, nslyr = TR["nilyr"], TR["nslyr"]
    dt = 3600.0
    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES[a.ns], land="continents")
    d = blocks.create_distrb_cart(nx, ny, nx // a.xblocks, ny, ns_boundary_type=a.ns)
    f = synth.make_block_fields(case, d)
    s = dyn.EvpDynamics(d, f, ndte=120, xmin=synth.global_min_dx(case))
    s.set_evp_parameters(dt)
    ctx = s.ctx
    rhos = C.rhos                                          # (what set_evp_parameters hands the library)
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
    z2 = lambda v=0.0: torch.zeros((nb, nyb, nxb), dtype=torch.float64, device=dev) + v
    z3 = lambda v=0.0: torch.zeros((nb, ncat, nyb, nxb), dtype=torch.float64, device=dev) + v
    zl = lambda nl: torch.zeros((nb, ncat, nl, nyb, nxb), dtype=torch.float64, device=dev)

    def timed(fn):
        times = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        t = sorted(times[1:])
        return {"ms_min": round(t[0], 3), "ms_median": round(t[len(t) // 2], 3), "ms_max": round(t[-1], 3), "first_call_ms": round(times[0], 1)}

    an, vn, sn, t = ib.state(torch, X, Y, ocean, ncat, ntr0, False, C)
    AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
    TN = torch.cat([torch.stack([torch.stack(q, dim=1) for q in t], dim=1), zl(2)], dim=2).contiguous()       # (nb, ncat, ntrcr, ny, nx)
    del an, vn, sn, t
    state = dict(aicen=AN, vicen=VN, vsnon=SN, trcrn=TN)
    listed = (AN > C.puny) & po[:, None]
    nlisted = int(listed.sum().item())
    Xn = X[:, None].expand(nb, ncat, nyb, nxb)
    Yn = Y[:, None].expand(nb, ncat, nyb, nxb)
    cat = torch.arange(ncat, dtype=torch.float64, device=dev)[None, :, None, None]
    r2 = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * X + ph) * torch.cos(q * Y)
    r = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * Xn + ph + cat) * torch.cos(q * Yn + 0.7 * cat)
    forcing = {k: z2() for k in evpk.DEDD_FORCING}
    coszen, coszen0 = z2(), z2()
    outp = {k: z3() for k in evpk.DEDD_OUT}
    outp.update(Sswabsn=zl(nslyr), Iswabsn=zl(nilyr), fswpenln=zl(nilyr + 1))
    outp.update({k: z2() for k in evpk.DEDD_OUT2D})
    ccsm3_forcing = dict(forcing, ocn_albedo2D=z2(0.06))
    ccsm3_out = dict(outp, coszen=z2())

    def workload(name):
        TN[:, :, ntr0:] = 0.0
        if name == "c_melting_mix":
            Ttop = -0.5 - 2.5 * r(43, 47)
            TN[:, :, TR["nt_Tsfc"] - 1] = torch.where(r(61, 67) > 0.5, z3(), Ttop)
            SN.copy_(AN * (0.005 + 0.02 * r(5, 3)))
            TN[:, :, ntr0] = 0.1 + 0.3 * r(13, 17)
            TN[:, :, ntr0 + 1] = 0.05 + 0.35 * r(29, 31)
            sw = 40.0 + 110.0 * r2(23, 19)
            coszen0.copy_(torch.where(ocean, 0.2 + 0.7 * r2(3, 2), z2()))
        else:
            TN[:, :, TR["nt_Tsfc"] - 1] = -6.0 - 15.0 * r(43, 47)
            SN.copy_(AN * (0.05 + 0.2 * r(5, 3)))
            sw = 5.0 + 30.0 * r2(23, 19) if name == "b_winter_mix" else z2()
            coszen0.copy_(torch.where(ocean, 0.05 + 0.25 * r2(3, 2), z2()) if name == "b_winter_mix" else z2())
        for k, w in (("swvdr", 0.28), ("swvdf", 0.24), ("swidr", 0.31), ("swidf", 0.17)):
            forcing[k].copy_(w * sw)

    def dedd(st=state, fo=forcing, cz=None, ou=outp):
        if cz is None:
            coszen.copy_(coszen0)
            cz = coszen
        ctx.step_radiation_dedd(st, fo, cz, ou, ntrcr, TRP)

    def ccsm3():
        ctx.step_radiation(state, ccsm3_forcing, ccsm3_out, ntrcr, TR)

    def exp_counts():
        """(bound without the trmin cut-off on the whole input, the restatement's count on the sample scaled to the whole input)"""
        hs = SN / torch.where(AN > 0.0, AN, z3(1.0))
        fs = torch.where(hs >= 1.0e-4, torch.clamp(hs / 0.03, max=1.0), z3())
        fp = torch.where(hs >= 1.0e-4, (1.0 - torch.clamp(hs / 0.03, max=1.0)) * TN[:, :, ntr0], TN[:, :, ntr0])
        lit = listed & ((forcing["swvdr"] + forcing["swidr"] + forcing["swvdf"] + forcing["swidf"]) > C.puny)[:, None]
        types = ((1.0 - fs - fp > 0.0).to(torch.int64) + (fs > 0.0).to(torch.int64) + (fp > C.puny).to(torch.int64)) * lit
        bound = 10 * (nslyr + nilyr + 2) * 3 * int(types.sum().item())
        nlit = int(lit.sum().item())
        if nlit == 0:
            return bound, 0, 0
        st = a.stride
        cut = lambda q: np.ascontiguousarray(np.moveaxis(q[..., ::st, ::st].cpu().numpy(), 0, -2).reshape(q.shape[1:-2] + (-1, q[..., ::st, ::st].shape[-1]))[None])
        y = {k: cut(v) for k, v in state.items()}
        y.update({k: cut(v) for k, v in forcing.items()})
        y["coszen"] = cut(coszen0)
        y.update({k: np.zeros_like(cut(v)) for k, v in outp.items()})
        tm = cut(po.to(torch.float64)) > 0.0
        p = dict(evpk.DEDD_DEFAULTS, tr=TRP, rhos=rhos)
        infos = npdedd.step_radiation_dedd([(1, tm.shape[2], 1, tm.shape[1])], tm, p, y)
        sample_lit = sum(i["lit"] for i in infos)
        counted = npdedd.exp_count(infos)
        return bound, int(round(counted * nlit / max(sample_lit, 1))), sample_lit

    for name in ("a_polar_night", "b_winter_mix", "c_melting_mix"):
        workload(name)
        row = {"case": name, "what": "evpk_step_radiation_dedd (k_shortwave_dedd<5, 4, 1>), state and outputs resident in HBM", "grid": a.grid,
               "ncat": ncat, "layers": [nilyr, nslyr], "block_array_cells": nb * nyb * nxb, "listed_cell_categories": nlisted, "reps": a.reps}
        row["step_radiation_dedd"] = timed(dedd)
        bound, counted, sample = exp_counts()
        sec = row["step_radiation_dedd"]["ms_min"] * 1e-3
        row.update(exp_bound_without_cutoff=bound, exp_counted_by_restatement=counted, restatement_sample_lit_columns=sample,
                   exp_per_second=counted / sec, exp_per_second_of_bound=bound / sec)
        row["step_radiation_ccsm3"] = timed(ccsm3)
        if not a.no_pageable:
            torch.cuda.synchronize()
            H, Hf, Ho = ({k: q.cpu().numpy() for k, q in src.items()} for src in (state, forcing, outp))
            t1 = []
            for _ in range(3):                                  # the first round is the warm-up (it sizes the staging pool)
                cz = coszen0.cpu().numpy()
                t0 = time.perf_counter()
                dedd(H, Hf, cz, Ho)
                t1.append(time.perf_counter() - t0)
            row["pageable_ms"] = round(1e3 * min(t1[1:]), 1)
            del H, Hf, Ho
        print(json.dumps(row), flush=True)
    s.close()


if __name__ == "__main__":
    main()
