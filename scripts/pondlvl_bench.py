#!/usr/bin/env python3
"""Time the two level-ice pond calls, evpk_step_therm1_lvl (k_therm1_open, k_thermo_vertical<5, 4, 1>, k_therm1_merge<5, 1>) and
evpk_step_radiation_dedd_lvl (k_shortwave_dedd<5, 4, 1, 1>), on one MI355X with the ice state and every output resident in HBM, beside
their tr_pond_cesm parents in the same run: the melting mixes of scripts/therm1s_bench.py and scripts/dedd_bench.py on the thickness
distribution of scripts/itd_bench.py (12 tracers: Tsfc, 4 x qice, qsno, 4 x sice, alvl, vlvl) with apnd, hpnd and ipnd behind them --
ponds of 10 .. 40 % of the level ice and 5 .. 40 cm on every category, a refrozen lid of up to 2 cm on half of them, frzpnd = 'hlid',
dpscale = 1e-3, hs1 = 0.03.  Every figure is the minimum, the median and the maximum over `--reps` timed calls behind one warm-up call:
the spread of this script within one session.
`--only lvl` / `--only cesm` restrict the run to the new calls / to the parents, so that a `rocprofv3 --kernel-trace --stats` run of
either gives the kernels' own times; `--kernel-ms MERGE_LVL` then adds the GB/s row of k_therm1_merge<5, 1> from that time, beside
evpk_cleanup_itd's case b_every_block_shifts of scripts/itd_bench.py, timed here.

    python scripts/pondlvl_bench.py --grid 3600x2700 --ns tripole --ncat 5 [--only lvl|cesm] [--kernel-ms 1.9]

Compulsory bytes of k_therm1_merge<5, 1>, fp64, each array element once (scripts/therm1s_bench.py has the parent's):
  a listed (cell, category): the parent's 25; vicen, vsnon, alvl, apnd, hpnd, ipnd, dhsn read; apnd, hpnd, ipnd written     35
  any other (cell, category) of a physical ocean cell: aicen, aicen_init, alvl read                                            3
  every (cell, category) of the block arrays: ffracn written                                                                   1
  a cell with a listed category: flw, frain, Tair read, the 22 cumulative planes read and written                             47
  a listed (cell, category) that holds a pond on return: nilyr enthalpy and nilyr salinity planes read                    2 nilyr
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
    ap.add_argument("--only", choices=["all", "lvl", "cesm"], default="all")
    ap.add_argument("--kernel-ms", default="", help="the time of k_therm1_merge<5, 1> from a kernel trace of `--only lvl`")
    a = ap.parse_args()
    import torch
    from cice5_amd import blocks, constants as C, dyn, evpk, synth
    nx, ny = (int(v) for v in a.grid.split("x"))
    ntr0, ncat = len(ib.DEP), a.ncat
    TR = dict(ib.TR, nt_sice=7, nt_vlvl=12, nt_apnd=ntr0 + 1, nt_hpnd=ntr0 + 2, nt_ipnd=ntr0 + 3)
    TRL, TRC = dict(TR, tr_pond_lvl=1), dict(TR, tr_pond_cesm=1)
    K = dict(Tocnfrz=C.Tocnfrz, ice_ref_salinity=C.ice_ref_salinity, hs_min=C.hs_min, cp_ice=C.cp_ice, Lfresh=C.Lfresh, Tmin=C.Tmin, puny=C.puny)
    ntrcr = ntr0 + 3
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
    zl = lambda nl: torch.zeros((nb, ncat, nl, nyb, nxb), dtype=torch.float64, device=dev)
    out = {"what": "evpk_step_therm1_lvl and evpk_step_radiation_dedd_lvl beside evpk_step_therm1 and evpk_step_radiation_dedd under tr_pond_cesm, "
                   "state and outputs resident in HBM", "grid": a.grid, "ns": a.ns, "ncat": ncat, "ntrcr": ntrcr, "layers": [nilyr, nslyr],
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

    def stacked(shifting, extra):
        an, vn, sn, t = ib.state(torch, X, Y, ocean, ncat, ntr0, shifting, C)
        AN, VN, SN = (torch.stack(q, dim=1).contiguous() for q in (an, vn, sn))
        TN = torch.stack([torch.stack(q, dim=1) for q in t], dim=1)
        if extra:
            TN = torch.cat([TN, zl(extra)], dim=2)
        return AN, VN, SN, TN.contiguous()

    AN, VN, SN, TN = stacked(False, 3)
    state = dict(aicen=AN, vicen=VN, vsnon=SN, trcrn=TN)
    nocean = int(po.sum().item())
    listed = (AN > C.puny) & po[:, None]
    nlisted = int(listed.sum().item())
    ncell_listed = int(listed.any(dim=1).sum().item())
    Xn = X[:, None].expand(nb, ncat, nyb, nxb)
    Yn = Y[:, None].expand(nb, ncat, nyb, nxb)
    cat = torch.arange(ncat, dtype=torch.float64, device=dev)[None, :, None, None]
    r2 = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * X + ph) * torch.cos(q * Y)
    r = lambda p, q, ph=0.0: 0.5 + 0.5 * torch.sin(p * Xn + ph + cat) * torch.cos(q * Yn + 0.7 * cat)
    forcing = {k: z2() for k in ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "sss", "aice", "frzmlt", "sst", "Tf", "strocnxT", "strocnyT",
                                 "uatm", "vatm", "wind", "zlvl", "frain")}
    forcing["shcoef"], forcing["lhcoef"], forcing["fswthrun"] = z3(), z3(), z3()
    inout = {"fswsfcn": z3(), "fswintn": z3(), "Sswabsn": zl(nslyr), "Iswabsn": zl(nilyr), "fpond": z2(), "mlt_onset": z2(), "frz_onset": z2()}
    outp = {k: z3() for k in evpk.THERMO_OUT + ["aicen_init", "vicen_init"]}
    outp.update({k: z2() for k in ("rside", "aice_init")})
    merged = {k: z2() for k in ["Cdn_atm"] + evpk.THERM1_MERGED}
    ponds = dict(dhsn=z3(), ffracn=z3(), Tair=z2(), fsnow=forcing["fsnow"], frzpnd="hlid", dpscale=1.0e-3, hs1=0.03)
    sw_forcing = {k: z2() for k in evpk.DEDD_FORCING}
    coszen, coszen0 = z2(), z2()
    sw_out = {k: z3() for k in evpk.DEDD_OUT}
    sw_out.update(Sswabsn=zl(nslyr), Iswabsn=zl(nilyr), fswpenln=zl(nilyr + 1))
    sw_out.update({k: z2() for k in evpk.DEDD_OUT2D})

    # the melting mix of scripts/therm1s_bench.py, with rain and ponds
    forcing["aice"].copy_(AN.sum(dim=1))
    forcing["Tf"].fill_(-1.8)
    forcing["frzmlt"].copy_(torch.where(r2(3, 5, 0.4) > 0.5, -20.0 - 200.0 * r2(7, 3), 30.0 * r2(5, 7)))
    forcing["sst"].copy_(-1.8 + 2.0 * r2(11, 9, 1.3))
    tau = 10.0 ** (-4.0 + 3.0 * r2(13, 17))
    forcing["strocnxT"].copy_(tau * torch.cos(9 * X)); forcing["strocnyT"].copy_(tau * torch.sin(9 * X))
    forcing["wind"].copy_(0.5 + 14.5 * r2(15, 21, 0.9))
    forcing["uatm"].copy_(forcing["wind"] * torch.cos(5 * Y)); forcing["vatm"].copy_(forcing["wind"] * torch.sin(5 * Y))
    forcing["zlvl"].fill_(10.0)
    forcing["rhoa"].fill_(1.3); forcing["sss"].fill_(34.0)
    forcing["fsnow"].copy_(torch.where(r2(19, 23) > 0.5, 2.0e-5 * r2(7, 5), z2()))
    forcing["frain"].copy_(torch.where(r2(17, 29) > 0.5, 1.0e-5 * r2(9, 11), z2()))
    forcing["potT"].copy_(271.0 + 6.0 * r2(31, 37)); forcing["flw"].copy_(280.0 + 50.0 * r2(41, 29, 2.0))
    forcing["Qa"].copy_(3.0e-3 + 1.0e-3 * r2(11, 13))
    ponds["Tair"].copy_(forcing["potT"])
    sw = 40.0 + 110.0 * r(23, 19)
    inout["fswsfcn"].copy_(0.5 * sw); inout["fswintn"].copy_(0.25 * sw); forcing["fswthrun"].copy_(0.05 * sw)
    wl = [0.5 ** k for k in range(nilyr)]
    for k in range(nilyr):
        inout["Iswabsn"][:, :, k] = 0.25 * sw * wl[k] / sum(wl)
    Ttop = -0.5 - 2.5 * r(43, 47)
    SN.copy_(AN * torch.where(r(53, 59) > 0.6, 0.02 + 0.1 * r(5, 3), z3()))
    Tsfc = torch.where(r(61, 67) > 0.5, z3(), Ttop - 0.3)
    TN[:, :, TR["nt_Tsfc"] - 1] = Tsfc
    TN[:, :, TR["nt_qsno"] - 1] = -C.rhos * (C.Lfresh - C.cp_ice * torch.clamp(0.5 * (Tsfc + Ttop), max=0.0))
    for k in range(nilyr):
        S = 2.0 + 3.0 * r(3, 2, 0.3 * k) + 2.0 * (k + 0.5) / nilyr
        Tm = -S * DEPRESST
        T = torch.minimum(Ttop + (-1.9 - Ttop) * (k + 0.5) / nilyr, Tm - 0.05)
        TN[:, :, TR["nt_sice"] - 1 + k] = S
        TN[:, :, TR["nt_qice"] - 1 + k] = -C.rhoi * (C.cp_ice * (Tm - T) + C.Lfresh * (1.0 - Tm / T) - CP_OCN * Tm)
    ice = AN > 0.0
    TN[:, :, TR["nt_alvl"] - 1] = torch.where(ice, 0.5 + 0.4 * r(7, 9), z3())
    TN[:, :, TR["nt_vlvl"] - 1] = TN[:, :, TR["nt_alvl"] - 1]
    TN[:, :, TR["nt_apnd"] - 1] = torch.where(ice, 0.1 + 0.3 * r(13, 17), z3())
    TN[:, :, TR["nt_hpnd"] - 1] = torch.where(ice, 0.05 + 0.35 * r(29, 31), z3())
    TN[:, :, TR["nt_ipnd"] - 1] = torch.where(ice & (r(37, 41) > 0.5), 0.02 * r(11, 5), z3())
    swt = 40.0 + 110.0 * r2(23, 19)
    coszen0.copy_(torch.where(ocean, 0.2 + 0.7 * r2(3, 2), z2()))
    for k, w in (("swvdr", 0.28), ("swvdf", 0.24), ("swidr", 0.31), ("swidf", 0.17)):
        sw_forcing[k].copy_(w * swt)
    out.update(listed_cell_categories=nlisted)

    keep = {k: q.clone() for k, q in list(state.items()) + list(inout.items()) + [("dhsn", ponds["dhsn"])]}

    def restore():
        for k, q in list(state.items()) + list(inout.items()):
            q.copy_(keep[k])
        ponds["dhsn"].copy_(keep["dhsn"])
        coszen.copy_(coszen0)

    def th(lvl):
        if lvl:
            stop = ctx.step_therm1_lvl(dt, state, forcing, inout, outp, merged, ponds, ntrcr, TRL, yday=100.0, constants=K, ustar_min=0.005)
        else:
            stop = ctx.step_therm1(dt, state, forcing, inout, outp, merged, ntrcr, TRC, yday=100.0, constants=K, ustar_min=0.005)
        assert stop is None, stop

    def rad(lvl):
        if lvl:
            ctx.step_radiation_dedd_lvl(dt, state, sw_forcing, coszen, sw_out, ponds, ntrcr, TRL)
        else:
            ctx.step_radiation_dedd(state, sw_forcing, coszen, sw_out, ntrcr, TRC)

    if a.only in ("all", "lvl"):
        out["step_therm1_lvl"] = timed(lambda: th(True), restore)
        npond = int((listed & (TN[:, :, TR["nt_hpnd"] - 1] > 0.0)).sum().item())      # the state the last call left
        gb = 8 * (35 * nlisted + 3 * (nocean * ncat - nlisted) + cells * ncat + 47 * ncell_listed + 2 * nilyr * npond) / 1e9
        out.update(ponds_on_return=npond, compulsory_GB_k_therm1_merge_lvl=gb)
        out["step_radiation_dedd_lvl"] = timed(lambda: rad(True), restore)
    if a.only in ("all", "cesm"):
        out["step_therm1_cesm"] = timed(lambda: th(False), restore)
        out["step_radiation_dedd_cesm"] = timed(lambda: rad(False), restore)
    del keep, AN, VN, SN, TN, state
    torch.cuda.empty_cache()

    if a.only == "all" or a.kernel_ms:
        # the yardstick: cleanup_itd where every block shifts (scripts/itd_bench.py, case b), same session, same box
        AN, VN, SN, TN = stacked(True, 0)
        keep = [q.clone() for q in (AN, VN, SN, TN)]
        fl = {k: z2() for k in ("fpond", "fresh", "fsalt", "fhocn")}
        a0, a1 = z2(), z2()

        def restore_itd():
            for q, k in zip((AN, VN, SN, TN), keep):
                q.copy_(k)

        def call():
            assert ctx.cleanup_itd(dt, AN, VN, SN, TN, a0, a1, ntr0, ib.DEP, ib.TR, ib.HIN_MAX[:ncat + 1], None, fl, None) is None
        row = timed(call, restore_itd)
        nl = int(lm.sum())
        cgb = 8 * nl * (3 * ncat + ncat * nslyr + 1 + 2) / 1e9 + 2 * 8 * nl * (3 + ntr0) * ncat / 1e9
        row.update(compulsory_GB=cgb, GBps_of_compulsory=cgb / (row["ms_min"] * 1e-3))
        out["cleanup_itd_b_every_block_shifts"] = row
        if a.kernel_ms and "compulsory_GB_k_therm1_merge_lvl" in out:
            km = float(a.kernel_ms)
            rate = out["compulsory_GB_k_therm1_merge_lvl"] / (km * 1e-3)
            out["k_therm1_merge_lvl_from_trace"] = {"ms": km, "GBps": rate, "GBps_ratio_to_cleanup_itd_b": rate / row["GBps_of_compulsory"]}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
