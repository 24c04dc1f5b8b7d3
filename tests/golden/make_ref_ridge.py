"""Makes tests/golden/ref_ridge_<cfg>.<case>.npz from the reference's own ridge_ice: oracle/_ref/<cfg>/ref_ridge (oracle/ref/Makefile, target ridge +
oracle/ref/ref_ridge.F90, built by __graft_entry__.build() where the reference is present).  Inputs come from ridgevec; only the
reference's OUTPUTS are stored, on the listed cells (physical cells with tmask) in (block, j, i) order:
    aice0 (L,)  aicen / vicen / vsnon (L, ncat)  trcrn (L, ncat, ntrcr)  the 2-D diagnostics (L,)  the per-category ones (L, ncat)
    l_stop, istop, jstop, icells, repeats (nblocks,): ridge_ice's return values and the number of "Repeat ridging" lines the reference
    wrote to nu_diag for the block
and ref_ridge_stops.npz with the stop records.  The generator asserts what the fixtures must contain.

    python -m tests.golden.make_ref_ridge
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import refrun, ridgevec as rv          # noqa: E402
from tests.golden.refrun import on_cells as on_listed          # noqa: E402,F401


def run_reference(cfg, x, sw):
    """one ridge_ice call per block by the reference build of `cfg`; returns dict of full block arrays + per-block scalars"""
    d = x["d"]
    nb, ncat, ntrcr = d.nblocks, x["ncat"], x["ntrcr"]
    kp, kr = sw
    tr = x["tracers"]
    w = refrun.Writer()
    w.i4(1); w.i4(nb, ntrcr, kp, kr, x["ndtd"]); w.r8(x["dt"], x["mu_rdg"]); w.arr(x["hin_max"].astype(np.float64))
    w.arr(x["trcr_depend"])
    w.i4(*[tr.get(k, 0) for k in ("nt_qsno", "nt_alvl", "nt_vlvl", "nt_apnd", "nt_hpnd", "nt_fbri", "tr_pond_cesm", "tr_pond_lvl", "tr_pond_topo")])
    for b, (ilo, ihi, jlo, jhi) in enumerate(rv.blocks_of(d)):
        w.i4(ilo, ihi, jlo, jhi)
        for k in ["tmask", "rdg_conv", "rdg_shear", "aice0", "aicen", "vicen", "vsnon", "trcrn"] + rv.DIAG_2D + rv.DIAG_3D:
            w.arr(x[k][b])
    w.i4(0)
    r, text = refrun.run(refrun.exe("ref_ridge", cfg), w.payload())
    nxb, nyb, nc = r.take(np.int32, (3,))
    assert (nxb, nyb, nc) == (d.nx_block, d.ny_block, ncat), (nxb, nyb, nc)
    out = {k: np.zeros_like(x[k]) for k in rv.STATE + rv.DIAG_2D + rv.DIAG_3D}
    sc = np.zeros((nb, 4), dtype=np.int32)
    for b in range(nb):
        sc[b] = r.take(np.int32, (4,))
        out["aice0"][b] = r.take(np.float64, (nyb, nxb))
        for k in ("aicen", "vicen", "vsnon"):
            out[k][b] = r.take(np.float64, (ncat, nyb, nxb))
        out["trcrn"][b] = r.take(np.float64, (ncat, ntrcr, nyb, nxb))
        for k in rv.DIAG_2D:
            out[k][b] = r.take(np.float64, (nyb, nxb))
        for k in rv.DIAG_3D:
            out[k][b] = r.take(np.float64, (ncat, nyb, nxb))
    r.done()
    repeats = np.zeros(nb, dtype=np.int32)
    cur = -1
    for line in text.splitlines():
        w = line.split()
        if w[:1] == ["BLOCK"]:
            cur = int(w[1]) - 1
        elif line.strip().startswith("Repeat ridging"):
            repeats[cur] += 1
    out.update(l_stop=sc[:, 0].copy(), istop=sc[:, 1].copy(), jstop=sc[:, 2].copy(), icells=sc[:, 3].copy(), repeats=repeats)
    return out


def restate(x, sw, exp=None, per_cell_iteration=False):
    """the numpy restatement on a copy of the inputs; returns (arrays, per-block results, stop)"""
    import math
    from tests import npridge
    y = {k: x[k].copy() for k in rv.STATE + rv.DIAG_2D + rv.DIAG_3D}
    diag = {k: y[k] for k in rv.DIAG_2D + rv.DIAG_3D}
    res, stop = npridge.ridge_ice(x["dt"], x["ndtd"], sw[0], x["mu_rdg"], x["rhos"], x["hin_max"], x["tmask"], rv.blocks_of(x["d"]),
                                  x["rdg_conv"], x["rdg_shear"], y["aice0"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], x["ntrcr"],
                                  x["trcr_depend"], x["tracers"], diag, exp or math.exp, per_cell_iteration)
    return y, res, stop


def main(outdir=HERE):
    seen = dict(repeat=0, norepeat=0, conv_in_repeat=0, tmpfac0=0, tmpfacn=0, clamp=0, raft1=0, raft0=0)
    for cfg, recs in rv.RECORDS.items():
        for tcase, swn in recs:
            sw = rv.SWITCHES[swn]
            x = rv.ridge_input(cfg, tcase)
            ref = run_reference(cfg, x, sw)
            assert not ref["l_stop"].any(), (cfg, tcase, swn, ref["l_stop"])
            m = x["listed"]
            assert (ref["icells"] == m.reshape(m.shape[0], -1).sum(axis=1)).all()
            y, res, stop = restate(x, sw)
            assert stop is None
            worst = 0.0
            for k in rv.STATE + rv.DIAG_2D + rv.DIAG_3D:
                a, b = on_listed(ref[k], m), on_listed(y[k], m)
                with np.errstate(invalid="ignore", divide="ignore"):
                    r = np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(a), np.abs(b)))
                worst = max(worst, float(r.max()) if r.size else 0.0)
            for b, r in enumerate(res):
                assert r["repeats"] == ref["repeats"][b], (cfg, tcase, swn, b, r["repeats"], ref["repeats"][b])
                if ref["icells"][b] == 0:
                    continue
                if ref["repeats"][b] > 0:
                    seen["repeat"] += 1
                    if cfg == "g26x18_b8x5":
                        seen["conv_in_repeat"] = max(seen["conv_in_repeat"], int(r["conv1"].sum()))
                else:
                    seen["norepeat"] += 1
                for k in ("tmpfac0", "tmpfacn", "clamp"):
                    seen[k] += r.get(k, 0)
            ridged = on_listed(ref["dardg2ndt"], m) > 0
            raft = on_listed(ref["araftn"], m)
            seen["raft1"] += int((ridged & (raft > 0)).sum())
            seen["raft0"] += int((ridged & (raft == 0)).sum())
            print(f"{cfg}.{tcase}_{swn}: restatement (libm exp) vs reference: max rel diff {worst:.3e}; repeats per block {ref['repeats'].tolist()}")
            rec = {k: on_listed(ref[k], m) for k in rv.STATE + rv.DIAG_2D + rv.DIAG_3D}
            rec.update({k: ref[k] for k in ("l_stop", "istop", "jstop", "icells", "repeats")})
            np.savez_compressed(os.path.join(outdir, f"ref_ridge_{cfg}.{rv.record_name(tcase, swn)}.npz"), **rec)
    print(seen)
    # what the fixtures must contain (ISSUE: block-wide iteration, both reductions, the round-off clamp, both values of mraftn)
    assert seen["repeat"] >= 1 and seen["norepeat"] >= 1, seen
    assert seen["conv_in_repeat"] >= 10, seen
    assert seen["tmpfac0"] >= 1 and seen["tmpfacn"] >= 1 and seen["clamp"] >= 1, seen
    assert seen["raft1"] >= 1 and seen["raft0"] >= 1, seen
    stops = {}
    for name in rv.STOPS:
        x = rv.stop_input(name)
        ref = run_reference("g24x16_b24x16", x, (1, 1))
        assert ref["l_stop"][0] == 1, name
        _, _, st = restate(x, (1, 1))
        assert st == (rv.STOPS[name]["reason"], 1, int(ref["istop"][0]), int(ref["jstop"][0])), (name, st, ref["istop"], ref["jstop"])
        stops[name] = np.array([ref["l_stop"][0], ref["istop"][0], ref["jstop"][0]], dtype=np.int32)
        print("stop", name, stops[name])
    np.savez_compressed(os.path.join(outdir, "ref_ridge_stops.npz"), **stops)


if __name__ == "__main__":
    main()
