"""Makes tests/golden/ref_itd_<cfg>.<case>.npz from the reference's own cleanup_itd, bound_state and aggregate: oracle/_ref/<cfg>/ref_itd
(oracle/ref/Makefile, target itd + oracle/ref/ref_itd.F90, built by __graft_entry__.build() where the reference is present).  Inputs come from itdvec;
only the reference's OUTPUTS are stored:
  after cleanup_itd alone, on the physical ocean cells in (block, j, i) order:
    aicen / vicen / vsnon (L, ncat)  trcrn (L, ncat, ntrcr)  aice0, aice, fpond, fresh, fsalt, fhocn (L,)  first_ice (L, ncat)
    l_stop, istop, jstop (nblocks,)
  after the chain cleanup_itd -> bound_state -> aggregate -> tendencies:
    g_aicen / g_vicen / g_vsnon (G, ncat), g_trcrn (G, ncat, ntrcr): the cells outside the physical windows (ghost cells, padding) in
    (block, j, i) order -- on physical cells bound_state changes nothing, which the generator asserts
    c_aice, c_vice, c_vsno, c_aice0 (nb, ny, nx), c_trcr (nb, ntrcr, ny, nx): aggregate's outputs on every cell
    daidtd, dvidtd, dagedtd (P,): the tendencies on the physical cells
and ref_itd_stops.npz with the stop records.  The generator asserts what the fixtures must contain (coverage()).

    python -m tests.golden.make_ref_itd
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import itdvec as iv, refrun          # noqa: E402
from tests.golden.refrun import Writer, on_cells, padded, same          # noqa: E402,F401

CELL2 = ["aice0", "aice"] + iv.FLUX
IDX = tuple(k for k in refrun.IDX if k not in ("nt_sice", "nt_FY"))          # what ref_itd.F90 reads


def run_reference(x):
    """the driver on one input; returns (after cleanup, after the chain or None), dicts of full block arrays"""
    cfg, d = x["cfg"], x["d"]
    _, _, _, _, mxb = iv.CONFIGS[cfg]
    nb, ncat, ntrcr, ny, nx = d.nblocks, x["ncat"], x["ntrcr"], d.ny_block, d.nx_block
    ew, ns, _ = iv.BOUNDS[x["bcase"]]
    kmt, ulat = iv.kmt_ulat(cfg, x["bcase"])
    tr = x["tracers"]
    t20 = np.zeros((mxb, ncat, iv.MAX_NTRCR, ny, nx))
    t20[:nb, :, :ntrcr] = x["trcrn"]
    w = Writer()
    w.arr(kmt.astype(np.float64)); w.arr(ulat.astype(np.float64)); w.i4(1); w.i4(ntrcr); w.i4(*[tr.get(k, 0) for k in IDX])
    w.r8(x["dt"], x["k"]["Tocnfrz"]); w.arr(x["hin_max"].astype(np.float64)); w.arr(x["trcr_depend"]); w.arr(x["tmask"])
    for k in ("aicen", "vicen", "vsnon"):
        w.arr(padded(x[k], mxb))
    w.arr(t20)
    for k in CELL2 + iv.TEND:
        w.arr(padded(x[k], mxb))
    w.arr(padded(x["first_ice"], mxb)); w.i4(0)
    r, _ = refrun.run(refrun.exe("ref_itd", cfg), w.payload(), refrun.domain_nml(ew, ns))
    hdr = r.take(np.int32, (6,))
    assert tuple(hdr) == (nx, ny, ncat, iv.MAX_NTRCR, mxb, nb), hdr
    blk = r.take(np.int32, (nb, 4))
    assert [tuple(r) for r in blk] == iv.blocks_of(d)
    st = r.take(np.int32, (nb, 3))
    one = dict(l_stop=st[:, 0].copy(), istop=st[:, 1].copy(), jstop=st[:, 2].copy())
    for k in ("aicen", "vicen", "vsnon"):
        one[k] = r.take(np.float64, (mxb, ncat, ny, nx))[:nb]
    one["trcrn"] = np.ascontiguousarray(r.take(np.float64, (mxb, ncat, iv.MAX_NTRCR, ny, nx))[:nb, :, :ntrcr])
    w = r.take(np.float64, (6, mxb, ny, nx))
    for q, k in enumerate(CELL2):
        one[k] = w[q, :nb].copy()
    one["first_ice"] = r.take(np.int32, (mxb, ncat, ny, nx))[:nb]
    chain = int(r.take(np.int32, (1,))[0])
    two = None
    if chain:
        two = {}
        for k in ("aicen", "vicen", "vsnon"):
            two[k] = r.take(np.float64, (mxb, ncat, ny, nx))[:nb]
        two["trcrn"] = np.ascontiguousarray(r.take(np.float64, (mxb, ncat, iv.MAX_NTRCR, ny, nx))[:nb, :, :ntrcr])
        w = r.take(np.float64, (4, mxb, ny, nx))
        for q, k in enumerate(("aice", "vice", "vsno", "aice0")):
            two[k] = w[q, :nb].copy()
        two["trcr"] = np.ascontiguousarray(r.take(np.float64, (mxb, iv.MAX_NTRCR, ny, nx))[:nb, :ntrcr])
        w = r.take(np.float64, (3, mxb, ny, nx))
        for q, k in enumerate(iv.TEND):
            two[k] = w[q, :nb].copy()
    r.done()
    return one, two


def restate(x, chain=True, fluxes=True):
    """the numpy restatement on a copy of the inputs: (after cleanup, after the chain or None, infos, stop)"""
    from cice5_amd import constants as C
    from oracle import orc
    from tests import npitd
    d = x["d"]
    y = {k: x[k].copy() for k in iv.STATE + CELL2 + iv.TEND + ["first_ice"]}
    fl = {k: y[k] for k in iv.FLUX} if fluxes else None
    infos, stop = npitd.cleanup_itd(iv.blocks_of(d), x["dt"], x["ntrcr"], x["trcr_depend"], x["tracers"], x["hin_max"], x["k"], y["aicen"],
                                    y["vicen"], y["vsnon"], y["trcrn"], y["aice0"], y["aice"], fl, y["first_ice"])
    if stop or not chain:
        return y, None, infos, stop
    z = {k: v.copy() for k, v in y.items()}
    nb, ncat, ntrcr, ny, nx = x["trcrn"].shape
    for k in ("aicen", "vicen", "vsnon", "trcrn"):                      # bound_state: ice_HaloUpdate, centre scalar, of every slice
        flat = z[k].reshape(nb, -1, ny, nx)
        for q in range(flat.shape[1]):
            w = np.ascontiguousarray(flat[:, q])
            orc.halo_r8(d, w, C.LOC_CENTER, C.KIND_SCALAR, 0.0)
            flat[:, q] = w
    z["vice"], z["vsno"], z["trcr"] = np.zeros((nb, ny, nx)), np.zeros((nb, ny, nx)), np.zeros((nb, ntrcr, ny, nx))
    npitd.aggregate(x["dt"], x["ntrcr"], x["trcr_depend"], x["tracers"], x["tmask"], iv.blocks_of(d), z["aicen"], z["vicen"], z["vsnon"],
                    z["trcrn"], z["aice"], z["vice"], z["vsno"], z["aice0"], z["trcr"], z["daidtd"], z["dvidtd"], z["dagedtd"],
                    x["k"]["Tocnfrz"])
    return y, z, infos, None


def record(x, one, two):
    m, ph = x["ocean"], x["phys"]
    rec = {k: on_cells(one[k], m) for k in iv.STATE + CELL2 + ["first_ice"]}
    rec.update({k: one[k] for k in ("l_stop", "istop", "jstop")})
    for k in iv.STATE:
        rec["g_" + k] = on_cells(two[k], ~ph)
    for k in ("aice", "vice", "vsno", "aice0", "trcr"):
        rec["c_" + k] = two[k]
    for k in iv.TEND:
        rec[k] = on_cells(two[k], ph)
    return rec


def restated_record(x, y, z):
    return record(x, dict(y, l_stop=np.zeros(x["d"].nblocks, np.int32), istop=np.zeros(x["d"].nblocks, np.int32),
                          jstop=np.zeros(x["d"].nblocks, np.int32)), z)


def coverage(x, ref, infos, seen):
    """counts the paths a record takes: from the reference's record `ref` and the restatement's per-block infos (the restatement equals
    the record bit for bit: tests/test_itd_ref.py)"""
    m = x["ocean"]
    nb = m.shape[0]
    cells = np.argwhere(m)                           # (L, 3): block, j, i in the record's order
    row = {tuple(c): q for q, c in enumerate(cells)}
    t_in = on_cells(x["trcrn"], m)
    a_out = ref["aicen"]
    seen["hin0>0" if x["hin_max"][0] > 0 else "hin0=0"] += 1
    for b, info in enumerate(infos):
        rows = np.array([q for q, c in enumerate(cells) if c[0] == b], dtype=np.int64)
        if not len(rows):
            continue
        J, I = info["listed"]
        seen["adjusted"] += len(info["adjusted"][0])
        if not info["boundaries"]:
            if np.array_equal(ref["trcrn"][rows], t_in[rows]) or not info["zap1"]:
                seen["block_noshift"] += 1
        else:
            donor = np.zeros(len(J), dtype=np.int64)
            for way, n, sel in info["boundaries"]:
                seen[way] += int(sel.sum())
                donor += sel
            seen["cascade"] += int((donor >= 2).sum())
            kd = x["kinds"][b, J, I]
            seen["edge_up_stays"] += int(((kd == iv.KINDS.index("edge_up")) & (donor == 0)).sum())
            seen["edge_down_moves"] += int(((kd == iv.KINDS.index("edge_down")) & (donor == 1)).sum())
            ride = 0
            for q in np.nonzero(donor == 0)[0]:
                r = row[(b, J[q], I[q])]
                live = a_out[r] > iv.PUNY
                if (ref["trcrn"][r][live] != t_in[r][live]).any():
                    ride += 1
            seen["ride_lastbit"] += ride
            if (donor > 0).any() and (donor == 0).any():
                seen["block_mixed"] += 1
            listed = {(int(j), int(i)) for j, i in zip(J, I)}
            for r in rows:
                _, j, i = cells[r]
                if (int(j), int(i)) not in listed and (t_in[r] != 0).any() and not (ref["trcrn"][r] != 0).any():
                    seen["unlisted_zeroed"] += 1
        for n, j, i, a in info["zap1"]:
            assert ref["first_ice"][row[(b, j, i)], n] == 1
            seen["zap1+" if a > 0 else "zap1-"] += 1
        for j, i in info["zap2"]:
            assert ref["aice"][row[(b, j, i)]] == 1.0
            seen["zap2"] += 1
        for n, j, i, why in info["zapT"]:
            assert ref["vsnon"][row[(b, j, i)], n] == 0.0
            seen["zapT_" + why] += 1
        seen["thin_kept"] += len(info.get("thin_kept", []))
    return seen


COVER = ["up", "down", "cascade", "edge_up_stays", "edge_down_moves", "block_noshift", "block_mixed", "ride_lastbit", "unlisted_zeroed", "adjusted", "hin0>0", "hin0=0", "zap1+",
         "zap1-", "zap2", "zapT_cold", "zapT_warm", "thin_kept"]


def main(outdir=HERE):
    seen = {k: 0 for k in COVER}
    for cfg, recs in iv.RECORDS.items():
        for tcase, bcase in recs:
            x = iv.itd_input(cfg, tcase, bcase)
            one, two = run_reference(x)
            assert not one["l_stop"].any() and two is not None, (cfg, tcase, bcase, one["l_stop"], one["istop"], one["jstop"])
            # bound_state leaves the physical cells alone
            for k in iv.STATE:
                assert np.array_equal(on_cells(one[k], x["phys"]), on_cells(two[k], x["phys"]), equal_nan=True), k
            rec = record(x, one, two)
            y, z, infos, stop = restate(x)
            assert stop is None
            got = restated_record(x, y, z)
            bad = [k for k in rec if not same(rec[k], got[k])]
            print(f"{cfg}.{tcase}_{bcase}: restatement vs reference differs in {bad or 'nothing'}")
            coverage(x, rec, infos, seen)
            path = os.path.join(outdir, f"ref_itd_{cfg}.{iv.record_name(tcase, bcase)}.npz")
            np.savez_compressed(path, **rec)
            print(f"   {os.path.getsize(path) / 1024:.0f} KiB")
    print(seen)
    assert all(seen[k] >= 1 for k in COVER), seen
    stops = {}
    for name, sp in iv.STOPS.items():
        x = iv.stop_input(name)
        one, two = run_reference(x)
        assert two is None
        b = int(np.nonzero(one["l_stop"])[0][0])
        _, _, _, st = restate(x)
        print("stop", name, "reference: blocks", np.nonzero(one["l_stop"])[0] + 1, "first", (b + 1, one["istop"][b], one["jstop"][b]), "restatement", st)
        assert (b + 1, int(one["istop"][b]), int(one["jstop"][b])) == sp["expect"], name
        stops[name] = np.stack([one["l_stop"], one["istop"], one["jstop"]]).astype(np.int32)
    np.savez_compressed(os.path.join(outdir, "ref_itd_stops.npz"), **stops)


if __name__ == "__main__":
    main()
