"""Makes tests/golden/ref_litd_<cfg>.<case>.npz and ref_therm2_<cfg>.<case>.npz from the reference's own linear_itd, add_new_ice,
lateral_melt, reduce_area, aggregate_area and cleanup_itd: oracle/_ref/<build>/ref_therm2 (oracle/ref/Makefile, target therm2 +
oracle/ref/ref_therm2.F90, built by __graft_entry__.build() where the reference is present).  Inputs come from litdvec.litd_input,
therm2vec.therm2_input and therm2vec.stop_input; only the reference's OUTPUTS are stored, on the physical ocean cells in (block, j, i)
order, the category / tracer axes last:

  ref_litd_*    (mode L: aggregate_area, the aice > puny list, linear_itd alone -- the call evpk_linear_itd makes)
      aicen / vicen / vsnon (L, ncat)  trcrn (L, ncat, ntrcr)  aice, aice0, fpond (L,)  l_stop, istop, jstop (nblocks,)
      hin_top: hin_max(ncat) as linear_itd leaves it in the module
  ref_therm2_*  (mode T: step_therm2 in its order, dumped after linear_itd, after add_new_ice, after lateral_melt / reduce_area and
                 after cleanup_itd)
      s<n>_<k>_at / s<n>_<k>_to for n = 1 .. 4, k in therm2vec.OUT (first_ice as int8): the flat positions at which the array differs bit
      for bit from what the stage before left -- for stage 1: from the input -- and the reference's values there.  Most cells keep most
      values from one stage to the next, and a full record of every stage would be four times the size of the ref_itd_* files;
      stages(rec, x) puts the four full records together again from the input x, which it checks against input_sha (sha256 of the
      input on the ocean cells as the generator saw it).
      stop (nblocks, 3, 4): l_stop, istop, jstop per block and stage;  hin_top
  ref_therm2_stop.npz   the stop record: stop (nblocks, 3, 4) of therm2vec.stop_input() under kitd = 0, ktherm = 1

The reference's AusCOM build fixes cp_ocn = 3989.24495292815 at compile time (drivers/auscom/ice_constants.F90:30), where therm2vec
carries the standard 4218: t_input() replaces that one scalar, and run_reference() asserts every constant of the input against what the
driver's header reports.  The single-category records run with kitd = 0: with ncat = 1 the reference's init_itd has no boundaries to
remap and reduce_area takes linear_itd's place (tests/test_therm2_host.py::test_single_category_takes_reduce_area restates exactly that).

The generator asserts what the device's stated departures (include/evpk.h) rely on -- physical land cells carry no ice before and after
and none of their 2-D fields changes; their tracers may be zeroed, as shift_ice's compute_tracers does in a block that shifts -- and
what the fixtures must contain (coverage()).

    python -m tests.golden.make_ref_therm2
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import itdvec as iv          # noqa: E402
from tests.golden import litdvec as lv         # noqa: E402
from tests.golden import therm2vec as tv       # noqa: E402
from tests.golden import refrun                # noqa: E402
from tests.golden.refrun import IDX, Writer, bits, on_cells, padded, same          # noqa: E402,F401

BCASE = "cyclic_open"
REF_CP_OCN = 3989.24495292815
W_OUT = ["aice0", "aice", "frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn"]
W_IN = W_OUT + ["frain", "frzmlt", "Tf", "sss", "rside"]
L_OUT = iv.STATE + ["aice", "aice0", "fpond"]
HIN_TOP = 999.9

# the builds: name -> (grid, ncat); ncat is a compile-time parameter of the reference
BUILDS = {"g26x18_b8x5": ("g26x18_b8x5", 5), "g24x16_b6x4": ("g24x16_b6x4", 5), "g26x18_b8x5_ncat3": ("g26x18_b8x5", 3),
          "g26x18_b8x5_ncat1": ("g26x18_b8x5", 1)}
# (grid, tracer table, ncat)
L_RECORDS = [(cfg, t, 5) for cfg in ("g26x18_b8x5", "g24x16_b6x4") for t in ("plain", "lvl_ponds", "cesm_ponds", "topo_ponds")] + \
            [("g26x18_b8x5", "plain", 3)]
# (grid, tracer table, ncat, kitd, ktherm, update_ocn_f)
T_RECORDS = [(cfg, t, 5, 1, kt, False) for cfg in ("g26x18_b8x5", "g24x16_b6x4") for t in tv.POND_CASES + ["bare"] for kt in (1, 2)] + \
            [("g26x18_b8x5", "plain", 5, 1, kt, True) for kt in (1, 2)] + [("g26x18_b8x5", "plain", 5, 0, 1, False)] + \
            [("g26x18_b8x5", "lvl_ponds", 1, 0, 1, False), ("g26x18_b8x5", "cesm_ponds", 1, 0, 2, False)]
STOP_RECORD = ("g26x18_b8x5", "plain", 5, 0, 1, False)
STAGES = ["linear_itd", "add_new_ice", "lateral_melt", "cleanup_itd"]


def build_of(cfg, ncat):
    return cfg if ncat == 5 else f"{cfg}_ncat{ncat}"


def l_path(cfg, tcase, ncat, outdir=HERE):
    return os.path.join(outdir, f"ref_litd_{cfg}.{tcase}{'' if ncat == 5 else f'_ncat{ncat}'}.npz")


def t_path(cfg, tcase, ncat, kitd, ktherm, ocnf, outdir=HERE):
    tag = f"{tcase}_k{ktherm}" + ("_ocnf" if ocnf else "") + ("" if kitd == 1 or ncat == 1 else "_kitd0") + ("" if ncat == 5 else f"_ncat{ncat}")
    return os.path.join(outdir, f"ref_therm2_{cfg}.{tag}.npz")


def t_input(cfg, tcase, ncat=5, stop=False):
    """therm2vec's input with the one scalar the reference fixes at compile time; a new dict, the arrays are therm2vec's"""
    x = tv.stop_input() if stop else tv.therm2_input(cfg, tcase, ncat=ncat)
    return dict(x, cp_ocn=REF_CP_OCN)


def run_reference(x, mode, kitd=1, ktherm=1, ocnf=False):
    """the driver on one input: (list of per-stage dicts of full block arrays, st (nb, 3, nstage), hin_top)"""
    cfg, d = x["cfg"], x["d"]
    ncat, ntrcr = x["ncat"], x["ntrcr"]
    _, _, _, _, mxb = lv.CONFIGS[cfg]
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    ew, ns, _ = iv.BOUNDS[BCASE]
    kmt, ulat = iv.refvec.kmt_ulat(*lv.CONFIGS[cfg][:4], ew, ns, iv.BOUNDS[BCASE][2])
    tr = x["tracers"]
    t20 = np.zeros((mxb, ncat, iv.MAX_NTRCR, ny, nx))
    t20[:nb, :, :ntrcr] = x["trcrn"]
    w = Writer()
    w.arr(kmt.astype(np.float64)); w.arr(ulat.astype(np.float64)); w.i4(mode); w.i4(ntrcr); w.i4(*[tr.get(k, 0) for k in IDX])
    w.i4(kitd, ktherm, int(ocnf))
    w.r8(x["dt"], x["k"]["Tocnfrz"], x["hi_min"], x.get("yday", 0.0), x.get("phi_init", 0.75), x.get("dSin0_frazil", 3.0))
    w.arr(x["hin_max"].astype(np.float64)); w.arr(x["trcr_depend"].astype(np.int32)); w.arr(x["tmask"].astype(np.int32))
    for k in ("aicen_init", "vicen_init", "aicen", "vicen", "vsnon"):
        w.arr(padded(x[k], mxb))
    w.arr(t20)
    for k in W_IN:
        w.arr(padded(x[k], mxb) if x.get(k) is not None else np.zeros((mxb, ny, nx)))
    sal = x.get("salinz")
    w.arr(padded(sal if sal is not None else np.zeros((nb, iv.NILYR + 1, ny, nx)), mxb))
    w.arr(padded(x["first_ice"].astype(np.int32), mxb)); w.i4(0)
    r, _ = refrun.run(refrun.exe("ref_therm2", build_of(cfg, ncat)), w.payload(), refrun.domain_nml(ew, ns))
    hdr = r.take(np.int32, (8,))
    assert tuple(hdr) == (nx, ny, ncat, iv.MAX_NTRCR, mxb, nb, iv.NILYR, 0), hdr            # (the last: pop_icediag = .false.)
    blk = r.take(np.int32, (nb, 4))
    assert [tuple(r) for r in blk] == iv.blocks_of(d)
    k = x["k"]
    const = r.take(np.float64, (10,))
    want = [k["rhoi"], k["rhos"], x.get("rhow", 1026.0), k["Lfresh"], k["cp_ice"], x.get("cp_ocn", REF_CP_OCN), k["ice_ref_salinity"], k["puny"],
            x.get("hfrazilmin", 0.05), k["hs_min"]]
    assert list(const) == want, (list(const), want)                                          # the reference's compile-time constants
    nstage = int(r.take(np.int32, (1,))[0])
    assert nstage == (1 if mode == 1 else 4)
    st = np.moveaxis(r.take(np.int32, (nstage, nb, 3)), 0, -1)                                 # (nb, 3, nstage)
    hin_top = float(r.take(np.float64, (1,))[0])
    out = []
    for s in range(nstage):
        one = {}
        for q in ("aicen", "vicen", "vsnon"):
            one[q] = r.take(np.float64, (mxb, ncat, ny, nx))[:nb]
        one["trcrn"] = np.ascontiguousarray(r.take(np.float64, (mxb, ncat, iv.MAX_NTRCR, ny, nx))[:nb, :, :ntrcr])
        w = r.take(np.float64, (len(W_OUT), mxb, ny, nx))
        for q, name in enumerate(W_OUT):
            one[name] = w[q, :nb].copy()
        one["first_ice"] = r.take(np.int32, (mxb, ncat, ny, nx))[:nb]
        out.append(one)
    r.done()
    return out, st, hin_top


def check_departures(x, stages, keys2d):
    """physical land cells: no ice before and after, no 2-D field changes (aice = 0, aice0 = 1 are aggregate_area's)"""
    land = x["phys"] & ~x["ocean"]
    for q in ("aicen", "vicen", "vsnon"):
        assert not on_cells(x[q], land).any(), q
    for one in stages:
        for q in ("aicen", "vicen", "vsnon"):
            assert not on_cells(one[q], land).any(), q
        assert not one["aice"][land].any() and (one["aice0"][land] == 1.0).all()
        for q in keys2d:
            if x.get(q) is not None:
                assert same(one[q][land], x[q][land]), q
        assert np.array_equal(on_cells(one["first_ice"], land), on_cells(x["first_ice"], land))


def l_record(x, one, st, hin_top):
    rec = {k: on_cells(one[k], x["ocean"]) for k in L_OUT}
    rec.update(l_stop=st[:, 0, 0].copy(), istop=st[:, 1, 0].copy(), jstop=st[:, 2, 0].copy(), hin_top=np.float64(hin_top))
    return rec


def cells_of_input(x):
    """the arrays of therm2vec.OUT of an input on its ocean cells, in the records' form"""
    full = {k: on_cells(x[k], x["ocean"]) for k in tv.OUT}
    full["first_ice"] = full["first_ice"].astype(np.int8)
    return full


def input_sha(x):
    h = hashlib.sha256()
    for k, v in cells_of_input(x).items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def t_record(x, stages_, st, hin_top):
    """every stage as the positions that differ bit for bit from the stage before (stage 1: from the input) and the values there"""
    m = x["ocean"]
    full = [cells_of_input(x)] + [{k: on_cells(one[k], m) for k in tv.OUT} for one in stages_]
    for f in full:
        f["first_ice"] = f["first_ice"].astype(np.int8)
    rec = {}
    for s in range(1, 5):
        for k in tv.OUT:
            at = np.nonzero(bits(full[s][k]).ravel() != bits(full[s - 1][k]).ravel())[0].astype(np.int32)
            rec[f"s{s}_{k}_at"] = at
            rec[f"s{s}_{k}_to"] = full[s][k].ravel()[at]
    rec["stop"] = st.astype(np.int32)
    rec["hin_top"] = np.float64(hin_top)
    rec["input_sha"] = np.array(input_sha(x))
    return rec


def stages(rec, x):
    """the four full per-stage records {k: array on the ocean cells} of a ref_therm2_* fixture made from the input x"""
    assert str(rec["input_sha"]) == input_sha(x), "the fixture was made from another input"
    out = [cells_of_input(x)]
    for s in range(1, 5):
        one = {}
        for k in tv.OUT:
            a = out[-1][k].copy()
            a.ravel()[rec[f"s{s}_{k}_at"]] = rec[f"s{s}_{k}_to"]
            one[k] = a
        out.append(one)
    return out[1:]


def l_input(cfg, tcase, ncat=5):
    return lv.litd_input(cfg, tcase, ncat=ncat)


def restate_l(x):
    """tests/nplitd.py on copies: (record on the ocean cells, infos, stop)"""
    from tests import nplitd
    y = {k: x[k].copy() for k in L_OUT}
    infos, stop = nplitd.linear_itd(iv.blocks_of(x["d"]), x["tmask"], x["ntrcr"], x["trcr_depend"], x["tracers"], x["hin_max"], x["hi_min"],
                                    x["k"], x["aicen_init"], x["vicen_init"], y["aicen"], y["vicen"], y["vsnon"], y["trcrn"], y["aice"], y["aice0"],
                                    y["fpond"])
    return {k: on_cells(y[k], x["ocean"]) for k in L_OUT}, infos, stop


def restate_t(x, kitd, ktherm, ocnf):
    """tests/nptherm2.py's step_therm2 on copies: (the four per-stage records on the ocean cells, infos, stop)"""
    from tests import nptherm2
    y = {k: x[k].copy() for k in tv.OUT}
    y.update({k: x[k] for k in ("aicen_init", "vicen_init", "frain", "frzmlt", "Tf", "sss", "rside", "salinz")})
    p = nptherm2.params(x, ktherm, ocnf)
    snaps = []
    infos, stop = nptherm2.step_therm2(iv.blocks_of(x["d"]), x["tmask"], p, y, kitd, x["hi_min"], y["first_ice"], stages=snaps)
    out = []
    for one in snaps:
        f = {k: on_cells(one[k], x["ocean"]) for k in tv.OUT}
        f["first_ice"] = f["first_ice"].astype(np.int8)
        out.append(f)
    return out, infos, stop


def differing(ref_stages, got_stages):
    """[(stage name, key, count)] of the arrays that differ, in stage order"""
    bad = []
    for s, (r, g) in enumerate(zip(ref_stages, got_stages)):
        for k in tv.OUT:
            if not same(r[k], g[k]):
                bad.append((STAGES[s], k, int((bits(r[k]) != bits(g[k])).sum())))
    return bad


# keys that only the mushy formulation can count (ice_therm_itd.F90:1461-1478 runs under ktherm == 2 alone)
MUSHY_ONLY = {"si_linear", "si_quadratic", "ti_clamped", "ti_unclamped", "sb_high", "sb_low"}


def coverage(seen_l, seen_t):
    """what the fixtures must contain, from the info counts of the restatement (which equals the records bit for bit:
    tests/test_therm2_ref.py): every path of linear_itd over the L records but the damax clamp, which linear_itd's own rules make
    unreachable (tests/test_litd_host.py); every path of add_new_ice / lateral_melt that tests/test_therm2_host.py asserts, at each
    ktherm.  Returns the keys that are missing."""
    from tests.test_therm2_host import REPORTED
    missing = [("L", k) for k, n in seen_l.items() if n == 0 and k != "melt_clamped"]
    for ktherm, seen in seen_t.items():
        missing += [(ktherm, k) for k, n in seen.items() if n == 0 and k not in REPORTED and not (ktherm == 1 and k in MUSHY_ONLY)]
    return missing


def main(outdir=HERE):
    from tests import nplitd, nptherm2
    seen_l = {k: 0 for k in nplitd.INFO_KEYS}
    for cfg, tcase, ncat in L_RECORDS:
        x = l_input(cfg, tcase, ncat)
        (one,), st, hin_top = run_reference(x, 1)
        assert not st[:, 0].any(), (cfg, tcase, ncat, st)
        assert hin_top == HIN_TOP
        check_departures(x, [one], ["fpond"])
        rec = l_record(x, one, st, hin_top)
        got, infos, stop = restate_l(x)
        assert stop is None
        bad = [k for k in L_OUT if not same(rec[k], got[k])]
        print(f"L {cfg}.{tcase} ncat={ncat}: restatement vs reference differs in {bad or 'nothing'}")
        for i in infos:
            for k in seen_l:
                seen_l[k] += i[k]
        path = l_path(cfg, tcase, ncat, outdir)
        np.savez_compressed(path, **rec)
        print(f"   {os.path.getsize(path) / 1024:.0f} KiB")
    print(seen_l)
    seen_t = {kt: {k: 0 for k in nptherm2.INFO_KEYS} for kt in (1, 2)}
    for cfg, tcase, ncat, kitd, ktherm, ocnf in T_RECORDS:
        x = t_input(cfg, tcase, ncat)
        full, st, hin_top = run_reference(x, 2, kitd, ktherm, ocnf)
        assert not st[:, 0].any(), (cfg, tcase, ncat, st)
        assert hin_top == (HIN_TOP if kitd == 1 else x["hin_max"][ncat])
        check_departures(x, full, ["frazil", "frz_onset", "meltl", "fpond", "fresh", "fsalt", "fhocn"])
        rec = t_record(x, full, st, hin_top)
        got, infos, stop = restate_t(x, kitd, ktherm, ocnf)
        assert stop is None
        bad = differing(stages(rec, x), got)
        print(f"T {cfg}.{tcase} ncat={ncat} kitd={kitd} ktherm={ktherm} ocnf={ocnf}: restatement vs reference differs in {bad or 'nothing'}")
        for i in infos:
            for k in seen_t[ktherm]:
                seen_t[ktherm][k] += i[k]
        path = t_path(cfg, tcase, ncat, kitd, ktherm, ocnf, outdir)
        np.savez_compressed(path, **rec)
        print(f"   {os.path.getsize(path) / 1024:.0f} KiB")
    print(seen_t)
    assert not coverage(seen_l, seen_t), coverage(seen_l, seen_t)
    cfg, tcase, ncat, kitd, ktherm, ocnf = STOP_RECORD
    x = t_input(cfg, tcase, ncat, stop=True)
    full, st, hin_top = run_reference(x, 2, kitd, ktherm, ocnf)
    blocks = np.nonzero(st[:, 0].any(axis=1))[0]
    b = int(blocks[0])
    print("stop: reference blocks", blocks + 1, "stages", [STAGES[s] for s in np.nonzero(st[b, 0])[0]], "cell", st[b, 1:, 3])
    assert not st[:, 0, :3].any() and st[b, 0, 3] == 1
    assert (b + 1, int(st[b, 1, 3]), int(st[b, 2, 3])) == x["stop_expect"][1:]
    np.savez_compressed(os.path.join(outdir, "ref_therm2_stop.npz"), stop=st.astype(np.int32))


if __name__ == "__main__":
    main()
