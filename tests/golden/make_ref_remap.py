"""Generates tests/golden/ref_remap_*.npz: outputs of the reference's OWN make_masks / construct_fields / limited_gradient /
departure_points / locate_triangles / triangle_coordinates / transport_integrals / update_fields (the remap slice module of
oracle/ref/Makefile, target `kernels`, driven by oracle/ref/ref_remap.F90) on the deterministic inputs of
tests/golden/refvec.py.  Only outputs are stored.

  ref_remap_blk.<variant>.npz    single-routine records on one block   <block>/<routine>/<array>
  ref_remap_<cfg>.<case>.npz     chain records   o<order>m<rule>/{mm,tm,sig}, and the two stop cases in ref_remap_<cfg>.stops.npz

sig: the rows (edge kind 0 east / 1 north, group, iflux - i, jflux - j, sign of triarea, count) and pat: (edge kind, index
into refvec.REMAP_PATTERNS, count), both counted over the reference's compressed lists -- what assert_remap_coverage reads.

NOT pinned by these fixtures: the call order of horizontal_remap (it reaches ice_grid and cannot be built; ref_remap.F90
restates it), l_fixed_area = .true., state_to_tracers / tracers_to_state.

Runs in the build container only; called by make_ref_golden.py, or alone:   python tests/golden/make_ref_remap.py
  --courant   prints, per Courant number, which chain cases the reference stops on (how refvec.REMAP_COURANT was found)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import refrun, refvec as rv  # noqa: E402
from tests.golden.refrun import Writer  # noqa: E402
from tests.golden import make_ref_kernels as mk  # noqa: E402

NG, NV = 6, 4


def put_head(w, op, tables, order, midpt, bounds=None):
    w.i4(op)
    if bounds is not None:
        w.i4(*bounds)
    w.i4(len(tables[0]), order, midpt); w.r8(rv.REMAP_DT)
    for t in tables:
        w.arr(np.ascontiguousarray(t, dtype=np.int32))


def block_records(exe):
    cfg = rv.REMAP_BLOCK_CFG
    nx, ny, bx, by, _ = rv.KERNEL_CONFIGS[cfg]
    shp, nn, ncp = (by + 2, bx + 2), (by + 2) * (bx + 2), rv.REMAP_NCAT + 1
    w, plan = Writer(), []
    for rec, bounds in rv.BLOCK_RECORDS[cfg].items():
        for var in rv.REMAP_BLOCK_VARIANTS:
            mm, tm, q, tables, order, midpt = rv.remap_block_inputs(rec, var)
            nt = len(tables[0])
            put_head(w, 30, tables, order, midpt, bounds)
            w.arr(mm); w.arr(tm)
            for k in rv.REMAP_BLOCK_GRID:
                w.arr(q[k])
            plan.append((f"{rec}/{var}", nt))
    r, _ = mk.run(exe, cfg, "cyclic", "open", "none", w, ncat=rv.REMAP_NCAT)
    out = {}
    for pre, nt in plan:
        T = lambda *s: r.take(np.float64, s)
        I = lambda *s: r.take(np.int32, s)
        o = {}
        o["make_masks/icells"] = I(ncp)
        o["make_masks/indxi"], o["make_masks/indxj"] = I(ncp, nn), I(ncp, nn)
        o["make_masks/mmask"] = T(ncp, *shp)
        o["make_masks/tmask"] = T(ncp - 1, nt, *shp)
        o["limited_gradient/gx"], o["limited_gradient/gy"] = T(*shp), T(*shp)
        for k in ("mc", "mx", "my"):
            o[f"construct_fields/{k}"] = T(ncp, *shp)
        for k in ("tc", "tx", "ty"):
            o[f"construct_fields/{k}"] = T(ncp - 1, nt, *shp)
        o["departure_points/stop"] = I(3)
        o["departure_points/dpx"], o["departure_points/dpy"] = T(*shp), T(*shp)
        if not o["departure_points/stop"][0]:
            for e in ("east", "north"):
                o[f"locate_triangles/{e}/icells"] = I(NG)
                o[f"locate_triangles/{e}/indxi"], o[f"locate_triangles/{e}/indxj"] = I(NG, nn), I(NG, nn)
                o[f"locate_triangles/{e}/xp"], o[f"locate_triangles/{e}/yp"] = T(NG, NV, *shp), T(NG, NV, *shp)
                o[f"locate_triangles/{e}/iflux"], o[f"locate_triangles/{e}/jflux"] = I(NG, *shp), I(NG, *shp)
                o[f"locate_triangles/{e}/triarea"], o[f"locate_triangles/{e}/edgearea"] = T(NG, *shp), T(*shp)
                o[f"triangle_coordinates/{e}/xp"], o[f"triangle_coordinates/{e}/yp"] = T(NG, NV, *shp), T(NG, NV, *shp)
                o[f"transport_integrals/{e}/mflx"] = T(ncp, *shp)
                o[f"transport_integrals/{e}/mtflx"] = T(ncp - 1, nt, *shp)
            o["update_fields/stop"] = I(ncp, 3)
            o["update_fields/mm"] = T(ncp, *shp)
            o["update_fields/tm"] = T(ncp - 1, nt, *shp)
        out.update({f"{pre}/{k}": v for k, v in o.items()})
    r.done()
    return out


def signatures(d, icng, indx, flux, tri, xy):
    """rows of sig and pat from the reference's compressed lists of every block"""
    sig, pat = {}, {}
    names = list(rv.REMAP_PATTERNS)
    for n in range(d.nblocks):
        for e in (0, 1):
            sh = rv._shifts(e == 1)
            cell = {v: k for k, v in sh.items()}
            edges = {}
            for g in range(NG):
                for q in range(icng[n][e, g]):
                    i, j = indx[n][e, 0, g, q], indx[n][e, 1, g, q]
                    a = tri[n][e, g, j - 1, i - 1]
                    assert a != 0.0
                    di, dj = flux[n][e, 0, g, j - 1, i - 1] - i, flux[n][e, 1, g, j - 1, i - 1] - j
                    k = (e, g + 1, int(di), int(dj), 1 if a > 0 else -1)
                    sig[k] = sig.get(k, 0) + 1
                    src = edges.setdefault((i, j), {})
                    src[g + 1] = cell[(int(di), int(dj))]
                    # xic: vertex 2 of group 5 / vertex 3 of group 4 when that triangle lies in BC (whose coordinates are the
                    # edge's: north x = xic, east y = -xic, ice_transport_remap.F90:2998-3014)
                    if (g + 1, src[g + 1]) in ((5, "BC"), (4, "BC")):
                        v = 2 if g + 1 == 5 else 3
                        xic = xy[n][e, 0, g, v, j - 1, i - 1] if e == 1 else -xy[n][e, 1, g, v, j - 1, i - 1]
                        src["xic%d" % (g + 1)] = 0 if xic == 0 else 1 if xic > 0 else -1
            for src in edges.values():
                for pi, name in enumerate(names):
                    ok = True
                    for g, want in rv.REMAP_PATTERNS[name].items():
                        if g == "xic":
                            got = src.get("xic5" if rv.REMAP_PATTERNS[name][5] == "BC" else "xic4")
                            ok &= got == want or (want == 1 and got == 0)          # `xic >= c0` holds at equality
                        elif isinstance(want, tuple):
                            ok &= src.get(g) != want[0]
                        else:
                            ok &= src.get(g) == want
                    if ok:
                        pat[(e, pi)] = pat.get((e, pi), 0) + 1
    return (np.array([k + (v,) for k, v in sorted(sig.items())], dtype=np.int32).reshape(-1, 6),
            np.array([k + (v,) for k, v in sorted(pat.items())], dtype=np.int32).reshape(-1, 3))


def chain(exe, cfg, case, combos, courant=None, stop=None):
    """-> {o<order>m<rule>/...}; stop cases leave rc, block, category, istop, jstop only"""
    base = rv.REMAP_CASES[case][0]
    ew, ns, land, _ = rv.DYN_CASES[base]
    d, f, mm, tm, tables = rv.remap_fields(cfg, case, courant=courant, stop=stop)
    nt, ncp, shp, nn = len(tables[0]), rv.REMAP_NCAT + 1, (d.ny_block, d.nx_block), d.ny_block * d.nx_block
    w = Writer()
    for order, midpt in combos:
        put_head(w, 31, tables, order, midpt)
        for n in range(d.nblocks):
            w.arr(mm[n]); w.arr(tm[n])
            for k in rv.REMAP_GRID:
                w.arr(f[k][n])
    r, bounds = mk.run(exe, cfg, ew, ns, land, w, ncat=rv.REMAP_NCAT)
    assert [tuple(x) for x in bounds] == [(b.ilo, b.ihi, b.jlo, b.jhi) for b in d.local_blocks]
    out = {}
    for order, midpt in combos:
        pre = f"o{order}m{midpt}"
        out[f"{pre}/stop"] = r.take(np.int32, (5,))
        if out[f"{pre}/stop"][0]:
            continue
        om, ot = np.zeros_like(mm), np.zeros_like(tm)
        icng, indx, flux, tri, xy = [], [], [], [], []
        for n in range(d.nblocks):
            om[n] = r.take(np.float64, (ncp,) + shp)
            ot[n] = r.take(np.float64, (ncp - 1, nt) + shp)
            icng.append(r.take(np.int32, (2, NG)))
            indx.append(r.take(np.int32, (2, 2, NG, nn)))
            flux.append(r.take(np.int32, (2, 2, NG) + shp))
            tri.append(r.take(np.float64, (2, NG) + shp))
            xy.append(r.take(np.float64, (2, 2, NG, NV) + shp))
        out[f"{pre}/mm"], out[f"{pre}/tm"] = om, ot
        out[f"{pre}/sig"], out[f"{pre}/pat"] = signatures(d, icng, indx, flux, tri, xy)
    r.done()
    return out


def find_courant(exes):
    for c in (0.9, 0.8, 0.7, 0.6, 0.55, 0.5, 0.45, 0.4, 0.3):
        bad = []
        for cfg, exe in exes.items():
            for case, (_, _, combos) in rv.REMAP_CASES.items():
                o = chain(exe, cfg, case, combos, courant=c)
                bad += [(cfg, case, k, tuple(v)) for k, v in o.items() if k.endswith("/stop") and v[0]]
        print(f"courant {c}: {len(bad)} stops", bad[:4])


def main(outdir=HERE):
    from tests import test_ref_pins as P
    exes = {}
    for cfg in rv.KERNEL_CONFIGS:
        mk.build(cfg)
        exes[cfg] = refrun.exe("ref_remap", cfg)
    if "--courant" in sys.argv:
        return find_courant(exes)
    out = block_records(exes[rv.REMAP_BLOCK_CFG])
    for var in rv.REMAP_BLOCK_VARIANTS:
        mk.save(os.path.join(outdir, f"ref_remap_blk.{var}.npz"), {k: v for k, v in out.items() if k.split("/")[1] == var})
    for cfg, exe in exes.items():
        per_case = {}
        for case, (_, _, combos) in rv.REMAP_CASES.items():
            per_case[case] = chain(exe, cfg, case, combos)
            mk.save(os.path.join(outdir, f"ref_remap_{cfg}.{case}.npz"), per_case[case])
        stops = {}
        for name, (_, order, midpt) in rv.REMAP_STOPS.items():
            stops[name] = chain(exe, cfg, "cyclic_open", [(order, midpt)], stop=name)[f"o{order}m{midpt}/stop"]
        mk.save(os.path.join(outdir, f"ref_remap_{cfg}.stops.npz"), stops)
        P.assert_remap_coverage(cfg, per_case, stops)


if __name__ == "__main__":
    main()
