"""Generates tests/golden/ref_dyn_<config>*.npz: outputs of the reference's OWN evp_prep1 / evp_prep2 / stress / stepu /
evp_finish / principal_stress (the slice module of oracle/ref/Makefile, target `kernels`, driven by oracle/ref/ref_kernels.F90)
on the deterministic inputs of tests/golden/refvec.py.  Only outputs are stored.

  ref_dyn_<cfg>.<variant>.npz  single-routine records  <block>/<variant>/<routine>/<array>
  ref_dyn_<cfg>.<case>.npz   chain records           ndte<n>/<array>   (split by case to keep every file under 1 MiB)

NOT pinned by these fixtures (ice_grid cannot be built): the T<->U averages.  aiu, umass, the U-grid wind stress handed to the
chain and the final strocnxT / strocnyT average are computed here with the restatement's orc_to_ugrid_blk / orc_to_tgrid_blk;
the raw U-point values evp_finish wrote are stored as strocnxT_u / strocnyT_u.

Runs in the build container only; called by make_ref_golden.py, or alone:   python tests/golden/make_ref_kernels.py
"""
from __future__ import annotations

import ctypes as ct
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from cice5_amd import constants as C  # noqa: E402
from oracle import orc  # noqa: E402
from tests.golden import refrun, refvec as rv  # noqa: E402
from tests.golden.refrun import Writer  # noqa: E402

SN = rv.STRESS_NAMES
# the planes ref_kernels.F90 reads / writes, in its order
PREP2_IN = ["aiu", "umass", "fcor", "uocn", "vocn", "strairx", "strairy", "ss_tltx", "ss_tlty", "fm", "strtltx", "strtlty", "strocnx",
            "strocny", "strintx", "strinty"] + SN + ["uvel", "vvel", "uvel_init", "vvel_init"]
PREP2_OUT = PREP2_IN[9:] + ["umassdti", "waterx", "watery", "forcex", "forcey"]
STRESS_IN = ["uvel", "vvel", "dxt", "dyt", "dxhy", "dyhx", "cxp", "cyp", "cxm", "cym", "tarear", "tinyarea", "strength"] + SN + \
            ["shear", "divu", "prs_sig", "rdg_conv", "rdg_shear"]
STEPU_IN = ["Cw", "aiu", "uocn", "vocn", "waterx", "watery", "forcex", "forcey", "umassdti", "fm", "uarear", "strocnx", "strocny", "strintx",
            "strinty", "uvel_init", "vvel_init", "uvel", "vvel"]
FINISH_IN = ["Cw", "uvel", "vvel", "uocn", "vocn", "aiu", "fm", "strintx", "strinty", "strairx", "strairy", "strocnx", "strocny", "strocnxT",
             "strocnyT"]
CHAIN_IN = ["aice", "vice", "vsno", "strairxT", "strairyT", "aiu", "umass", "strairx", "strairy", "fcor", "uocn", "vocn", "ss_tltx", "ss_tlty",
            "Cdn_ocn", "strength", "dxt", "dyt", "dxhy", "dyhx", "cxp", "cyp", "cxm", "cym", "tarear", "tinyarea", "uarear", "fm", "strtltx",
            "strtlty", "strocnx", "strocny", "strintx", "strinty"] + SN + ["uvel", "vvel"]
CHAIN_OUT = ["fm", "strtltx", "strtlty", "strocnx", "strocny", "strintx", "strinty"] + SN + \
            ["uvel", "vvel", "tmass", "_sx", "_sy", "_umassdti", "_waterx", "_watery", "_forcex", "_forcey", "uvel_init", "vvel_init", "shear",
             "divu", "prs_sig", "rdg_conv", "rdg_shear", "strocnxT_u", "strocnyT_u", "sig1", "sig2"]


def build(cfg):
    return refrun.build("ref_kernels", cfg, rv.KERNEL_CONFIGS[cfg], rv.NCAT)


def run(exe, cfg, ew, ns, land, w, ncat=None):
    """-> (Reader behind the header, block bounds); ref_remap's header carries its ncat as a seventh integer"""
    nx, ny, bx, by, mxb = rv.KERNEL_CONFIGS[cfg]
    kmt, ulat = rv.kmt_ulat(nx, ny, bx, by, ew, ns, land)
    r, _ = refrun.run(exe, kmt.tobytes() + ulat.tobytes() + w.payload() + np.int32(0).tobytes(), refrun.domain_nml(ew, ns))
    hdr = r.take(np.int32, (6 if ncat is None else 7,))
    assert tuple(hdr[:5]) == (nx, ny, bx + 2, by + 2, mxb) and (ncat is None or hdr[6] == ncat), hdr
    return r, r.take(np.int32, (int(hdr[5]), 4))


def put_params(w, p, tilt):
    w.i4(10, p.ndte, p.revised_evp, int(tilt))
    w.r8(p.revp, p.ecci, p.dtei, p.dte2T, p.denom1, p.arlx1i, p.brlx, p.cosw, p.sinw, p.dragio)


def single_records(exe, cfg):
    """one call of each routine per (block record, variant)"""
    nx, ny, bx, by, _ = rv.KERNEL_CONFIGS[cfg]
    shp = (by + 2, bx + 2)
    w, plan = Writer(), []
    for rec, (ilo, ihi, jlo, jhi) in rv.BLOCK_RECORDS[cfg].items():
        for var, v in rv.BLOCK_VARIANTS.items():
            q = rv.block_inputs(cfg, rec, var)
            put_params(w, rv.block_params(var), v["tilt_from_slope"])
            pre = f"{rec}/{var}"
            w.i4(11, ilo, ihi, jlo, jhi)
            for k in ("aice", "vice", "vsno", "strairxT", "strairyT"):
                w.arr(q[k])
            w.arr(q["tmask"])
            plan += [(f"{pre}/evp_prep1/{k}", np.float64, shp) for k in ("strairx", "strairy", "tmass")] + [(f"{pre}/evp_prep1/icetmask", np.int32, shp)]
            w.i4(12, ilo, ihi, jlo, jhi); w.r8(rv.DYN_DT)
            for k in PREP2_IN:
                w.arr(q[k])
            for k in ("umask", "icetmask", "iceumask"):
                w.arr(q[k])
            plan += [(f"{pre}/evp_prep2/{k}", np.float64, shp) for k in PREP2_OUT] + [(f"{pre}/evp_prep2/iceumask", np.int32, shp),
                     (f"{pre}/evp_prep2/icell", np.int32, (2,)), (f"{pre}/evp_prep2/indx", np.int32, (4, shp[0] * shp[1]))]
            w.i4(13, v["ksub"], q["icellt"]); w.arr(q["indxt"])
            for k in STRESS_IN:
                w.arr(q[k])
            plan += [(f"{pre}/stress/{k}", np.float64, shp) for k in STRESS_IN[13:]] + [(f"{pre}/stress/str", np.float64, (8,) + shp)]
            w.i4(14, q["icellu"]); w.arr(q["indxu"])
            for k in STEPU_IN:
                w.arr(q[k])
            w.arr(q["str"])
            plan += [(f"{pre}/stepu/{k}", np.float64, shp) for k in ("strocnx", "strocny", "strintx", "strinty", "uvel", "vvel")]
            w.i4(15, q["icellu"]); w.arr(q["indxu"])
            for k in FINISH_IN:
                w.arr(q[k])
            plan += [(f"{pre}/evp_finish/{k}", np.float64, shp) for k in ("strocnx", "strocny", "strocnxT", "strocnyT")]
            w.i4(16)
            for k in ("stressp_1", "stressm_1", "stress12_1", "prs"):
                w.arr(q[k])
            plan += [(f"{pre}/principal_stress/{k}", np.float64, shp) for k in ("sig1", "sig2")]
    r, _ = run(exe, cfg, "cyclic", "open", "none", w)
    out = {k: r.take(dt, s) for k, dt, s in plan}
    r.done()
    return out


def to_grid(d, f, a, fn):
    """orc_to_ugrid_blk / orc_to_tgrid_blk on every block (the UNPINNED averages of ice_grid)"""
    L = orc.lib()
    fn = getattr(L, fn)
    fn.argtypes = [ct.c_int] * 6 + [orc.c_f64p] * 4
    out = np.zeros_like(a)
    for n, b in enumerate(d.local_blocks):
        fn(d.nx_block, d.ny_block, b.ilo, b.ihi, b.jlo, b.jhi, orc._p64(a[n]), orc._p64(f["tarea"][n]), orc._p64(f["uarea"][n]), orc._p64(out[n]))
    return out


def chain_records(exe, cfg, case):
    ew, ns, land, var = rv.DYN_CASES[case]
    d, f = rv.dyn_fields(cfg, case)
    nb, shp = d.nblocks, (d.ny_block, d.nx_block)
    # pass 1: the reference's evp_prep1 per block, for tmass (-> umass)
    w = Writer()
    for n, b in enumerate(d.local_blocks):
        w.i4(11, b.ilo, b.ihi, b.jlo, b.jhi)
        for k in ("aice", "vice", "vsno", "strairxT", "strairyT"):
            w.arr(f[k][n])
        w.arr(f["tmask"][n])
    r, bounds = run(exe, cfg, ew, ns, land, w)
    assert [tuple(x) for x in bounds] == [(b.ilo, b.ihi, b.jlo, b.jhi) for b in d.local_blocks]
    tmass = np.zeros((nb,) + shp)
    for n in range(nb):
        r.take(np.float64, (2,) + shp); tmass[n] = r.take(np.float64, shp); r.take(np.int32, shp)
    g = dict(f)
    g["umass"] = to_grid(d, f, tmass, "orc_to_ugrid_blk")
    g["aiu"] = to_grid(d, f, f["aice_init"], "orc_to_ugrid_blk")
    if var["wind_on_ugrid"]:
        g["strairx"], g["strairy"] = f["strax"], f["stray"]
    else:
        for k in ("strairx", "strairy"):
            a = f[k + "T"].copy(); orc.halo_r8(d, a, C.LOC_CENTER, C.KIND_VECTOR, 0.0)
            g[k] = to_grid(d, f, a, "orc_to_ugrid_blk")
    # pass 2: the chains
    w, out = Writer(), {}
    for ndte in rv.DYN_NDTE:
        pk, po = rv.dyn_params(cfg, case, ndte, f, d)
        for k in ("revp", "ecci", "denom1", "arlx1i", "brlx", "cosw", "sinw", "ndte", "revised_evp"):
            assert getattr(pk, k) == getattr(po, k), k
        put_params(w, po, var["tilt_from_slope"])
        w.i4(20); w.r8(rv.DYN_DT); w.i4(ndte, int(ns == "tripole"))
        for n in range(nb):
            for k in CHAIN_IN:
                w.arr(g[k][n])
            for k in ("tmask", "umask", "iceumask"):
                w.arr(f[k][n])
    r, _ = run(exe, cfg, ew, ns, land, w)
    for ndte in rv.DYN_NDTE:
        o = {k: np.zeros((nb,) + shp) for k in CHAIN_OUT}
        o["iceumask"], o["icetmask"] = np.zeros((nb,) + shp, np.int32), np.zeros((nb,) + shp, np.int32)
        cnt = np.zeros((nb, 2), np.int32)
        for n in range(nb):
            pl = r.take(np.float64, (len(CHAIN_OUT),) + shp)
            for i, k in enumerate(CHAIN_OUT):
                o[k][n] = pl[i]
            o["iceumask"][n], o["icetmask"][n] = r.take(np.int32, (2,) + shp)
            cnt[n] = r.take(np.int32, (2,))
        assert np.array_equal(o["tmass"], tmass)
        for k in ("strocnxT", "strocnyT"):          # u2tgrid_vector with the restatement's (unpinned) average
            a = o[k + "_u"].copy(); orc.halo_r8(d, a, C.LOC_NECORNER, C.KIND_VECTOR, 0.0)
            t = o[k + "_u"].copy()                   # to_tgrid writes physical cells only; the rest keeps evp_finish's values
            for n, b in enumerate(d.local_blocks):
                t[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = to_grid(d, f, a, "orc_to_tgrid_blk")[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi]
            o[k] = t
        o["icell"] = cnt
        for k, v in o.items():
            if not k.startswith("_"):
                out[f"ndte{ndte}/{k}"] = v
    r.done()
    return d, f, out


def save(path, out):
    np.savez_compressed(path, **out)
    kib = os.path.getsize(path) / 1024
    print(f"wrote {os.path.relpath(path, ROOT)} ({kib:.0f} KiB, {len(out)} arrays)")
    assert kib < 1024, "fixture over 1 MiB: split it"


def main(outdir=HERE):
    from tests import test_ref_pins as P
    for cfg in rv.KERNEL_CONFIGS:
        exe = build(cfg)
        out = single_records(exe, cfg)
        P.assert_block_coverage(cfg, out)
        for var in rv.BLOCK_VARIANTS:                # one file per variant: dense random planes do not compress
            save(os.path.join(outdir, f"ref_dyn_{cfg}.{var}.npz"), {k: v for k, v in out.items() if k.split("/")[1] == var})
        for case in rv.DYN_CASES:
            d, f, out = chain_records(exe, cfg, case)
            P.assert_chain_coverage(cfg, case, d, f, out)
            save(os.path.join(outdir, f"ref_dyn_{cfg}.{case}.npz"), out)


if __name__ == "__main__":
    main()
