"""Deterministic inputs of the cleanup_itd / aggregate fixtures (tests/golden/make_ref_itd.py -> ref_itd_<cfg>.<case>.npz) and of the
tests that feed the same bytes to the numpy restatement (tests/npitd.py) and to the HIP path.  Everything comes from refvec.hash01.

A state "after ridging": thickness distributions inside their category bounds on 60 % of the ocean cells (the rest is ice-free), with
physically meaningful enthalpies (zap_snow_temperature would otherwise zap every category), and on top of it the cells that make
cleanup_itd work.  Each ice cell draws a kind:
  up, up2     one category thicker than its upper bound (up2: thicker than the next bound too, the receiver empty: a cascade)
  down, down2 one category thinner than its lower bound (down2: thinner than the bound below, the receiver empty)
  edge_up, edge_down  a category whose thickness IS its upper resp. lower bound: stays (hicen > hin_max) resp. moves down (hicen <= hin_max)
  thin1       category 1 thinner than hin_max(0) (adjusted where hin_max(0) > 0)
  tiny+, tiny-  a category of area +-0.5 puny with volume, snow and tracers (zap I)
  over        the areas sum to 1 + 4e-12 (zap II)
  cold, warm  a snow enthalpy whose temperature is below Tmin resp. above Tmax
  thinsnow    a warm snow enthalpy on snow thinner than hs_min (kept)
The shifting kinds occur only in blocks with b % 3 != 0 (b: 0-based local block), so that some blocks never call shift_ice; in a
one-block grid the block shifts.  Some ice-free cells carry tracer values (shift_ice's compute_tracers zeroes them).
"""
from __future__ import annotations

import numpy as np

from . import refvec, ridgevec
from .refvec import hash01, seed_of

CONFIGS = ridgevec.CONFIGS
NCAT = refvec.NCAT
MAX_NTRCR = refvec.MAX_NTRCR
DT = 3600.0 * 2                                   # dt * ndtd of step_ridge
PUNY = 1.0e-11
K = dict(Tocnfrz=refvec.TOCNFRZ, ice_ref_salinity=5.0, hs_min=1.0e-4, cp_ice=2106.0, Lfresh=2.835e6 - 2.501e6, Tmin=-100.0, puny=PUNY,
         rhoi=917.0, rhos=330.0)
NILYR, NSLYR = 4, 1                               # NICELYR, NSNWLYR of the reference build

# Tsfc, qice x 4, qsno, alvl, vlvl, apnd, hpnd, fbri, a brine tracer: ridgevec's tables with nt_Tsfc = 1 and four enthalpy layers
_FULL = dict(nt_Tsfc=1, nt_qice=2, nilyr=NILYR, nt_qsno=6, nslyr=NSLYR, nt_alvl=7, nt_vlvl=8, nt_apnd=9, nt_hpnd=10, nt_fbri=11, tr_brine=1)
TRACER_CASES = {
    "lvl_ponds": ([0, 1, 1, 1, 1, 2, 0, 1, 2 + 7, 2 + 9, 1, 2 + 11], dict(_FULL, tr_pond_lvl=1)),
    "cesm_ponds": ([0, 1, 1, 1, 1, 2, 0, 1, 0, 2 + 9, 1, 2 + 11], dict(_FULL, tr_pond_cesm=1)),
    "plain": ([0, 1, 1, 1, 1, 2, 1], dict(nt_Tsfc=1, nt_qice=2, nilyr=NILYR, nt_qsno=6, nslyr=NSLYR, nt_iage=7)),
    "topo_ponds": ([0, 1, 1, 1, 1, 2, 0, 1, 0, 2 + 9, 1, 2 + 11], dict(_FULL, tr_pond_topo=1)),
}
HIN0 = {"lvl_ponds": 0.0, "cesm_ponds": 0.1, "plain": 0.1, "topo_ponds": 0.0}          # hin_max(0) of the record
# (ew, ns, land pattern) of a record; the chain (bound_state, aggregate, tendencies) is part of every record
BOUNDS = {"cyclic_open": ("cyclic", "open", "patch"), "cyclic_tripole": ("cyclic", "tripole", "none"), "open_open": ("open", "open", "none")}
RECORDS = {
    "g26x18_b8x5": [("lvl_ponds", "cyclic_open"), ("cesm_ponds", "cyclic_open"), ("plain", "cyclic_open"), ("topo_ponds", "cyclic_open"),
                    ("lvl_ponds", "cyclic_tripole"), ("plain", "open_open")],
    "g24x16_b24x16": [("lvl_ponds", "cyclic_open"), ("cesm_ponds", "cyclic_open"), ("plain", "cyclic_open"), ("topo_ponds", "cyclic_open")],
}
STATE = ["aicen", "vicen", "vsnon", "trcrn"]
FLUX = ["fpond", "fresh", "fsalt", "fhocn"]
TEND = ["daidtd", "dvidtd", "dagedtd"]
KINDS = ["up", "up2", "down", "down2", "edge_up", "edge_down", "thin1", "tiny+", "tiny-", "over", "cold", "warm", "thinsnow"]


def record_name(tcase, bcase):
    return f"{tcase}_{bcase}"


def decomp(cfg, bcase="cyclic_open"):
    from cice5_amd import blocks
    nx, ny, bx, by, _ = CONFIGS[cfg]
    ew, ns, _ = BOUNDS[bcase]
    return blocks.create_distrb_cart(nx, ny, bx, by, ew_boundary_type=ew, ns_boundary_type=ns)


def kmt_ulat(cfg, bcase):
    nx, ny, bx, by, _ = CONFIGS[cfg]
    ew, ns, land = BOUNDS[bcase]
    return refvec.kmt_ulat(nx, ny, bx, by, ew, ns, land)


def tmask(cfg, d, bcase="cyclic_open"):
    """int32 (nb, ny, nx): the land mask on physical cells, ghost cells halo-updated as the model's tmask is (padding: 0)"""
    from cice5_amd import blocks, constants as C
    from oracle import orc
    nx, ny, _, _, _ = CONFIGS[cfg]
    kmt, _ = kmt_ulat(cfg, bcase)

    def fn(I, J):
        ok = (J >= 1) & (J <= ny) & (I >= 1) & (I <= nx)
        return np.where(ok, kmt[np.clip(J - 1, 0, ny - 1), np.clip(I - 1, 0, nx - 1)], 0.0)
    w = np.ascontiguousarray(blocks.to_blocks(d, fn))
    for n, b in enumerate(d.local_blocks):                       # (cells outside the physical window start as 0)
        m = np.zeros(w.shape[1:], dtype=bool)
        m[b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
        w[n][~m] = 0.0
    orc.halo_r8(d, w, C.LOC_CENTER, C.KIND_SCALAR, 0.0)
    return np.ascontiguousarray((w != 0).astype(np.int32))


def physical(d):
    m = np.zeros((d.nblocks, d.ny_block, d.nx_block), dtype=bool)
    for n, b in enumerate(d.local_blocks):
        m[n, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    return m


def blocks_of(d):
    return [(b.ilo, b.ihi, b.jlo, b.jhi) for b in d.local_blocks]


def itd_input(cfg, tcase, bcase="cyclic_open", ncat=NCAT, tag="fix", quiet=False):
    """dict of the arrays of one cleanup_itd + aggregate call on every block.  quiet: no cell shifts and none is zapped."""
    d = decomp(cfg, bcase)
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    dep, tr = TRACER_CASES[tcase]
    ntrcr = len(dep)
    h = lambda k, shape: hash01(shape, seed_of(cfg, "itd", tag, bcase, tcase if k.startswith("t") else "", k))
    hin = ridgevec.HIN_MAX.copy() if ncat == NCAT else np.concatenate([ridgevec.HIN_MAX[:ncat], [9.0]])
    hin[0] = HIN0[tcase]
    tm = tmask(cfg, d, bcase)
    phys = physical(d)
    ocean = phys & (tm != 0)
    ice = ocean & (h("ice", (nb, ny, nx)) < 0.6)
    aicen = h("a", (nb, ncat, ny, nx)) + 0.05
    aicen[h("hole", (nb, ncat, ny, nx)) < 0.25] = 0.0
    aicen[:, 0][aicen.sum(axis=1) == 0.0] = 0.3
    target = 0.05 + 0.9 * h("tot", (nb, ny, nx))
    aicen = aicen * (target / aicen.sum(axis=1))[:, None]
    frac = 0.05 + 0.9 * h("hh", (nb, ncat, ny, nx))
    lo = np.maximum(hin[:-1], 0.1)[:, None, None]
    hi = lo + frac * (hin[1:, None, None] - lo)
    vicen = aicen * hi
    vsnon = aicen * (0.01 + 0.4 * h("hs", (nb, ncat, ny, nx)))
    vsnon[h("s0", (nb, ncat, ny, nx)) < 0.2] = 0.0
    # tracers: a surface temperature, enthalpies of ice at -2 .. -20 C and of snow at -0.1 .. -40 C, fractions / depths in [0, 1)
    trcrn = h("trcrn", (nb, ncat, ntrcr, ny, nx)) * 2.0 - 0.7
    trcrn[:, :, tr["nt_Tsfc"] - 1] = -20.0 * h("tTsfc", (nb, ncat, ny, nx))
    for l in range(NILYR):
        trcrn[:, :, tr["nt_qice"] - 1 + l] = -K["rhoi"] * (K["cp_ice"] * (2.0 + 18.0 * h(f"tq{l}", (nb, ncat, ny, nx))) + 0.9 * K["Lfresh"])
    trcrn[:, :, tr["nt_qsno"] - 1] = -K["rhos"] * (K["Lfresh"] + K["cp_ice"] * (0.1 + 39.9 * h("tqs", (nb, ncat, ny, nx))))
    for k in ("nt_alvl", "nt_apnd", "nt_fbri", "nt_vlvl", "nt_hpnd"):
        nt = tr.get(k, 0)
        if nt:
            f = h("t" + k, (nb, ncat, ny, nx))
            f[h("t0" + k, (nb, ncat, ny, nx)) < 0.1] = 0.0
            trcrn[:, :, nt - 1] = f
    kinds = np.full((nb, ny, nx), -1, dtype=np.int64)
    if not quiet:
        u = h("kind", (nb, ny, nx))
        sel = ice & (u < 0.45)
        kinds[sel] = (u[sel] / 0.45 * len(KINDS)).astype(np.int64)
        noshift = np.array([(b % 3 == 0) and nb > 1 for b in range(nb)])
        kinds[noshift[:, None, None] & (kinds >= 0) & (kinds <= 5)] = -1
    cat = (h("kcat", (nb, ny, nx)) * 1000).astype(np.int64)
    for b, j, i in zip(*np.nonzero(kinds >= 0)):
        kd = KINDS[kinds[b, j, i]]
        a, v, s, t = aicen[b, :, j, i], vicen[b, :, j, i], vsnon[b, :, j, i], trcrn[b, :, :, j, i]
        c = cat[b, j, i]
        if kd in ("up", "up2"):
            n = c % (ncat - 1) if kd == "up" else c % max(ncat - 2, 1)
            a[n] = max(a[n], 0.01)
            v[n] = a[n] * hin[n + 1] * 1.3
            if kd == "up2" and n + 2 < ncat:
                a[n + 1] = 0.0; v[n + 1] = 0.0; s[n + 1] = 0.0
                v[n] = a[n] * hin[n + 2] * 1.1
        elif kd in ("down", "down2"):
            n = 1 + c % (ncat - 1) if kd == "down" else 2 + c % max(ncat - 2, 1)
            n = min(n, ncat - 1)
            a[n] = max(a[n], 0.01)
            v[n] = a[n] * max(hin[n], 0.2) * 0.7
            if kd == "down2" and n >= 2:
                a[n - 1] = 0.0; v[n - 1] = 0.0; s[n - 1] = 0.0
                v[n] = a[n] * max(hin[n - 1], 0.2) * 0.6
        elif kd in ("edge_up", "edge_down"):          # a thickness exactly on a boundary (2 ** -6 * hin is exact, and so is the quotient)
            n = c % (ncat - 1) if kd == "edge_up" else 1 + c % (ncat - 1)
            a[n] = 2.0 ** -6
            v[n] = a[n] * (hin[n + 1] if kd == "edge_up" else hin[n])
        elif kd == "thin1":
            a[0] = max(a[0], 0.01)
            v[0] = a[0] * 0.04
        elif kd in ("tiny+", "tiny-"):
            n = c % ncat
            a[n] = 0.5e-11 if kd == "tiny+" else -0.5e-11
            v[n] = 0.3e-11; s[n] = 0.1e-11
        elif kd == "over":
            a[a == 0.0] = 0.01
            a *= 1.0 / a.sum()
            for _ in range(8):
                tot = 0.0
                for n in range(ncat):
                    tot = tot + a[n]
                if 1.0 < tot < 1.0 + PUNY and abs(tot - (1.0 + 4e-12)) < 2e-12:
                    break
                a[ncat - 1] += (1.0 + 4.0e-12) - tot
            v[:] = a * hi[b, :, j, i]
        elif kd in ("cold", "warm", "thinsnow"):
            n = int(np.argmax(a))
            s[n] = a[n] * (0.5e-4 if kd == "thinsnow" else 0.2)
            t[n, tr["nt_qsno"] - 1] = -K["rhos"] * (K["Lfresh"] + K["cp_ice"] * 150.0) if kd == "cold" else -K["rhos"] * K["Lfresh"] * 0.9
    # ice-free cells: an empty state; one in seven keeps tracer values
    free = ~ice
    keep = free & ocean & (h("keep", (nb, ny, nx)) < 0.15)
    for arr in (aicen, vicen, vsnon):
        np.moveaxis(arr, 1, -1)[free] = 0.0
    np.moveaxis(trcrn.reshape(nb, ncat * ntrcr, ny, nx), 1, -1)[free & ~keep] = 0.0
    empty = (aicen == 0.0)                                                     # a category without ice: no volume; most have no tracers
    vicen[empty] = 0.0
    vsnon[empty] = 0.0
    wipe = empty & ~keep[:, None] & (h("wipe", (nb, ncat, ny, nx)) < 0.8)
    np.moveaxis(trcrn, 2, -1)[wipe] = 0.0
    c_ = np.ascontiguousarray
    aice0 = h("aice0", (nb, ny, nx)) - 0.5                                    # overwritten by the call on every cell
    aice = h("aice", (nb, ny, nx)) - 0.5
    out = dict(d=d, cfg=cfg, bcase=bcase, tmask=tm, phys=phys, ocean=ocean, kinds=kinds, ncat=ncat, ntrcr=ntrcr,
               trcr_depend=np.array(dep, dtype=np.int32), tracers=dict(tr), hin_max=hin, dt=DT, k=dict(K),
               aicen=c_(aicen), vicen=c_(vicen), vsnon=c_(vsnon), trcrn=c_(trcrn), aice0=c_(aice0), aice=c_(aice),
               first_ice=np.zeros((nb, ncat, ny, nx), dtype=np.int32))
    for k in FLUX + TEND:
        out[k] = c_(h("f" + k, (nb, ny, nx)) - 0.5)
    return out


# stop records (g26x18_b8x5, "plain", cyclic_open): cells overwritten in blocks 6 and 11 (1-based), two cells in the lower block so that
# "first" and "last" differ.  cells: (block, i, j) 1-based block indices, all physical ocean cells.
#   bounds      aice = 1.3 in three cells: the loop at :1648-1655 does not exit, the LAST one in (j, i) order is reported          reason 1
#   neg_dvice   a negative volume under an area > puny in category 3: a donor on the downward pass at boundary 2, shift_ice's
#               error loop does not exit either                                                                                   reason 3
#   neg_aicen   an area of -1e-9: zap_small_areas returns at the FIRST one in (n, j, i) order                                      reason 6
STOPS = {"bounds": dict(reason=1, cells=[(6, 3, 2), (6, 5, 4), (6, 2, 4), (11, 4, 3)], expect=(6, 5, 4)),
         "neg_dvice": dict(reason=3, cells=[(6, 3, 2), (6, 5, 4), (6, 2, 4), (11, 4, 3)], expect=(6, 5, 4)),
         "neg_aicen": dict(reason=6, cells=[(6, 5, 4), (6, 3, 2), (6, 2, 4), (11, 4, 3)], expect=(6, 2, 4))}


def stop_input(name):
    x = itd_input("g26x18_b8x5", "plain", tag="stop")
    sp = STOPS[name]
    for q, (b, i, j) in enumerate(sp["cells"]):
        assert x["ocean"][b - 1, j - 1, i - 1], (name, b, i, j)
        for k in ("aicen", "vicen", "vsnon"):
            x[k][b - 1, :, j - 1, i - 1] = 0.0
        a, v = x["aicen"][b - 1, :, j - 1, i - 1], x["vicen"][b - 1, :, j - 1, i - 1]
        if name == "bounds":
            a[1] = 1.3; v[1] = 1.3
        elif name == "neg_dvice":
            a[2] = 0.2; v[2] = -0.1
        else:                      # the first cell in (n, j, i) order is not the first in (j, i) order: category 2 at (2, 4), category 4 before it in the list
            n = 1 if (i, j) == (2, 4) else 3
            a[n] = -1.0e-9; v[n] = 1.0e-9
            a[0] = 0.3; v[0] = 0.09                 # (the cell's total area stays within bounds)
    return x
