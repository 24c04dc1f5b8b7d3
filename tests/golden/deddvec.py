"""Deterministic inputs of the Delta-Eddington shortwave tests (tests/npdedd.py, evpk_step_radiation_dedd): the grids, masks, state and
forcing of tests/golden/radvec.py (no shape larger than 26 x 18 cells; two blocks at least, the second ice-free) with the tables "plain"
(nilyr 4, nslyr 1) and "deep" (7, 2), two further tracer planes behind the table's own -- apnd and hpnd, which the tr_pond_cesm variant
names as nt_apnd, nt_hpnd and the variant without a pond tracer leaves beyond ntrcr -- and draws of their own:
  coszen   per ocean cell: 0.05 .. 0.95 (above 0.01); 1e-6 .. 0.009 (between puny and 0.01); -0.3 .. 0 (sun below the horizon under a
           forcing that is still lit: max(puny, coszen) is stored); 0 on land, as compute_coszen leaves it
  sw*      radvec's: night under winter, humid, hotocean and steady forcing, lit otherwise; one lit cell in ten has swidr = swidf = 0
           (fnidr = 0 on a lit cell)
  vsnon    per category with ice: bare; 0.05 mm (below hs_min); 1 .. 29 mm (hs_min <= hs < hs0: fs < 1, all three surface types where a pond
           lies beside it); 5 .. 40 cm (hs >= hs0: fs = 1, fi <= 0; ks of band 3 is of order 1e3 per metre, so these columns reach the trmin
           cut-off and both exp_min clamps by themselves), capped as therm1vec caps its deep snow
  Tsfc     one category in five: -1.5 .. 0 C (0 < fT <= 1 on dT_mlt = 1.5); the rest radvec's (0 C, or cold: fT = 0)
  apnd     none; or 0.1 .. 0.5 of the category with hpnd 1 .. 4 mm (below hpmin), 1 .. 19 cm (the transition to bare ice) or 25 .. 60 cm
The outputs are pre-filled with non-zero draws.
"""
from __future__ import annotations

import numpy as np

from . import radvec
from .refvec import hash01, seed_of

CONFIGS = radvec.CONFIGS
PUNY = radvec.PUNY
TABLES = radvec.TABLES
PONDS = ["cesm", "none"]
NAMELIST = dict(R_ice=0.0, R_pnd=0.0, R_snw=1.5, dT_mlt=1.5, rsnw_mlt=1500.0, kalg=0.60, hs0=0.03, pndaspect=0.8,
                awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282, awtidf=0.36218)          # source/ice_init.F90:289-304, :318-321
STATE = ["aicen", "vicen", "vsnon", "trcrn"]
FORCING = ["swvdr", "swvdf", "swidr", "swidf"]
OUT3D = radvec.OUT3D + ["albpndn", "apeffn", "snowfracn"]
OUT_LAYERS = radvec.OUT_LAYERS
OUT2D = [q for q in radvec.OUT2D if q != "coszen"] + ["albpnd", "apeff_ai"]
WRITTEN = OUT3D + OUT_LAYERS + OUT2D
SNOW = [("bare", 0.25), ("thinsnow", 0.1), ("mid", 0.3), ("deep", 0.35)]
POND = [("none", 0.3), ("shallow", 0.2), ("trans", 0.25), ("deep", 0.25)]
SUN = [("high", 0.6), ("low", 0.2), ("below", 0.2)]


def _kind(u, kinds):
    edges = np.cumsum([w for _, w in kinds])
    idx = np.minimum(np.searchsorted(edges, u * edges[-1], side="right"), len(kinds) - 1)
    return np.array([k for k, _ in kinds], dtype=object)[idx]


def dedd_input(cfg, tcase, pond="cesm", ncat=5):
    """dict of the arrays and scalars of one evpk_step_radiation_dedd call on every block"""
    x = radvec.rad_input(cfg, tcase, ncat=ncat)
    d, tr = x["d"], dict(x["tracers"])
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    s2, s3 = (nb, ny, nx), (nb, ncat, ny, nx)
    h = lambda q, shape: hash01(shape, seed_of(cfg, "dedd", tcase, str(ncat), q))
    ocean = x["ocean"]
    a, v = x["aicen"], x["vicen"]
    ice = a > 0.0
    safe = np.where(ice, a, 1.0)
    hi = v / safe
    # snow
    sk = _kind(h("snowkind", s3), SNOW)
    u = h("hs", s3)
    hs = np.where(sk == "thinsnow", 0.5e-4, np.where(sk == "mid", 0.001 + 0.028 * u, np.where(sk == "deep", 0.05 + 0.35 * u, 0.0)))
    hs = np.minimum(hs, 0.45 * hi + 0.2)
    x["vsnon"] = np.ascontiguousarray(np.where(ice, a * hs, 0.0))
    x["snow_kinds"] = sk
    # Tsfc
    t0 = x["trcrn"]
    ntr0 = t0.shape[2]
    t = np.zeros((nb, ncat, ntr0 + 2, ny, nx))
    t[:, :, :ntr0] = t0
    mid = ice & (h("Tmid", s3) < 0.2)
    Ts = t[:, :, tr["nt_Tsfc"] - 1]
    Ts[mid] = (-1.5 * (0.02 + 0.96 * h("Tsfc", s3)))[mid]
    # ponds: two planes behind the table's own tracers
    pk = _kind(h("pondkind", s3), POND)
    up, uh = h("apnd", s3), h("hpnd", s3)
    apnd = np.where(pk == "none", 0.0, 0.1 + 0.4 * up)
    hpnd = np.where(pk == "shallow", 0.001 + 0.003 * uh, np.where(pk == "trans", 0.01 + 0.18 * uh, np.where(pk == "deep", 0.25 + 0.35 * uh, 0.0)))
    t[:, :, ntr0] = np.where(ice, apnd, 0.0)
    t[:, :, ntr0 + 1] = np.where(ice, hpnd, 0.0)
    x["trcrn"] = np.ascontiguousarray(t)
    x["pond_kinds"] = pk
    tr.update(tr_pond_cesm=0, tr_pond_lvl=0, tr_pond_topo=0)
    if pond == "cesm":
        tr.update(tr_pond_cesm=1, nt_apnd=ntr0 + 1, nt_hpnd=ntr0 + 2)
        x["ntrcr"] = ntr0 + 2
    else:
        tr.update(nt_apnd=0, nt_hpnd=0)
    x["tracers"] = tr
    # the sun
    sun = _kind(h("sunkind", s2), SUN)
    uc = h("coszen", s2)
    cz = np.where(sun == "high", 0.05 + 0.9 * uc, np.where(sun == "low", 1.0e-6 + 0.009 * uc, -0.3 * uc))
    x["coszen"] = np.ascontiguousarray(np.where(ocean, cz, 0.0))
    x["sun_kinds"] = sun
    novis = h("nonir", s2) < 0.1
    for q in ("swidr", "swidf"):
        x[q] = np.ascontiguousarray(np.where(novis, 0.0, x[q]))
    for q in ("albpndn", "apeffn", "snowfracn"):
        x[q] = h("o" + q, s3) - 0.5
    for q in ("albpnd", "apeff_ai"):
        x[q] = h("o" + q, s2) - 0.5
    x.update(NAMELIST)
    for q in STATE + FORCING + WRITTEN + ["coszen"]:
        x[q] = np.ascontiguousarray(x[q], dtype=np.float64)
    return x
