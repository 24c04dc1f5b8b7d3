"""Deterministic inputs of the shortwave tests (tests/nprad.py, evpk_step_radiation, evpk_prep_radiation): the grids, masks, tracer tables
and state of tests/golden/therm1svec.py (no shape larger than 26 x 18 cells; the second block of each grid is ice-free), so that the result
can go straight on into step_therm1, with the tables "plain" (nilyr 4, nslyr 1) and "deep" (7, 2) and a forcing of their own:
  sw*            night (all four zero) under therm1vec's winter, humid, hotocean and steady forcing, lit (20 .. 150 W m-2 in all, split
                 over the four bands with a draw per band) under summer, spring and dry
  ocn_albedo2D   0.06 + 0.002 per row: it varies with the row
  Tsfc           therm1vec's, on both sides of -1 C (fT = 0 and fT < 0); every second "thin" column (3 cm of bare ice) gets Tsfc = 0: thin,
                 warm, bare ice, whose near-infrared albedo falls below the ocean's, so that the max against the ocean albedo is taken
  hs, hi         therm1vec's: bare and snow-covered categories, hi below ahmax (fh < 1) and well above it (fh capped at 1)
and for evpk_prep_radiation on its own:
  sw2*           the four sw* times a draw of 0.5 .. 1.5 per band and cell (the changed forcing)
  sf_tiny        cells whose scale_factor of entry is replaced by 5e-12 (0 < scale_factor <= puny)
aice is therm1vec's sum of aicen: zero in the ice-free block and on open water.
"""
from __future__ import annotations

import numpy as np

from . import therm1svec
from .refvec import hash01, seed_of

CONFIGS = therm1svec.CONFIGS
PUNY = therm1svec.PUNY
TABLES = ["plain", "deep"]
SCALARS = dict(albicev=0.78, albicei=0.36, albsnowv=0.98, albsnowi=0.70, ahmax=0.3, snowpatch=0.02, albocn=0.06,
               awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282, awtidf=0.36218)
STATE = ["aicen", "vicen", "vsnon", "trcrn"]
FORCING = ["swvdr", "swvdf", "swidr", "swidf", "ocn_albedo2D"]
OUT3D = ["alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun"]
OUT_LAYERS = ["Sswabsn", "Iswabsn", "fswpenln"]
OUT2D = ["coszen", "alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "scale_factor"]
WRITTEN = OUT3D + OUT_LAYERS + OUT2D
RADIATION = ["fswsfcn", "fswintn", "fswthrun", "fswpenln", "Sswabsn", "Iswabsn"]      # what prep_radiation rescales
LIT = ("summer", "spring", "dry")
BANDS = dict(swvdr=0.28, swvdf=0.24, swidr=0.31, swidf=0.17)


def rad_input(cfg, tcase, ncat=5):
    """dict of the arrays and scalars of one evpk_step_radiation call on every block (therm1svec's input with the forcing above; the
    outputs are pre-filled with non-zero values, since the call overwrites every cell)"""
    x = therm1svec.therm1s_input(cfg, tcase, ncat=ncat)
    d, tr = x["d"], x["tracers"]
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    nilyr, nslyr = tr["nilyr"], tr["nslyr"]
    s2, s3 = (nb, ny, nx), (nb, ncat, ny, nx)
    h = lambda q, shape: hash01(shape, seed_of(cfg, "rad", tcase, str(ncat), q))
    lit = np.isin(x["forcing_kinds"], LIT)
    total = np.where(lit, 20.0 + 130.0 * h("sw", s2), 0.0)
    for q, w in BANDS.items():
        x[q] = total * w * (0.8 + 0.4 * h(q, s2))
        x[q[:2] + "2" + q[2:]] = x[q] * (0.5 + h("2" + q, s2))
    x["ocn_albedo2D"] = np.broadcast_to(0.06 + 0.002 * np.arange(ny)[None, :, None], s2).copy()
    thin = (x["state_kinds"] == "thin") & (h("thinwarm", s3) < 0.5)
    t = x["trcrn"]
    t[:, :, tr["nt_Tsfc"] - 1][thin] = 0.0
    x["thin_warm"] = thin
    for q in OUT3D:
        x[q] = h("o" + q, s3) - 0.5
    x["Sswabsn"] = h("oS", (nb, ncat, nslyr, ny, nx)) - 0.5
    x["Iswabsn"] = h("oI", (nb, ncat, nilyr, ny, nx)) - 0.5
    x["fswpenln"] = h("oP", (nb, ncat, nilyr + 1, ny, nx)) - 0.5
    for q in OUT2D + ["fswfac"]:
        x[q] = h("o" + q, s2) - 0.5
    x["sf_tiny"] = x["ocean"] & (x["aice"] > 0.0) & (h("sftiny", s2) < 0.12)
    x.update(SCALARS)
    for q in STATE + FORCING + WRITTEN + ["fswfac", "aice"] + [k[:2] + "2" + k[2:] for k in BANDS]:
        x[q] = np.ascontiguousarray(x[q], dtype=np.float64)
    return x
