"""Deterministic inputs of the linear_itd tests (tests/nplitd.py, evpk_linear_itd): the geometry, land masks and tracer tables of
tests/golden/itdvec.py, its quiet state -- thickness distributions inside their category bounds on 60 % of the ocean cells -- as the state
before the vertical thermodynamics (aicen_init, vicen_init), and seeded growth / melt of vicen on top of it.  Each ice cell draws a kind:
  quiet     vicen = vicen_init: a listed cell that shifts nothing
  tiny      every category grows or melts by a relative 3e-12 .. 3e-10: transfers around puny times the donor (the "very small" resets)
  flagA     category 1 grows beyond hicen_init of category 2:                 remap_flag false, hicen(n) >= hbnew(n)
  flagB     category 1 melts away entirely and category 2 thins below its old thickness:   hicen(n+1) <= hbnew(n)
  flagC     category 1 grows by more than the width of an empty category 2:   hbnew(n) > hin_max(n+1)
  flagD     category 3 melts by more than the width of an empty category 2:   hbnew(n) < hin_max(n-1)
  flat      new ice in an empty category 1, a hair thinner than hin_max(1):   hbnew(1) - hbnew(0) <= puny in fit_line
  whole_da  category 1 near its upper bound grows past it, category 2 empty:  the whole category moves (daice > aicen (1 - puny))
  whole_dv  the same, leaving a sliver of area 1.05e-11 aicen at the thin end: dvice > vicen (1 - puny) while daice is not
  himin     category 1 melts to 0.01 m:                                       the hi_min clamp
  mix       every category's thickness changes by up to +-15 %
Block 1 (0-based) of a grid of several blocks is ice-free (a block without a listed cell) but keeps tracer values; the other blocks mix
the kinds, so transfers up and down occur in the same block.  No shape larger than 26 x 18 cells.
"""
from __future__ import annotations

import numpy as np

from . import itdvec, ridgevec
from .refvec import hash01, seed_of

CONFIGS = {"g26x18_b8x5": ridgevec.CONFIGS["g26x18_b8x5"], "g24x16_b6x4": itdvec.refvec.CONFIGS["g24x16_b6x4"]}
TRACER_CASES = itdvec.TRACER_CASES
HI_MIN = 0.05
PUNY = itdvec.PUNY
KINDS = [("quiet", 0.12), ("tiny", 0.14), ("flagA", 0.04), ("flagB", 0.04), ("flagC", 0.04), ("flagD", 0.04), ("flat", 0.04), ("whole_da", 0.04),
         ("whole_dv", 0.04), ("himin", 0.05), ("mix", 0.41)]
STATE = itdvec.STATE


def _base(cfg, tcase, ncat):
    """itdvec's quiet state on one of CONFIGS (itdvec.CONFIGS has no g24x16_b6x4: the builder is told where the grid is)"""
    if cfg in itdvec.CONFIGS:
        return itdvec.itd_input(cfg, tcase, ncat=ncat, tag="litd", quiet=True)
    saved = dict(itdvec.CONFIGS)
    itdvec.CONFIGS[cfg] = CONFIGS[cfg]
    try:
        return itdvec.itd_input(cfg, tcase, ncat=ncat, tag="litd", quiet=True)
    finally:
        itdvec.CONFIGS.clear()
        itdvec.CONFIGS.update(saved)


def _cell(x, b, j, i, cats):
    """empty the cell, then set the categories of cats: {n (0-based): (aicen_init, hicen_init, aicen, hicen)}"""
    for k in ("aicen_init", "vicen_init", "aicen", "vicen", "vsnon"):
        x[k][b, :, j, i] = 0.0
    for n, (ai, hi, a, h) in cats.items():
        x["aicen_init"][b, n, j, i] = ai
        x["vicen_init"][b, n, j, i] = ai * hi
        x["aicen"][b, n, j, i] = a
        x["vicen"][b, n, j, i] = a * h
        x["vsnon"][b, n, j, i] = a * 0.2


def litd_input(cfg, tcase, ncat=itdvec.NCAT, quiet=False):
    """dict of the arrays of one linear_itd call on every block.  quiet: vicen = vicen_init everywhere."""
    x = _base(cfg, tcase, ncat)
    d = x["d"]
    nb, ny, nx = d.nblocks, d.ny_block, d.nx_block
    h = lambda k, shape: hash01(shape, seed_of(cfg, "litd", tcase, str(ncat), k))
    hin = x["hin_max"]
    x["aicen_init"] = x["aicen"].copy()
    x["vicen_init"] = x["vicen"].copy()
    x["hi_min"] = HI_MIN
    x["fpond"] = np.ascontiguousarray(h("fpond", (nb, ny, nx)) - 0.5)
    ice = x["aicen_init"].sum(axis=1) > 0.0
    kinds = np.full((nb, ny, nx), -1, dtype=np.int64)
    if not quiet:
        u = h("kind", (nb, ny, nx))
        edges = np.cumsum([w for _, w in KINDS])
        kinds[ice] = np.searchsorted(edges, u[ice] * edges[-1], side="right")
        eps = 3.0e-12 * 100.0 ** h("eps", (nb, ny, nx))
        sign = np.where(h("sign", (nb, ny, nx)) < 0.5, -1.0, 1.0)
        fac = 1.0 + 0.3 * (h("mix", (nb, ncat, ny, nx)) - 0.5)
        for b, j, i in zip(*np.nonzero(kinds >= 0)):
            kd = KINDS[kinds[b, j, i]][0]
            if kd == "tiny":
                x["vicen"][b, :, j, i] = x["vicen_init"][b, :, j, i] * (1.0 + sign[b, j, i] * eps[b, j, i])
            elif kd == "mix":
                x["vicen"][b, :, j, i] = x["vicen_init"][b, :, j, i] * fac[b, :, j, i]
            elif kd == "flagA" and ncat >= 2:
                _cell(x, b, j, i, {0: (0.1, 0.4, 0.1, 1.02), 1: (0.1, 1.0, 0.1, 1.0)})
            elif kd == "flagB" and ncat >= 2:
                _cell(x, b, j, i, {0: (0.1, 0.4, 0.0, 0.0), 1: (0.1, 1.0, 0.1, 0.39)})
            elif kd == "flagC" and ncat >= 3:
                _cell(x, b, j, i, {0: (0.1, 0.4, 0.1, 0.4 + 1.1 * (hin[2] - hin[1]))})
            elif kd == "flagD" and ncat >= 3:
                _cell(x, b, j, i, {2: (0.1, hin[2] + 0.3, 0.1, hin[2] + 0.3 - 0.9)})
            elif kd == "flat":
                _cell(x, b, j, i, {0: (0.0, 0.0, 2.0 ** -6, hin[1] - 5.0e-12)})
            elif kd == "whole_da" and ncat >= 2:
                _cell(x, b, j, i, {0: (0.1, 0.6, 0.1, 0.9)})
            elif kd == "whole_dv" and ncat >= 2:
                # fit_line's right case: hL = 3 hicen - 2 hbnew(1) = 3 hicen_init - 2 hin_max(1) + dh; the sliver below hin_max(1) holds
                # (delta / W)^2 of the area, W = hR - hL = 0.12
                delta = 0.12 * np.sqrt(1.05e-11)
                _cell(x, b, j, i, {0: (0.1, 0.6, 0.1, 0.6 + (3.0 * hin[1] - 3.0 * 0.6 - delta))})
            elif kd == "himin":
                _cell(x, b, j, i, {0: (0.1, 0.3, 0.1, 0.01)})
    if nb > 1:                                        # a block without a listed cell; its tracers stay as they are
        for k in ("aicen_init", "vicen_init", "aicen", "vicen", "vsnon"):
            x[k][1] = 0.0
        kinds[1] = -1
    x["kinds"] = kinds
    return x
