"""evpk_thermo_vertical without a GPU: the entry point is declared, exported and bound, and the numpy restatement tests/nptherm1.py -- the
checker of tests/test_therm1_gpu.py -- takes every branch of thermo_vertical's BL99 path on the inputs of tests/golden/therm1vec.py,
converges everywhere, trips no stop, and conserves mass and energy when that is recomputed from the returned arrays alone.

**Parity with the reference is unpinned for all of thermo_vertical**: no reference-built record exists for it.

Counted and printed, not asserted, because no input can reach it:
  tin_reset       the zTin > 0 reset of init_vertical_profile: zTin = min(root, Tmlts) and Tmlts = -depressT zSin <= 0 for every zSin
                  that passes the zSin >= min_salin - puny check before it
  stop reason 4   zTin > Tmlts, for the same reason
  botmelt_snow    bottom melt that goes on into the snow needs every ice layer gone first; the category then melts away, which
                  `vanished` asserts -- whether energy is left over for the snow depends on the draw
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from cice5_amd import evpk
from tests import nptherm1
from tests.golden import itdvec as iv
from tests.golden import therm1vec as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["plain", "topo_ponds", "lvl_ponds", "deep"]
LVAP, FERRMAX = 2.501e6, 1.0e-3


def arrays(x):
    """copies of every array a call may write, and the read-only ones as they are"""
    y = {k: (x[k].copy() if x[k] is not None else None) for k in tv.WRITTEN}
    y.update({k: x[k] for k in tv.IN2D + tv.IN3D})
    return y


def restate(x, conduct=0, iters=None):
    """(arrays, infos, stop) of the restatement on copies"""
    y = arrays(x)
    infos, stop = nptherm1.step(iv.blocks_of(x["d"]), x["tmask"], nptherm1.params(x, conduct), y, iters)
    return y, infos, stop


_cache = {}


def restated(cfg, tcase, ncat=5, conduct=0):
    key = (cfg, tcase, ncat, conduct)
    if key not in _cache:
        x = tv.therm1_input(cfg, tcase, ncat=ncat)
        its = []
        _cache[key] = (x,) + restate(x, conduct, its) + (its,)
    return _cache[key]


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "evpk.h")).read()
    assert re.search(r"^#define EVPK_HAS_THERMO_VERTICAL 1$", hdr, re.M)
    assert re.search(r"^#define EVPK_THERMO_STOP 16$", hdr, re.M)
    assert re.search(r"^#define EVPK_VERSION 6$", hdr, re.M)
    assert re.search(r"^int evpk_thermo_vertical\(evpk_ctx \*c, const evpk_thermo_args \*a, int32_t stop\[5\]", hdr, re.M)
    body = re.search(r"typedef struct \{([^}]*)\} evpk_thermo_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [w.strip().split()[-1].lstrip("*") for part in body.split(";") for w in part.split(",") if w.strip()]
    assert names == [n for n, _ in evpk.ThermoArgs._fields_]                            # the ctypes mirror, member for member
    assert "**Parity is unpinned for all of thermo_vertical**" in hdr
    for word in ("frzmlt_bottom_lateral", "atmo_boundary_layer", "merge_fluxes", "tmask"):
        assert word in hdr[hdr.index("SURVEY S8 row f-10"):hdr.index("#define EVPK_HAS_THERMO_VERTICAL")]


def test_symbol_is_exported_and_bound():
    L = ct.CDLL(evpk.LIB_PATH)
    assert "evpk_thermo_vertical" in evpk.EXPORTS and hasattr(L, "evpk_thermo_vertical")
    assert callable(evpk.Context.thermo_vertical) and evpk.THERMO_STOP == 16
    assert evpk.THERMO_OUT == nptherm1.OUT15 == tv.OUT15 and set(evpk.THERMO_STOP_REASONS) == set(range(1, 8))


def test_fortran_interface():
    src = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    assert "bind(C, name='evpk_thermo_vertical')" in src and "type, bind(C) :: evpk_thermo_args" in src
    assert "EVPK_THERMO_STOP = 16" in src
    body = src[src.index("type, bind(C) :: evpk_thermo_args"):src.index("end type evpk_thermo_args")]
    body = re.sub(r"!.*", "", body)
    names = [re.sub(r"\s*=.*", "", w).strip() for line in body.splitlines()[1:] if "::" in line for w in re.split(r",(?![^(]*\))", line.split("::")[1])]
    assert names == [n for n, _ in evpk.ThermoArgs._fields_]


REPORTED = {"tin_reset", "botmelt_snow"}


@pytest.mark.parametrize("cfg", list(tv.CONFIGS))
def test_inputs_take_every_branch_converge_and_trip_no_stop(cfg):
    """the counts of the restatement's info records, summed over the blocks and the tracer tables of one grid"""
    tot = {k: 0 for k in nptherm1.INFO_KEYS}
    for tcase in TABLES:
        x, y, infos, stop, its = restated(cfg, tcase)
        assert stop is None, (tcase, stop)                      # every listed cell converges, none trips reasons 1 - 7
        listed = int(((x["aicen"] > tv.PUNY) & x["ocean"][:, None]).sum())
        assert len(its) == listed > 300 and max(i[-1] for i in its) < nptherm1.NITERMAX
        for i in infos:
            for k in tot:
                tot[k] += i[k]
        assert any(i["l_snow"] and i["no_snow"] and i["melting_surface"] and i["cond1"] and i["botmelt"] for i in infos), "a block that mixes"
        assert (x["aicen"][1] == 0.0).all() and infos[1]["cells"] == 0, "an ice-free block"
        if x["tracers"].get("tr_pond_topo"):
            assert sum(i["fpond_changed"] for i in infos) > 0
        else:
            assert np.array_equal(y["fpond"], x["fpond"])
        assert (x["fsnow"][x["ocean"]] == 0.0).any() and (x["fsnow"][x["ocean"]] > 0.0).any()
        gone = (x["aicen"] > tv.PUNY) & x["ocean"][:, None] & (y["aicen"] == 0.0)     # melted away: zero state, Tsfc = Tbot
        assert gone.sum() == sum(i["vanished"] for i in infos) > 0
        assert not y["vicen"][gone].any() and not y["vsnon"][gone].any()
        nt = x["tracers"]["nt_Tsfc"] - 1
        assert np.array_equal(y["trcrn"][:, :, nt][gone], np.broadcast_to(x["Tbot"][:, None], gone.shape)[gone])
    print(cfg, tot)
    for k in nptherm1.INFO_KEYS:
        if k not in REPORTED:
            assert tot[k] > 0, k


@pytest.mark.parametrize("cfg", list(tv.CONFIGS))
@pytest.mark.parametrize("tcase", ["plain", "deep"])
def test_mass_and_energy_from_the_returned_arrays(cfg, tcase):
    """from outside the restatement's own code.  Mass: freshn dt against rhoi dhi + rhos dhs with evaporation and snowfall, to puny rhoi.
    Energy: the balance of conservation_check_vthermo (ice_therm_vertical.F90:2359-2363) recomputed from the state of entry, the state
    returned and the returned fluxes, to ferrmax"""
    x, y, infos, stop, its = restated(cfg, tcase)
    k, tr, dt = x["k"], x["tracers"], x["dt"]
    nilyr, nslyr = tr["nilyr"], tr["nslyr"]
    listed = (x["aicen"] > tv.PUNY) & x["ocean"][:, None]
    a = np.where(listed, x["aicen"], 1.0)

    def energy(z, first):
        hi, hs = z["vicen"] / a, z["vsnon"] / a
        e = np.zeros(hi.shape)
        for l in range(nslyr):
            q = z["trcrn"][:, :, tr["nt_qsno"] - 1 + l]
            if first:                                           # the hs_min rule of init_vertical_profile
                q = np.where(hs / nslyr > k["hs_min"] / nslyr, q, -k["rhos"] * k["Lfresh"])
            e = e + hs / nslyr * q
        for l in range(nilyr):
            e = e + hi / nilyr * z["trcrn"][:, :, tr["nt_qice"] - 1 + l]
        return hi, hs, e
    hi0, hs0, e0 = energy(x, True)
    hi1, hs1, e1 = energy(y, False)
    fsnow = x["fsnow"][:, None]
    hsn_new = np.where(fsnow > 0.0, fsnow / k["rhos"] * dt, 0.0)
    mass = np.abs(y["freshn"] * dt - (y["evapn"] * dt - k["rhoi"] * (hi1 - hi0) - k["rhos"] * (hs1 - hs0 - hsn_new)))
    assert mass[listed].max() <= tv.PUNY * k["rhoi"], float(mass[listed].max())
    efinal = e1 - y["evapn"] * dt * LVAP
    einp = (y["fsurfn"] - y["flatn"] + y["fswintn"] - y["fhocnn"] - fsnow * k["Lfresh"]) * dt
    ferr = np.abs(efinal - e0 - einp) / dt
    print(cfg, tcase, "max ferr", float(ferr[listed].max()), "max mass error", float(mass[listed].max()))
    assert ferr[listed].max() <= FERRMAX, float(ferr[listed].max())
    assert (np.abs(y["freshn"][listed]) > 0.0).sum() > 300
    for q in tv.OUT15:                                          # zero wherever the cell is not listed
        assert not y[q][~listed].any(), q


def test_both_conductivities_differ_and_converge():
    x, y0, _, stop0, _ = restated("g26x18_b8x5", "lvl_ponds", conduct=0)
    _, y1, _, stop1, _ = restated("g26x18_b8x5", "lvl_ponds", conduct=1)
    assert stop0 is None and stop1 is None
    assert not np.array_equal(y0["trcrn"], y1["trcrn"]) and not np.array_equal(y0["congeln"], y1["congeln"])


@pytest.mark.parametrize("ncat", [3, 1])
def test_fewer_categories(ncat):
    x, y, infos, stop, its = restated("g26x18_b8x5", "cesm_ponds", ncat=ncat)
    assert stop is None and len(its) > 100


@pytest.mark.parametrize("reason", sorted(tv.STOPS))
def test_restatement_reports_the_first_stop(reason):
    """the crafted value sits in four places chosen so that block, category, row and column each decide once (therm1vec._four_places)"""
    x = tv.stop_input(reason)
    _, _, stop = restate(x)
    P = x["stop_places"]
    assert P[1][:2] == P[0][:2] and P[1][3] > P[0][3] and P[1][2] < P[0][2]              # same category: a later row, a smaller column
    assert P[2][0] == P[0][0] and P[2][1] > P[0][1] and (P[2][3], P[2][2]) < (P[0][3], P[0][2])     # higher category, earlier cell
    assert P[3][0] > P[0][0] and P[3][1] < P[0][1]                                        # higher block, lower category
    assert stop == (reason,) + P[0], (stop, P)


@pytest.mark.parametrize("kind", sorted(tv.MIXED))
def test_restatement_puts_the_check_sequence_before_the_cell(kind):
    x = tv.stop_mixed_input(kind)
    _, _, stop = restate(x)
    assert stop == x["stop_expect"], (stop, x["stop_expect"])
