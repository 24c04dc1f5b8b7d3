"""evpk_step_radiation_dedd without a GPU: the entry point is declared, exported and bound (header, ctypes structure and Fortran type member
by member); the tables the library holds (evpk_dedd_table) equal, bit for bit, the copy typed for the restatement tests/npdedd.py and --
where the reference is present -- the literals of the cited lines; exp_min is the double nearest to e^-10; the array version of dev_exp
equals npridge.dev_exp element for element; and the inputs of tests/golden/deddvec.py take every branch the restatement counts.

Parity with the reference: tests/test_shortwave_ref.py holds the restatement to reference-built records of run_dEdd and below; the call
order and the aggregation lines of coupling_prep stay unpinned.

The spread between the restatement on the port of the device's exp and on libm is printed per array: a record, not
a bound.
"""
import ctypes as ct
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

from cice5_amd import evpk
from tests import npdedd
from tests.golden import deddvec as dv
from tests.golden import itdvec as iv
from tests.npridge import dev_exp
from tests.test_rad_host import _fortran_names, _struct_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/source/ice_shortwave.F90"
CFG = "g26x18_b8x5"
COVERAGE = ["three_types", "fi_nonpos", "hs_lt_hsmin", "hs_mid", "hs_ge_hs0", "hp_lt_hpmin", "hp_trans", "hp_gt_hp0", "trmin_skipped",
            "extins_clamped", "trnlay_clamped", "dfdir_clamped", "dfdif_clamped", "coszen_neg_lit", "coszen_gt_p01", "coszen_small",
            "night_on_ice", "fnidr_zero_lit", "fT_zero", "fT_mid"]
# namelist variant -> the counter it has to raise (and, for the variants that switch a path off, the counter that must then be zero)
VARIANTS = {"rsnw_mlt_3000": (dict(rsnw_mlt=3000.0), "tab_high"), "rsnw_mlt_4": (dict(rsnw_mlt=4.0), "tab_low"),
            "R_snw_2": (dict(R_snw=2.0), "rsnw_nm_fresh"), "R_ice_neg": (dict(R_ice=-1.0), "R_ice_neg"), "R_pnd_neg": (dict(R_pnd=-1.0), "R_pnd_neg"),
            "hs0_0": (dict(hs0=0.0), "hs0_off"), "kalg_0": (dict(kalg=0.0), "kalg_zero")}


def params(x, **kw):
    p = {k: x[k] for k in npdedd.NAMELIST}
    p["tr"] = x["tracers"]
    p["rhos"] = x["k"]["rhos"]
    p.update(kw)
    return p


def arrays(x, penl=True):
    """copies of every array the call writes (coszen included), and the read-only ones as they are"""
    y = {k: x[k].copy() for k in dv.WRITTEN + ["coszen"]}
    y.update({k: x[k] for k in dv.STATE + dv.FORCING})
    if not penl:
        y["fswpenln"] = None
    return y


def restate(x, M=npdedd.PORTS, penl=True, **kw):
    y = arrays(x, penl)
    infos = npdedd.step_radiation_dedd(iv.blocks_of(x["d"]), x["tmask"], params(x, **kw), y, M)
    return y, infos


_cache = {}


def restated(cfg, tcase, pond="cesm", ncat=5, penl=True, **kw):
    """the inputs and the restatement on the ports: computed once per case, shared, not modified"""
    key = (cfg, tcase, pond, ncat, penl) + tuple(sorted(kw.items()))
    if key not in _cache:
        x = dv.dedd_input(cfg, tcase, pond, ncat=ncat)
        _cache[key] = (x,) + restate(x, penl=penl, **kw)
    return _cache[key]


def total(infos):
    return {k: sum(i[k] for i in infos) for k in npdedd.INFO_KEYS}


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "evpk.h")).read()
    assert re.search(r"^#define EVPK_HAS_STEP_RADIATION_DEDD 1$", hdr, re.M)
    assert re.search(r"^#define EVPK_VERSION 6$", hdr, re.M)
    assert re.search(r"^int evpk_step_radiation_dedd\(evpk_ctx \*c, const evpk_dedd_args \*a\);$", hdr, re.M)
    assert re.search(r"^int evpk_dedd_table\(const char \*name, double \*out, int32_t n\);$", hdr, re.M)
    assert _struct_names(hdr, "evpk_dedd_args") == [n for n, _ in evpk.DeddArgs._fields_]          # the ctypes mirror, member for member
    assert dict(evpk.DeddArgs._fields_)["t"] is evpk.ItdTracers
    block = hdr[hdr.index("evpk_step_radiation_dedd: step_radiation"):hdr.index("#define EVPK_HAS_STEP_RADIATION_DEDD")]
    assert "**Parity unpinned**" in block
    for word in ("ice_shortwave.F90:1251-1577", "ice_step_mod.F90:1408-1451", ":3782-3883", ":3893-3958", ":1607-2024", ":2034-3261", ":3270-3772",
                 "CICE_RunMod.F90:503-548", "tmask", "dT_mlt", "0x3F07CD79B5647C9B", "dhsn", "ffracn", "albcnt", "compute_coszen", "zero-layer",
                 "tr_pond_lvl", "tr_pond_topo", "tr_aero"):
        assert word in block, word


def test_symbol_is_exported_and_bound():
    L = ct.CDLL(evpk.LIB_PATH)
    for name in ("evpk_step_radiation_dedd", "evpk_dedd_table"):
        assert name in evpk.EXPORTS and hasattr(L, name)
    assert callable(evpk.Context.step_radiation_dedd)
    assert evpk.DEDD_STATE == dv.STATE and evpk.DEDD_FORCING == dv.FORCING and evpk.DEDD_OUT == dv.OUT3D == npdedd.OUT3D
    assert evpk.DEDD_OUT_LAYERS == dv.OUT_LAYERS == npdedd.OUT_LAYERS and evpk.DEDD_OUT2D == dv.OUT2D == npdedd.OUT2D
    assert evpk.DEDD_SCALARS == npdedd.NAMELIST == list(dv.NAMELIST) and evpk.DEDD_DEFAULTS == dv.NAMELIST


def test_fortran_interface():
    src = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    assert "bind(C, name='evpk_step_radiation_dedd')" in src
    assert _fortran_names(src, "evpk_dedd_args") == [n for n, _ in evpk.DeddArgs._fields_]
    assert "type (evpk_itd_tracers) :: t" in src[src.index("type, bind(C) :: evpk_dedd_args"):src.index("end type evpk_dedd_args")]
    core = open(os.path.join(ROOT, "fortran", "ice_step_dyn.F90")).read()
    assert "subroutine evpk_step_radiation_dedd_core" in core and "subroutine evpk_step_radiation_core" in core


def _own_tables():
    t = dict(rsnw_tab=npdedd.RSNW_TAB, Qs_tab=npdedd.QS_TAB.T.ravel(), ws_tab=npdedd.WS_TAB.T.ravel(), gs_tab=npdedd.GS_TAB.T.ravel(),
             gauspt=np.array(npdedd.GAUSPT), gauswt=np.array(npdedd.GAUSWT), scalars=np.array(npdedd.SCALARS))
    t.update({k: np.array(v) for k, v in npdedd.MEAN.items()})
    return t


def test_tables_equal_the_restatements_copy_bit_for_bit():
    own = _own_tables()
    assert sorted(own) == sorted(evpk.DEDD_TABLES)
    for name, n in evpk.DEDD_TABLES.items():
        got = evpk.dedd_table(name)
        assert got.shape == (n,) == own[name].shape, name
        assert got.tobytes() == np.ascontiguousarray(own[name], dtype=np.float64).tobytes(), name
    assert len(evpk.DEDD_SCALAR_NAMES) == evpk.DEDD_TABLES["scalars"]
    with pytest.raises(evpk.EvpkError):
        evpk.DEDD_TABLES["nosuch"] = 3
        try:
            evpk.dedd_table("nosuch")
        finally:
            del evpk.DEDD_TABLES["nosuch"]
    out = np.zeros(5)
    assert evpk.lib().evpk_dedd_table(b"rsnw_tab", evpk._p64(out), 5) == 1 and not out.any()


def _literals(lines, lo, hi):
    """the numeric literals with a _dbl_kind suffix of lines lo .. hi (1-based, inclusive), in order"""
    text = "".join(lines[lo - 1:hi])
    text = re.sub(r"!.*", "", text)
    return np.array([float(w) for w in re.findall(r"(?<![\w.])((?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)_dbl_kind", text)])


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference is not on this machine")
def test_tables_equal_the_literals_of_the_cited_lines():
    lines = open(REF).readlines()
    T = evpk.dedd_table
    assert np.array_equal(T("rsnw_tab"), _literals(lines, 2368, 2376))
    for name, (lo, hi) in dict(Qs_tab=(2380, 2413), ws_tab=(2417, 2450), gs_tab=(2454, 2487)).items():
        ref = _literals(lines, lo, hi).reshape(32, 3)                       # the band runs fastest in the reference
        assert np.array_equal(T(name).reshape(3, 32), ref.T), name
    for group, (lo, hi) in dict(i_ssl=(2497, 2499), i_dl=(2503, 2505), i_int=(2509, 2511), i_p_ssl=(2515, 2517), i_p_int=(2521, 2523)).items():
        ref = _literals(lines, lo, hi).reshape(3, 3)
        for q, row in zip("kwg", ref):
            assert np.array_equal(T(q + group + "_mn"), row), q + group
    ref = _literals(lines, 2530, 2532).reshape(3, 3)
    for q, row in zip(("kw", "ww", "gw"), ref):
        assert np.array_equal(T(q), row), q
    g = _literals(lines, 3477, 3485)
    assert np.array_equal(T("gauspt"), g[:8]) and np.array_equal(T("gauswt"), g[8:])
    s = dict(zip(evpk.DEDD_SCALAR_NAMES, T("scalars")))
    cited = dict(hi_ssl=(139, 139), hs_ssl=(140, 140), hpmin=(143, 143), hp0=(144, 144), rsnw_fresh=(3832, 3832), rsnw_nonmelt=(3833, 3833),
                 rsnw_sig=(3834, 3834), cp67=(2262, 2262), cp78=(2264, 2264), cp01=(2266, 2266), rhoi=(2535, 2535), fr_max=(2536, 2536),
                 fr_min=(2537, 2537), fp_ice=(2540, 2540), fm_ice=(2541, 2541), fp_pnd=(2542, 2542), fm_pnd=(2543, 2543), trmin=(3397, 3397),
                 refindx=(3431, 3431), cp063=(3432, 3432), cp455=(3433, 3433), ssl_div=(2636, 2636), alg_depth=(2881, 2881))
    for name, (lo, hi) in cited.items():
        assert _literals(lines, lo, hi).tolist() == [s[name]], name
    assert _literals(lines, 3954, 3954).tolist() == [s["pnd_fac"]]
    assert "argmax = c10" in lines[1375] and "exp_min = exp(-argmax)" in lines[1382] and "dT_pnd = c1" in lines[3931]


def test_exp_min_is_the_double_nearest_to_exp_minus_ten():
    getcontext().prec = 80
    e = Decimal(-10).exp()
    s = dict(zip(evpk.DEDD_SCALAR_NAMES, evpk.dedd_table("scalars")))
    f = float(s["exp_min"])
    assert f == npdedd.EXP_MIN == float(e) and f.hex() == "0x1.7cd79b5647c9bp-15"
    lo, hi = float(np.nextafter(f, 0.0)), float(np.nextafter(f, 1.0))
    assert abs(Decimal(f) - e) < abs(Decimal(lo) - e) and abs(Decimal(f) - e) < abs(Decimal(hi) - e)


def test_array_exp_equals_the_scalar_port_element_for_element():
    """a seeded sample over the three range-reduction branches of dev_exp (|x| <= ln2/2, up to 3 ln2/2, beyond), the tiny branch, the
    arguments of the clamps (down to -2000) and the exact branch edges"""
    rng = np.random.default_rng(20)
    x = np.concatenate([rng.uniform(-0.3465, 0.3465, 4000), rng.uniform(-1.0397, -0.3466, 4000), rng.uniform(0.3466, 1.0397, 1000),
                        rng.uniform(-40.0, -1.04, 6000), rng.uniform(1.04, 5.0, 500), rng.uniform(-2000.0, -40.0, 2000),
                        rng.uniform(-3.7e-9, 3.7e-9, 500),
                        np.array([0.0, -0.0, 0.34657359027997264, -0.34657359027997264, 1.0397207708399179, -1.0397207708399179, -10.0, -745.2])])
    got = npdedd.dev_exp_v(x)
    want = np.array([dev_exp(float(v)) for v in x])
    assert got.tobytes() == want.tobytes()
    ax = np.abs(x)
    assert (ax <= 0.34657359027997264).sum() > 1000 and ((ax > 0.34657359027997264) & (ax < 1.0397207708399179)).sum() > 1000
    assert (ax >= 1.0397207708399179).sum() > 1000


@pytest.mark.parametrize("cfg", list(dv.CONFIGS))
def test_inputs_take_every_branch(cfg):
    """the restatement's counters, summed over the blocks, the two tracer tables and the two pond variants of one grid: every item of the
    input list of tests/golden/deddvec.py, each non-zero.  The pond-depth classes count columns with fp > puny on a lit cell"""
    tot = {k: 0 for k in npdedd.INFO_KEYS}
    for tcase in dv.TABLES:
        for pond in dv.PONDS:
            x, y, infos = restated(cfg, tcase, pond)
            listed = int(((x["aicen"] > dv.PUNY) & x["ocean"][:, None]).sum())
            assert sum(i["listed"] for i in infos) == listed > 300
            assert x["aicen"].shape[0] >= 2 and (x["aicen"][1] == 0.0).all() and infos[1]["listed"] == 0, "an ice-free block"
            assert max(x["aicen"].shape[-2:]) <= 26 and min(x["aicen"].shape[-2:]) <= 18
            t = total(infos)
            for k in tot:
                tot[k] += t[k]
            if pond == "none":
                assert t["set_pond"] == listed and t["hp_trans"] == t["hp_gt_hp0"] == t["hp_lt_hpmin"] == 0 and t["three_types"] == 0
                assert (y["apeffn"] > 0.0).any() and not y["albpndn"].any()
            else:
                assert t["set_pond"] == 0 and t["cesm_infiltrated"] > 0 and y["albpndn"].any()
    print(cfg, tot)
    for k in COVERAGE:
        assert tot[k] > 0, k
    assert tot["tab_inside"] > 0 and tot["tab_low"] == tot["tab_high"] == 0 and tot["R_ice_neg"] == tot["R_pnd_neg"] == tot["kalg_zero"] == 0


@pytest.mark.parametrize("name", list(VARIANTS))
def test_namelist_variants_raise_their_own_counter(name):
    kw, counter = VARIANTS[name]
    base = total(restated(CFG, "plain")[2])
    x, y, infos = restated(CFG, "plain", **kw)
    t = total(infos)
    assert base[counter] == 0 and t[counter] > 0, (name, counter, t[counter])
    if name == "hs0_0":
        assert t["hs_mid"] == t["hs_ge_hs0"] == t["cesm_infiltrated"] == 0
    want = restated(CFG, "plain")[1]
    assert any(not np.array_equal(y[k], want[k]) for k in dv.WRITTEN), "the variant changes the result"


@pytest.mark.parametrize("cfg", list(dv.CONFIGS))
@pytest.mark.parametrize("tcase", dv.TABLES)
@pytest.mark.parametrize("pond", dv.PONDS)
def test_zeros_budget_and_sums_from_the_returned_arrays(cfg, tcase, pond):
    """from outside the restatement's own code, on its returned arrays: zero wherever the cell is not listed or not lit; the absorbed
    shortwave equals the incoming one minus the reflected one up to the roundings of some sixty flux differences of magnitude at most S
    (256 * 2^-52 * S); the 2-D sums of coupling_prep; coszen changed on the listed lit cells only"""
    x, y, infos = restated(cfg, tcase, pond)
    ncat = x["aicen"].shape[1]
    listed = (x["aicen"] > dv.PUNY) & x["ocean"][:, None]
    S = x["swvdr"] + x["swvdf"] + x["swidr"] + x["swidf"]
    lit = np.broadcast_to((S > dv.PUNY)[:, None], listed.shape) & listed
    for q in dv.OUT3D:
        off = ~listed if q in ("apeffn", "snowfracn") else ~lit
        assert not y[q][off].any(), q
    for q in dv.OUT_LAYERS:
        assert not y[q][np.broadcast_to(~lit[:, :, None], y[q].shape)].any(), q
    for q in ("alvdrn", "alidrn", "alvdfn", "alidfn"):
        assert (y[q][lit] > 0.0).all() and (y[q][lit] < 1.0).all(), q
    absorbed = (x["swvdr"][:, None] * (1.0 - y["alvdrn"]) + x["swvdf"][:, None] * (1.0 - y["alvdfn"]) + x["swidr"][:, None] * (1.0 - y["alidrn"])
                + x["swidf"][:, None] * (1.0 - y["alidfn"]))
    tot = y["fswsfcn"] + y["fswintn"] + y["fswthrun"]
    err = np.abs(tot - absorbed)[lit] / np.broadcast_to(S[:, None], tot.shape)[lit]
    print(f"  {cfg} {tcase} {pond}: largest budget error / S = {err.max():.3e}")
    assert (err <= 1.0e-9).all()
    assert tot[lit].any() and y["Sswabsn"].any() and y["Iswabsn"].any()
    changed = y["coszen"] != x["coszen"]
    anylit = lit.any(axis=1)
    assert not changed[~anylit].any() and (y["coszen"][anylit] >= dv.PUNY).all() and changed.any()
    sun = y["coszen"] > dv.PUNY
    for m, q, gate in (("alvdr", "alvdrn", False), ("alidr", "alidrn", False), ("alvdf", "alvdfn", False), ("alidf", "alidfn", False),
                       ("apeff_ai", "apeffn", False), ("albice", "albicen", True), ("albsno", "albsnon", True), ("albpnd", "albpndn", True)):
        want = np.zeros(S.shape)
        for n in range(ncat):
            want = np.where(sun | (not gate), want + y[q][:, n] * x["aicen"][:, n], want)
        assert np.array_equal(want, y[m]), m


def test_spread_between_ports_and_libm():
    """a record, not a bound: the largest difference of every output between the two math sets, relative to the
    array's largest magnitude"""
    worst = {}
    for cfg in dv.CONFIGS:
        for tcase in dv.TABLES:
            x, y, _ = restated(cfg, tcase)
            z, _ = restate(x, npdedd.LIBM)
            for k in dv.WRITTEN + ["coszen"]:
                scale = float(np.abs(y[k]).max())
                spread = float(np.abs(y[k] - z[k]).max()) / scale if scale else 0.0
                worst[k] = max(worst.get(k, 0.0), spread)
    for k, v in worst.items():
        print(f"  {k:14s} {v:.3e}")
    print("largest relative spread", max(worst.values()))
    assert all(np.isfinite(v) for v in worst.values())
