"""evpk_bound_state / evpk_step_dynamics on the host side, no GPU: the header, the ctypes structure and the Fortran bind(C) type agree
member for member; fortran/ice_step_dyn.F90 compiles against the reference's real modules and ice_step_mod.F90 compiles with the lines it
replaces replaced (compile only, as tests/test_ref_interfaces.py; skipped where the reference or the Fortran compiler is absent); the
rule that rebuilds tracer_type / depend / has_dependents from trcr_depend equals the tables the remap tests use.
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from cice5_amd import evpk
from tests import refcompile as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evpk.h")).read(), flags=re.S)


def c_members(hdr, name):
    """member names of `typedef struct { ... } name;` in declaration order"""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + name + r"\s*;", hdr).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.search(r"(\w+)\s*(?:\[\d+\])?$", first.strip()).group(1))
        names += [re.search(r"(\w+)", r).group(1) for r in rest]
    return names


def test_header_declares_the_two_entry_points():
    hdr = header()
    assert re.search(r"#define\s+EVPK_HAS_STEP_DYNAMICS\s+1\b", hdr)
    assert re.search(r"#define\s+EVPK_VERSION\s+6\b", hdr)
    assert re.search(r"int\s+evpk_bound_state\s*\(\s*evpk_ctx\s*\*c,\s*int32_t ncat,\s*int32_t ntrcr,\s*int32_t ntrcr_dim,\s*double \*aicen,"
                     r"\s*double \*vicen,\s*double \*vsnon,\s*double \*trcrn\)", hdr)
    assert re.search(r"int\s+evpk_step_dynamics\s*\(\s*evpk_ctx\s*\*c,\s*const evpk_dyn_args \*a,\s*int32_t stop\[5\]", hdr)
    for n in ("evpk_bound_state", "evpk_step_dynamics"):
        assert n in evpk.EXPORTS and hasattr(ct.CDLL(evpk.LIB_PATH), n)


def test_ctypes_structure_has_the_headers_member_order():
    hdr = header()
    want = c_members(hdr, "evpk_dyn_args")
    assert want[:4] == ["advection", "ridge", "dt", "ndtd"] and want[-1] == "diag" and len(want) == 42
    assert [n for n, _ in evpk.DynArgs._fields_] == want
    assert [n for n, _ in evpk.ItdTracers._fields_] == c_members(hdr, "evpk_itd_tracers")
    assert [n for n, _ in evpk.ItdConstants._fields_] == c_members(hdr, "evpk_itd_constants")
    assert [n for n, _ in evpk.RidgeDiag._fields_] == c_members(hdr, "evpk_ridge_diag")
    # int32 x 2, double, int32 x 4 (+ pad), pointer, 13 + 2 int32 (+ pad), pointer, 7 doubles, 3 int32 (+ pad), 3 pointers, 2 int32, double,
    # 20 pointers
    assert ct.sizeof(evpk.DynArgs) == 8 + 8 + 16 + 8 + 60 + 4 + 8 + 56 + 16 + 24 + 8 + 8 + 8 * 20
    pointers = [n for n, t in evpk.DynArgs._fields_ if t in (evpk.c_f64p, evpk.c_i32p) or n == "diag"]
    assert len(pointers) == 25


def test_fortran_type_has_the_headers_member_order():
    src = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    body = re.search(r"type, bind\(C\) :: evpk_dyn_args\n(.*?)end type evpk_dyn_args", src, flags=re.S).group(1)
    names = []
    for line in body.split("\n"):
        line = line.split("!")[0]
        if "::" in line:
            names += [re.match(r"\s*(\w+)", v).group(1) for v in line.split("::")[1].split(",")]
    assert names == c_members(header(), "evpk_dyn_args")
    for n in ("evpk_bound_state", "evpk_step_dynamics"):
        assert re.search(r"bind\(C, name='" + n + r"'\)", src)


DEPENDS = [[0, 1, 1, 2, 2, 0], [0, 2, 1], [0, 1, 2], []]


def test_tracer_tables_rule_equals_the_tables_of_the_remap_tests():
    """remap_tracer_tables (the default of Context.step_dynamics, and the rule fortran/ice_step_dyn.F90 writes out) against the tables
    tests/golden uses for the remap state cases, and by hand on a table with a tracer of each type"""
    from oracle import orc
    from tests.golden import itdvec, refvec
    cases = DEPENDS + [v[0] for v in refvec.TRACER_CASES.values()] + [v[0] for v in itdvec.TRACER_CASES.values()]
    for dep in cases:
        got, want = evpk.remap_tracer_tables(dep), refvec.remap_tables(np.array(dep, dtype=np.int32))
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w), dep
        for g, w in zip(got, orc.remap_tables(list(dep))):
            assert np.array_equal(g, w), dep
    # Tsfc on the area, qice on the ice volume, alvl on the area, apnd on alvl (tracer 3), hpnd on apnd (tracer 4): types 1, 2, 1, 2, 3
    tt, dp, hd = evpk.remap_tracer_tables([0, 1, 0, 2 + 3, 2 + 4])
    assert list(tt) == [1, 1, 1, 2, 1, 2, 3] and list(dp) == [0, 0, 0, 1, 0, 5, 6] and list(hd) == [1, 0, 0, 0, 1, 1, 0]
    with pytest.raises(evpk.EvpkError, match="must have nt2 > nt1"):
        evpk.remap_tracer_tables([2 + 2, 0])


needs_ref = pytest.mark.skipif(not (os.path.isdir(R.REF) and os.path.exists(R.FC)), reason="needs the reference sources and amdflang")
CALL = "      call evpk_step_dynamics_core (dt, ndtd)\n"


@needs_ref
@pytest.mark.parametrize("extra", [[], ["-DACCESS"]], ids=["AusCOM", "AusCOM+ACCESS"])
def test_ice_step_dyn_compiles_against_the_reference_and_ice_step_mod_with_the_one_call(tmp_path, extra):
    """evpk_mod, our ice_dyn_evp and ice_step_dyn against the reference's ice_state / ice_flux / ice_itd / ice_zbgc_shared /
    ice_transport_driver / ... as they are; then source/ice_step_mod.F90 with :1126-1192 of step_dynamics replaced by the one call (the
    edited text exists in the scratch directory only)"""
    rc = R.RefCompile(str(tmp_path), extra)
    rc.need("ice_dyn_evp", include_top=False)
    rc.compile(os.path.join(ROOT, "fortran", "evpk_mod.F90"), True)
    rc.compile(os.path.join(ROOT, "fortran", "ice_dyn_evp.F90"), True)
    rc.need("ice_step_mod", skip={"ice_dyn_evp"}, include_top=False)
    rc.compile(os.path.join(ROOT, "fortran", "ice_step_dyn.F90"), True)
    assert os.path.exists(os.path.join(rc.mods, "ice_step_dyn.mod"))
    lines = open(os.path.join(R.REF, "source", "ice_step_mod.F90")).read().split("\n")
    a = next(k for k, l in enumerate(lines) if l.strip() == "if (advection == 'upwind') then")
    b = next(k for k, l in enumerate(lines) if k > a and l.strip() == "enddo" and lines[k + 1].strip() == "!$OMP END PARALLEL DO"
             and "ice_timer_stop(timer_column)" in lines[k + 3])
    assert (a + 1, b + 1) == (1126, 1192)
    use = next(k for k, l in enumerate(lines) if k > 1078 and l.strip().startswith("use ice_blocks"))
    assert use + 1 == 1081
    edited = tmp_path / "ice_step_mod_edited.F90"
    edited.write_text("\n".join(lines[:use]) + "\n      use ice_step_dyn, only: evpk_step_dynamics_core\n" + "\n".join(lines[use:a]) + "\n" + CALL +
                      "\n".join(lines[b + 1:]) + "\n")
    rc.compile(str(edited), True)
    assert os.path.exists(os.path.join(rc.mods, "ice_step_mod.mod"))
