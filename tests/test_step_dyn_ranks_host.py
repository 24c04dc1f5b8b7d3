"""The interface of step_dynamics on x-slab ranks, checked without a GPU: the feature macro, the two evpk_stats members and their
mirrors, and the header's contract for nranks > 1."""
import ctypes as ct
import os
import re

from cice5_amd import evpk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "evpk.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_announces_step_dynamics_on_ranks():
    hdr = _header()
    assert re.search(r"#define\s+EVPK_HAS_STEP_DYNAMICS_RANKS\s+1\b", hdr)
    assert re.search(r"#define\s+EVPK_VERSION\s+6\b", hdr)


def test_stats_end_with_the_bound_state_members():
    names = [n for n, _ in evpk.Stats._fields_]
    assert names[-3:] == ["delivery_bad", "bound_state_rounds", "bound_state_planes"]
    assert [t for _, t in evpk.Stats._fields_[-2:]] == [ct.c_int32, ct.c_int32]
    # the header's struct and the Fortran mirror list the same members in the same order
    body = re.search(r"typedef struct \{([^}]*)\}\s*evpk_stats;", _header()).group(1)
    assert re.findall(r"([A-Za-z_0-9]+)\s*[,;]", body) == names
    f90 = open(os.path.join(ROOT, "fortran", "evpk_mod.F90")).read()
    typ = re.search(r"type, bind\(C\), public :: evpk_stats(.*?)end type evpk_stats", f90, flags=re.S).group(1)
    members = [w.strip() for decl in re.findall(r"::\s*(.*)", typ) for w in decl.split(",")]
    assert members == names
    assert re.search(r"integer \(c_int32_t\) :: bound_state_rounds, bound_state_planes", typ)
    # no offset before them moved: the struct grew by exactly the two members
    assert evpk.Stats.bound_state_rounds.offset == evpk.Stats.delivery_bad.offset + 8
    assert ct.sizeof(evpk.Stats) == evpk.Stats.bound_state_planes.offset + 4


def test_header_states_the_contract_for_more_than_one_rank():
    hdr = _header(comments=True)
    assert not re.search(r"nranks > 1\s*\(follow-ups?\)", hdr)
    assert "follow-up" not in hdr
    assert hdr.count("COLLECTIVE") >= 3                         # evpk_aggregate(bound = 1), evpk_bound_state, evpk_step_dynamics
    assert "still posts every remaining exchange of the call" in hdr
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)                      # (comment lines joined)
    assert flat.count("nranks > 1 on a context that is not connected yet") == 5          # one per entry point
