"""Which instance of the one-workgroup exact-order solver a plane selects (csrc/sor.hip: tiny_shape, k_sor_tiny<C, NW>), asked
of the library itself through the host-only papof_sor_tiny_shape -- no device, no restatement of the heuristic here.  Every
plane of at most kTinyMaxCells cells is enumerated: the instances that are compiled and dispatched must be exactly the ones
some plane selects, and the planes the GPU tests rely on must select the instance they are listed under."""
import ctypes
import os
import re

import pytest

from _sor_shapes import NOT_TINY, TINY_MAX_CELLS, TINY_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from papteam_opticalflow_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    capi.load()
    return capi


def _instances():
    """{C: NW} of the instances csrc/sor.hip compiles: the one list both tiny_shape's candidates and sor_tiny_solve's dispatch
    are expanded from, and every k_sor_tiny<C, NW> the file names otherwise"""
    text = open(os.path.join(ROOT, "papteam_opticalflow_amd", "csrc", "sor.hip")).read()
    lists = re.findall(r"^#define PAPOF_TINY_SHAPES\(X\)(.*)$", text, re.M)
    assert len(lists) == 1, "one list of instances expected"
    inst = [(int(c), int(nw)) for c, nw in re.findall(r"X\((\d+),\s*(\d+)\)", lists[0])]
    assert inst and len(dict(inst)) == len(inst)
    # both users expand the list and nothing launches an instance beside it
    assert len(re.findall(r"PAPOF_TINY_SHAPES\(PAPOF_TINY_\w+\)", text)) == 2
    assert not re.findall(r"k_sor_tiny<\s*\d", text) and not re.findall(r"PAPOF_TINY\(\s*\d", text)
    return dict(inst)


@pytest.fixture(scope="module")
def chosen(capi):
    """{(H, W): (C, waves)} for every plane of at most kTinyMaxCells cells, (0, 0) where no instance holds it"""
    L = capi.load()
    c, nw = ctypes.c_int(0), ctypes.c_int(0)
    out = {}
    for h in range(1, TINY_MAX_CELLS + 1):
        for w in range(1, TINY_MAX_CELLS // h + 1):
            assert L.papof_sor_tiny_shape(h, w, ctypes.byref(c), ctypes.byref(nw)) == 0
            out[(h, w)] = (c.value, nw.value)
    return out


def test_every_compiled_instance_is_selected_by_some_plane(chosen):
    inst = _instances()
    reached = {}
    for (h, w), (c, nw) in chosen.items():
        if c:
            reached.setdefault(c, []).append(nw)
        else:
            assert nw == 0, (h, w)
    assert set(reached) == set(inst), "instances compiled: %s, selected by a plane: %s" % (sorted(inst), sorted(reached))
    for c, waves in reached.items():  # a launch never has more waves than the instance's register budget allows
        assert 1 <= min(waves) and max(waves) == inst[c], (c, min(waves), max(waves), inst[c])
    print("planes per instance:", {c: len(v) for c, v in sorted(reached.items())},
          "none:", sum(1 for v in chosen.values() if not v[0]))


def test_planes_past_each_limit_are_left_to_the_hyperplane_kernels(capi, chosen):
    for hw in NOT_TINY:
        assert chosen[hw] == (0, 0), hw
    for hw in [(1, 8193), (8193, 1), (3, 2731), (2731, 3), (91, 91), (1080, 1920)]:  # more cells than kTinyMaxCells
        assert hw[0] * hw[1] > TINY_MAX_CELLS and capi.sor_tiny_shape(*hw) == (0, 0), hw
    # ... and each of them is ONE row or column past a plane that is
    assert chosen[(1, 3192)][0] and chosen[(798, 3)][0] and chosen[(4, 1536)][0] and chosen[(198, 23)][0]


@pytest.mark.parametrize("c,hw,waves,what", TINY_SHAPES)
def test_listed_plane_selects_its_instance(chosen, c, hw, waves, what):
    assert chosen[hw] == (c, waves), (hw, what)


def test_the_list_covers_every_instance():
    assert {c for c, _, _, _ in TINY_SHAPES} == set(_instances())
    assert len({hw for _, hw, _, _ in TINY_SHAPES}) == len(TINY_SHAPES)
    inst = _instances()
    for c in inst:  # a full workgroup of every instance is among them
        assert any(cc == c and waves == inst[c] for cc, _, waves, _ in TINY_SHAPES), c


def test_query_refuses_bad_arguments(capi):
    L = capi.load()
    c, nw = ctypes.c_int(7), ctypes.c_int(7)
    for h, w in [(0, 5), (5, 0), (-1, 3), (3, -1)]:
        assert L.papof_sor_tiny_shape(h, w, ctypes.byref(c), ctypes.byref(nw)) != 0
    assert L.papof_sor_tiny_shape(4, 4, None, ctypes.byref(nw)) != 0
    assert L.papof_sor_tiny_shape(4, 4, ctypes.byref(c), None) != 0
    assert L.papof_sor_tiny_shape(1 << 20, 1 << 20, ctypes.byref(c), ctypes.byref(nw)) == 0  # no overflow: not tiny
    assert (c.value, nw.value) == (0, 0)
