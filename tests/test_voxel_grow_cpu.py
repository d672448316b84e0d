"""The size arithmetic of a voxel map that grows (lmono_amd/csrc/voxel_grow.hpp through lmono_amd/host/voxel_grow_test) against its
restatement (tests/voxel_grow_ref.py), and the three entry points of a live table in the header, the prototype table and the library."""
import ctypes
import os
import re
import subprocess

import pytest

from tests import voxel_grow_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")
NEW = ["lmono_voxel_map_reserve", "lmono_voxel_map_set_growth", "lmono_voxel_map_capacity"]


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["make", "-s", "-C", HOST, "voxel_grow_test"])
    return os.path.join(HOST, "voxel_grow_test")


def _run(prog, *args):
    out = subprocess.check_output([prog] + [str(a) for a in args], text=True)
    return [[int(v) for v in line.split()] for line in out.strip().split("\n")]


def test_the_restatement_itself():
    assert [G.slots(m) for m in (1, 2, 3, 4, 5, 1 << 30)] == [2, 4, 8, 8, 16, 1 << 31]
    assert G.ladder(3, 20) == [3, 6, 12, 20] and G.ladder(8, 0) == [8] and G.ladder(8, 8) == [8] and G.ladder(2, 8) == [2, 4, 8]
    assert G.capacities(3, 20, [3, 4, 7, 13, 21]) == [3, 6, 12, 20, 20]


def test_slot_counts(prog):
    ms = [1, 2, 3, 4, 5, 6, 7, 8, 9, 1000, 1 << 20, (1 << 20) + 1, (1 << 30) - 1, 1 << 30]
    assert _run(prog, "slots", *ms) == [[m, G.slots(m)] for m in ms]
    for m, s in _run(prog, "slots", *ms):
        assert s >= 2 * m and s & (s - 1) == 0 and (s == 2 or s // 2 < 2 * m)


CASES = {
    "one_step_at_a_time": (3, 20, [1, 3, 4, 6, 7, 12, 13, 20]),
    "limit_no_power_of_two_multiple": (3, 20, [3, 6, 12, 20]),
    "several_doublings_in_one_call": (2, 1 << 12, [700, 701, 4096]),
    "straight_to_the_limit": (1, 1000, [1000]),
    "does_not_fit_at_the_limit": (2, 8, [8, 9, 8]),
    "does_not_fit_from_the_start": (3, 20, [21, 5]),
    "growth_off": (8, 0, [8, 9, 100]),
    "limit_equal_to_the_size": (8, 8, [8, 9]),
    "largest": (1 << 29, 1 << 30, [(1 << 29) + 1, 1 << 30]),
    "empty_calls": (5, 40, [0, 0, 5, 5, 6]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_capacity_after_each_call(prog, case):
    m0, limit, voxels = CASES[case]
    want = G.capacities(m0, limit, voxels)
    assert _run(prog, "grow", m0, limit, *voxels) == [[v, c] for v, c in zip(voxels, want)]
    if case == "limit_no_power_of_two_multiple":
        assert want == [3, 6, 12, 20]
    if case == "several_doublings_in_one_call":
        assert want == [1024, 1024, 4096]
    if case == "does_not_fit_at_the_limit":
        assert want == [8, 8, 8]


def test_bad_arguments_are_refused(prog):
    for args in (["slots", "0"], ["slots", str((1 << 30) + 1)], ["grow", "8", "4", "1"], ["grow", "0", "0", "1"], ["nothing"], []):
        assert subprocess.run([prog] + args, capture_output=True).returncode == 2


def test_the_entry_points_are_declared_listed_and_exported():
    import __graft_entry__ as g
    g.build()
    import lmono_amd
    from lmono_amd import _abi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmono_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(lmono_amd.lib_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in the header"
        assert name in _abi.PROTOTYPES, name + " is not in the prototype table"
        assert hasattr(lib, name), name + " is not exported"
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _abi.PROTOTYPES["lmono_voxel_map_reserve"] == (I, [P, I, P, P])
    assert _abi.PROTOTYPES["lmono_voxel_map_set_growth"] == (I, [P, P, I64])
    assert _abi.PROTOTYPES["lmono_voxel_map_capacity"] == (I, [P, P, P])
