"""The sharp picks of k_select settled in parallel rounds (lmono_amd/csrc/sel_rounds.hpp), host build of the same header run lane by lane
as the kernel runs it, against the reference walk (sort by (curvature, index), take the next unsuppressed, mark, stop at 20).
tests/sel_rounds_check.cpp says what is swept: every ordering of up to 8 keys x every gap mask, ties at distances 1 - 6, staircases of
30 - 300 candidates (with their round count), all gaps long, reaches across lane and sector borders, more than 20 and more than 64
members, 20 000 random sectors of up to 704 points.  Built a second time with the host's address and undefined-behaviour sanitizers
(a stand-alone program, a shorter sweep)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST = (r"checked=(\d+) ties=(\d+) staircases=(\d+) fallback=(\d+) filtered=(\d+) over20=(\d+) edge=(\d+) maxrounds=(\d+) hitmask_wrong=0 wrong=0")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sel_rounds")
    src = os.path.join(ROOT, "tests", "sel_rounds_check.cpp")
    # the two builds side by side; the sanitized one runs the short form of the sweep (argument "short": the exhaustive part stops at 6 keys)
    builds = (("plain", ["-O3"], []), ("san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["short"]))
    exe = {name: str(d / ("sel_rounds_check_" + name)) for name, _, _ in builds}
    cc = {name: subprocess.Popen(["g++", "-std=c++17", "-pthread"] + flags + [src, "-o", exe[name]]) for name, flags, _ in builds}
    run = {}
    for name, _, args in builds:
        assert cc[name].wait() == 0
        run[name] = subprocess.Popen([exe[name]] + args, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    res = {}
    for name, p in run.items():
        out = p.communicate()[0]
        res[name] = subprocess.CompletedProcess(p.args, p.returncode, out)
    return res


def test_rounds_equal_the_reference_walk(outputs):
    res = outputs["plain"]
    print(res.stdout)
    m = re.fullmatch(LAST, res.stdout.strip().splitlines()[-1])
    assert m, res.stdout[-4000:]
    assert res.returncode == 0
    checked, ties, stairs, fallback, filtered, over20, edge, maxrounds = (int(v) for v in m.groups())
    # the sweep is no empty one, and every branch was met many times
    assert checked > 5000000
    assert ties > 10000 and stairs == 542 and edge > 10000
    assert fallback > 100 and filtered > 1000 and over20 > 5000
    assert maxrounds == 50                      # the staircase of 300: one member per round, ceil(300 / 6) rounds


def test_rounds_clean_under_address_and_ub_sanitizers(outputs):
    res = outputs["san"]
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-4000:]
    assert re.fullmatch(LAST, res.stdout.strip().splitlines()[-1]), res.stdout[-4000:]
