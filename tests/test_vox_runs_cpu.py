"""Run lengths of k_voxel's segments (lmono_amd/csrc/vox_runs.hpp), host build of the same header, against the walk over the
continuation bitmap one bit after the other that it replaced (tests/vox_runs_check.cpp says what is swept): every head position and
run length over three words and over rings that end next to a word boundary, the runs that end at bits 63, 64, 127 and at the ring's
last point, words of all ones and all zeros, random bitmaps of up to 2304 points.

The kernel's keys carry no run length (the packed form with a "scan the bitmap" escape was not built), so there is no escape to test."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_length_helper_equals_the_walk_bit_by_bit(tmp_path):
    exe = str(tmp_path / "vox_runs_check")
    subprocess.check_call(["g++", "-O2", os.path.join(ROOT, "tests", "vox_runs_check.cpp"), "-o", exe])
    res = subprocess.run([exe], text=True, stdout=subprocess.PIPE)
    print(res.stdout)
    last = res.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"checked=(\d+) ends63=(\d+) ends64=(\d+) ends127=(\d+) endslen=(\d+) wrong=0", last)
    assert m, res.stdout[-4000:]
    assert res.returncode == 0
    checked, e63, e64, e127, elen = (int(v) for v in m.groups())
    # the sweep is no empty one, and the boundary cases were all met many times
    assert checked > 1000000
    assert min(e63, e64, e127, elen) > 1000
