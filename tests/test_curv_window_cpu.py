"""Curvature and gap flags of a sector from a wave's registers (lmono_amd/csrc/curv_window.hpp, what k_select computes in place of
reading k_curvature's arrays): host build of the same header over 64 modelled lanes with 5, 6 and 11 points a lane, against the plain
per-point loop of k_curvature's expressions, bit for bit (tests/curv_window_check.cpp says what is swept): random rings, coordinates
whose partial sums round differently in another order, steps next to the gap threshold, denormals, sector lengths from 1 to 64 M, the
halo at both ends of a ring; and the check has teeth -- the reverse order of summation differs on the cancelling inputs.

The second test builds the same program with the address and undefined-behaviour sanitizers: a stand-alone host program."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "curv_window_check.cpp")
LAST = r"checked=(\d+) sectors=(\d+) cancelling=(\d+) denormal=(\d+) reverse_differs=(\d+) wrong=0"


def _run(exe):
    res = subprocess.run([exe], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(res.stdout[-4000:])
    m = re.fullmatch(LAST, res.stdout.strip().splitlines()[-1])
    assert m, res.stdout[-4000:]
    assert res.returncode == 0
    return [int(v) for v in m.groups()]


def test_window_equals_the_per_point_loop_bit_by_bit(tmp_path):
    exe = str(tmp_path / "curv_window_check")
    # -ffp-contract=off: the device code is compiled so, and a fused multiply-add in dx dx + dy dy would round otherwise
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", SRC, "-o", exe])
    checked, sectors, cancelling, denormal, reverse_differs = _run(exe)
    # 12 sector lengths x 4 placements x 3 widths, 3 + 3 + 1 + 1 sweeps
    assert sectors == 12 * 4 * 3 * 8
    # an element is one curvature and ten gap flags
    assert checked % 11 == 0 and cancelling % 11 == 0 and denormal == cancelling and checked > 8 * cancelling // 2
    # teeth: where 1e8 and -1e8 stand among values of order 1, the sum from the right absorbs other small values than the sum from the
    # left does; a tenth of the elements at least must show it
    assert reverse_differs > cancelling // 11 // 10


def test_window_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "curv_window_check_san")
    cc = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                        text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout[-4000:]
    _run(exe)
