"""The 28 wave sums of k_lm_solve as one reduce-scatter (lmono_amd/csrc/wave_sum28.hpp), host build of the same header over 64
modelled lanes, against the butterfly it replaced (tests/wave_sum28_check.cpp says what is swept): all 28 slots bit for bit on random
doubles, on cancelling inputs where the pairing order shows, on denormals, infinities and a NaN lane; and the check has teeth -- the
reverse mask order differs from the butterfly on the cancelling inputs.

The second test builds the same program with the address and undefined-behaviour sanitizers: a stand-alone host program."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "wave_sum28_check.cpp")
LAST = r"checked=(\d+) cancelling=(\d+) special=(\d+) reverse_differs=(\d+) wrong=0"


def _run(exe):
    res = subprocess.run([exe], text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(res.stdout[-4000:])
    m = re.fullmatch(LAST, res.stdout.strip().splitlines()[-1])
    assert m, res.stdout[-4000:]
    assert res.returncode == 0
    return [int(v) for v in m.groups()]


def test_scatter_equals_the_butterfly_bit_by_bit(tmp_path):
    exe = str(tmp_path / "wave_sum28_check")
    # -ffp-contract=off: nothing to contract here, but the device code this models is compiled so
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", SRC, "-o", exe])
    checked, cancelling, special, reverse_differs = _run(exe)
    assert cancelling == 64 * 63 and special == 200
    assert checked == (2000 + cancelling + special) * 56          # 28 slots, both lanes that hold each
    # teeth: 1e300 and -1e300 meet at the first stage where their lanes' numbers differ in that stage's mask only below it; the reverse
    # order meets them at another stage for every pair of lanes but those that differ in one bit alone (6 x 64 ordered pairs), and the
    # 1.0s absorbed before or after the cancellation then differ
    assert reverse_differs > cancelling // 2


def test_scatter_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "wave_sum28_check_san")
    cc = subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                        text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert cc.returncode == 0, cc.stdout[-4000:]
    _run(exe)
