"""The ring / half-sweep decisions of k_ring_tag (lmono_amd/csrc/ring_decide.hpp), host build of the same header, against the exact
decision as the oracle's C restatement evaluates it (tests/ring_decide_check.cpp says what is swept):

- elevation, 16 / 32 / 64 lines, five ranges from 0.6 to 200 m: float by float across three guards on either side of every threshold of
  ring_id (the rounding boundaries, the -8.83 branch switch, the discard limits), the whole interval of the polynomial and beyond it
  strided, z = +-0, denormal and huge z.  Only the threshold at 0 deg (16 and 32 lines), where three guards hold 2e9 floats, is not
  stepped float by float as a whole: every float within 3000 of its centre and of both guard edges, and 20 000 evenly strided ones.
- azimuth, 13 start directions (the axes with both signs of zero, every quadrant, two next to an axis, x0 = y0 = 0), four ranges: the same
  around the thresholds pi and 3 pi / 2 and around 0 and pi / 2, which are none, and 20 000 directions round the circle.
- every input with the reciprocal square root moved by one ulp up and down.

Whenever the fast path answers, the answer is the exact one (wrong = 0); no input farther than two guards from every threshold is handed
to the exact form (far_fallback = 0); x = y = 0 and x x + y y outside [1e-30, 1e30] are handed over."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_ring_and_half_decisions_equal_the_exact_ones(tmp_path):
    exe = str(tmp_path / "ring_decide_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "ring_decide_check.cpp"), "-o", exe])
    res = subprocess.run([exe], text=True, stdout=subprocess.PIPE)
    print(res.stdout)
    last = res.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"ring: checked=(\d+) fast=(\d+) fallback=(\d+) \| half: checked=(\d+) fast=(\d+) fallback=(\d+) \| handed_over=5/5 \| wrong=0 far_fallback=0", last)
    assert m, res.stdout[-4000:]
    assert res.returncode == 0
    # the sweep is no empty one: both paths were taken millions of times for both decisions
    assert all(int(v) > 1000000 for v in m.groups())
