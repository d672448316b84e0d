"""scripts/pnp_settling.py -- the settling table of DESIGN.md 6g, on the restatement tests/pnp_ref.py (CPU only): the share of 4-point
samples that are valid, and that end within 1 mm of the true translation, after K steps with the first `damp` of them damped by 4^-k.
40 scenes of 150 noise-free points, 256 samples each, the guess displaced by the full 30 degrees and 20 m.

  python scripts/pnp_settling.py [--steps 6,8,10,12,16,20] [--damp 0,4,6,8] [--scenes 40]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def settle(steps, damp, scenes=40):
    """-> (share valid, share valid and within 1 mm), averaged over the scenes."""
    from tests import pnp_cases as S
    from tests import pnp_ref as P
    valid, close = [], []
    for seed in range(scenes):
        p3, p2, g, truth, _ = S.scene(150, seed, 0.0, noise=0.0, angle_deg=30.0, trans=20.0)
        pd = np.concatenate([p3.astype(np.float64), p2.astype(np.float64)], 1)
        idx, _ = P.sample(0, seed, 256, 150)
        t, _, good = P.solve4(pd, idx, g, steps, damp)
        err = np.abs(t - truth[:3]).max(1)
        valid.append(good.mean()); close.append(((err < 1e-3) & good).mean())
    return float(np.mean(valid)), float(np.mean(close))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="6,8,10,12,16,20")
    ap.add_argument("--damp", default="0,4,6,8")
    ap.add_argument("--scenes", type=int, default=40)
    a = ap.parse_args()
    for k in [int(x) for x in a.steps.split(",")]:
        for d in [int(x) for x in a.damp.split(",")]:
            if d <= k:
                print("K %2d damped %d: valid %.3f within 1 mm %.3f" % ((k, d) + settle(k, d, a.scenes)))


if __name__ == "__main__":
    main()
