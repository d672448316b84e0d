"""Pose-graph inputs for the tests beyond what workloads/s4.py makes (whose output stays byte-stable), and the expansion of both
reduce-buffer layouts to a dense system in keyframe order.

  small_graph    a few keyframes turning through yaw = +-180 with real pitch / roll, optional loops (one exact, one gross)
  covered        an S4 graph plus three loops measured from its own odometry: inside the Huber radius, one across the yaw seam
  random_loops   S4 keyframes with loops between uniformly random pairs: long-range loops no ordering can shrink -> wide bands
  BANDS          frozen parameters of one random_loops graph per band class of the solver (see the table for what each exercises)

Both layouts store the lower band in elimination (position) order:
  GPU     H [n][w+1][16] (block (p, p - d) row-major) | g [4n] | cost [n]
  oracle  H [4n][4(w+1)] (scalar row i, columns 4 (i/4 - w) ..) | g [4n] | cost [1]"""
import numpy as np

from tests import posegraph_ref as A
from workloads import s4


def _R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def loop_record(poses, i, j, noise_t=(0.0, 0.0, 0.0), noise_yaw_deg=0.0):
    """loop_info row (relative_t, relative_q (w x y z), relative_yaw in [-180, 180)) of keyframe j seen from keyframe i."""
    Ri, Rj = _R(poses[i, 3:]), _R(poses[j, 3:])
    rel_t = Ri.T @ (poses[j, :3] - poses[i, :3]) + np.asarray(noise_t)
    q = s4._quat(Ri.T @ Rj)
    yaw = (s4._yaw_deg(Rj) - s4._yaw_deg(Ri) + noise_yaw_deg + 180.0) % 360.0 - 180.0
    return [rel_t[0], rel_t[1], rel_t[2], q[3], q[0], q[1], q[2], yaw]


def _pack(truth, odom, loops, info):
    return dict(truth=truth, odom=odom, loops=np.array(loops, np.int32).reshape(-1, 2), loop_info=np.array(info, np.float64).reshape(-1, 8))


def small_graph(n, loops=True, seed=0):
    """n keyframes on an arc whose yaw runs 150, 150 + 70 / (n - 1), ... 220 degrees (through the +-180 seam), pitch / roll of
    a few degrees.  With loops: keyframe 0 -> n - 1 measured from the odometry to 1 mm (inside the Huber radius) and
    1 -> n - 1 (0 -> 1 when n = 2) with a 2 m error (outside it)."""
    rng = np.random.default_rng(seed)
    yaw = np.linspace(150.0, 220.0, n)
    truth, odom = np.zeros((n, 7)), np.zeros((n, 7))
    t = np.zeros(3)
    for i in range(n):
        R = s4._rot([yaw[i], 3.0 * np.sin(1.0 + i), -2.0 * np.cos(2.0 + i)])
        if i:
            t = t + R @ np.array([1.5, 0.0, 0.05])
        truth[i, :3] = t; truth[i, 3:] = s4._quat(R)
        Ro = s4._rot([yaw[i] + (rng.normal(0, 0.3) if i else 0.0), 3.0 * np.sin(1.0 + i), -2.0 * np.cos(2.0 + i)])
        odom[i, :3] = t + (rng.normal(0, 0.03, 3) if i else 0.0); odom[i, 3:] = s4._quat(Ro)
    lp, info = [], []
    if loops:
        k = 1 if n > 2 else 0
        lp = [(0, n - 1), (k, n - 1)]
        info = [loop_record(odom, 0, n - 1, noise_t=(0.001, -0.001, 0.0005), noise_yaw_deg=0.01),
                loop_record(odom, k, n - 1, noise_t=(2.0, 0.0, 0.0))]
        if n >= 5:                                           # a loop that does not touch the fixed keyframe
            lp.append((1, n - 2)); info.append(loop_record(truth, 1, n - 2, noise_t=(0.01, 0.0, 0.0)))
    return _pack(truth, odom, lp, info)


def covered(g):
    """g plus three loops measured from g's own odometry (1 mm, 0.01 degree off), so that they lie inside the Huber radius: two
    long ones, and one over the first five keyframes whose odometry yaw jumps across the +-180 seam (there yaw_b - yaw_a -
    relative_yaw = +-360 and NormalizeAngle acts)."""
    n = len(g["odom"])
    yaw = np.array([s4._yaw_deg(_R(q)) for q in g["odom"][:, 3:]])
    seam = int(np.nonzero(np.abs(yaw[5:] - yaw[:-5]) > 180.0)[0][0])
    extra = [(n // 7, n // 2), (n // 3 + 1, n - 3), (seam, seam + 5)]
    info = [loop_record(g["odom"], i, j, noise_t=(0.001, 0.002, -0.001), noise_yaw_deg=0.01) for i, j in extra]
    return dict(truth=g["truth"], odom=g["odom"], loops=np.concatenate([g["loops"].reshape(-1, 2), np.array(extra, np.int32)]),
                loop_info=np.concatenate([g["loop_info"].reshape(-1, 8), np.array(info)]))


def random_loops(n, n_loops, seed, keep=None, noise_t=0.02, noise_yaw_deg=0.05):
    """S4 keyframes (two laps of the figure 8, drifting odometry) with n_loops loops between uniformly random pairs at least 5
    apart, measured from the truth plus noise; keep: only the first `keep` of them (the pairs and their noise do not depend on it)."""
    base = s4.make_graph(n=n, loop_gap=n, seed=seed)          # loop_gap = n: no revisit loops
    rng = np.random.default_rng(1000 + seed)
    lp, info = [], []
    while len(lp) < n_loops:
        i, j = sorted(int(v) for v in rng.integers(0, n, 2))
        nt, ny = rng.normal(0, noise_t, 3), rng.normal(0, noise_yaw_deg)
        if j - i < 5:
            continue
        lp.append((i, j)); info.append(loop_record(base["truth"], i, j, noise_t=nt, noise_yaw_deg=ny))
    keep = n_loops if keep is None else keep
    return _pack(base["truth"], base["odom"], lp[:keep], info[:keep])


# The CPU-pinned graphs of the linearisation tests: n = 2, 6, 120 and 300 with outliers.
LINEARISATION_GRAPHS = {
    "n2": lambda: small_graph(2, seed=1),
    "n6": lambda: small_graph(6, seed=2),
    "n120": lambda: covered(s4.make_graph(n=120, loop_gap=30, seed=3)),
    "n300_outliers": lambda: covered(s4.make_graph(n=300, outliers=3)),
}

def assert_coverage(ref):
    """What a graph of the linearisation tests must contain at its starting point, or the comparison proves less than it says."""
    s = A.squared_norms(ref, ref.x0)[ref.loop]
    assert (s > 0.01).any() and (s <= 0.01).any(), "needs a loop edge outside and one inside the Huber radius"
    assert (np.abs(A.raw_yaw_difference(ref, ref.x0)) > 180.0).any(), "needs an edge on which NormalizeAngle acts"
    assert max(np.abs(ref.pitch).max(), np.abs(ref.roll).max()) > 0.1, "needs a real pitch or roll"


# One graph per band class, found by a deterministic search over (seed, loop count, loops dropped from the end) with the
# oracle's bandwidth: name -> (n, n_loops, seed, keep, lowest w, highest w, panel width).  n % panel width is part of the case.
BANDS = {
    "w8_last": (601, 400, 0, 57, 113, 120, 8),            # w = 113: the last width-8 bands, n % 8 = 1
    "w4_first": (601, 400, 0, 64, 121, 128, 4),           # w = 128: the first width-4 bands, n % 4 = 1
    "w4_widest": (603, 400, 0, 253, 240, 255, 4),         # w = 255: the widest band the solver takes, n % 4 = 3
    "refused": (603, 400, 0, 400, 256, 10 ** 9, 4),       # w = 299: refused at create
}


def search_band(oracle, n, lo, hi, n_loops=400, seeds=range(8)):
    """How BANDS was found: the first (seed, keep) in that order, keep falling from n_loops, whose oracle bandwidth lies in [lo, hi]."""
    for seed in seeds:
        full = random_loops(n, n_loops, seed)
        for keep in range(n_loops, 0, -1):
            w = oracle.PoseGraph(full["odom"], full["loops"][:keep], full["loop_info"][:keep]).bandwidth
            if lo <= w <= hi:
                return (n, n_loops, seed, keep), w
            if w < lo:
                break
    return None, None


def band_graph(name):
    n, n_loops, seed, keep = BANDS[name][:4]
    return random_loops(n, n_loops, seed, keep=keep)


def panel_width(w):
    """The solver's panel width for half bandwidth w (pg_panel_width in posegraph.hip)."""
    return 8 if w <= 120 else 4


def _to_keyframe_order(Hp, gp, pos):
    idx = (4 * np.asarray(pos, np.int64)[:, None] + np.arange(4)[None, :]).reshape(-1)       # keyframe-order scalar -> position-order scalar
    return Hp[np.ix_(idx, idx)], gp[idx]


def expand_gpu(buf, n, w, pos):
    """GPU reduce buffer -> (H [4n,4n], g [4n], cost [n] per position) in keyframe order."""
    buf = np.asarray(buf, np.float64)
    hsz = n * (w + 1) * 16
    assert buf.size == hsz + 5 * n
    B = buf[:hsz].reshape(n, w + 1, 4, 4)
    Hp = np.zeros((4 * n, 4 * n))
    for p in range(n):
        for d in range(min(w, p) + 1):
            blk = B[p, d]
            if d == 0:
                assert np.array_equal(blk, blk.T), "diagonal block %d is not symmetric" % p
                Hp[4 * p:4 * p + 4, 4 * p:4 * p + 4] = blk
            else:
                Hp[4 * p:4 * p + 4, 4 * (p - d):4 * (p - d) + 4] = blk
                Hp[4 * (p - d):4 * (p - d) + 4, 4 * p:4 * p + 4] = blk.T
        assert not B[p, min(w, p) + 1:].any(), "block row %d has entries left of column 0" % p
    H, g = _to_keyframe_order(Hp, buf[hsz:hsz + 4 * n], pos)
    return H, g, buf[hsz + 4 * n:].copy()


def expand_oracle(buf, n, w, pos):
    """Oracle reduce buffer -> (H [4n,4n], g [4n], cost) in keyframe order."""
    buf = np.asarray(buf, np.float64)
    n4, bw = 4 * n, 4 * (w + 1)
    assert buf.size == n4 * bw + n4 + 1
    B = buf[:n4 * bw].reshape(n4, bw)
    Hp = np.zeros((n4, n4))
    for i in range(n4):
        c0 = 4 * (i // 4 - w)
        lo = max(c0, 0)
        Hp[i, lo:i + 1] = B[i, lo - c0:i + 1 - c0]
        Hp[lo:i + 1, i] = B[i, lo - c0:i + 1 - c0]
        assert not B[i, :lo - c0].any() and not B[i, i + 1 - c0:].any(), "scalar row %d has entries outside the lower band" % i
    H, g = _to_keyframe_order(Hp, buf[n4 * bw:n4 * bw + n4], pos)
    return H, g, float(buf[n4 * bw + n4])


def close(a, b, rel=1e-12):
    """max|a - b| <= rel (max|b| + 1), the fp64-against-fp64 form of tests/test_ba_factors_gpu.py; returns (ok, gap, bound)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    gap = float(np.abs(a - b).max()) if a.size else 0.0
    bound = rel * (float(np.abs(b).max()) + 1.0 if b.size else 1.0)
    return gap <= bound, gap, bound
