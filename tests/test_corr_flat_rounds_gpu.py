"""k_corr_flat's round (carried line window, single-pass posting with empty requests, per-wave prefixes, two pool counters): the
correspondences of the default search against the oracle's, index for index, on inputs chosen so that each part of the round is at work.
Every case first shows on the ORACLE's output alone that it is not vacuous (most features have partners; where the case needs
growing balls, some have none: those searched up to the 5 m ball)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAR_Q = np.array([0.0, 0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.0, 0.05, 1.0])
FAR_T = np.array([3.0, 2.0, 0.5])          # a few metres off: most features need several nearest-point rounds
NEAR_Q = np.array([0.0, 0.0, 0.008, 1.0]) / np.linalg.norm([0.0, 0.0, 0.008, 1.0])
NEAR_T = np.array([0.75, -0.01, 0.0])      # close to the true motion (0.8 m per scan)
IDENT_Q = np.array([0.0, 0.0, 0.0, 1.0])
IDENT_T = np.zeros(3)


def _register(ctx, xyzi, off, n_lines=64, min_range=5.0):
    import torch
    import lmono_amd
    dev = torch.from_numpy(xyzi).cuda()
    batch = lmono_amd.ScanBatch(ctx, len(off) - 1, len(xyzi))
    batch.scanreg(dev.data_ptr(), off, n_lines, min_range, keepalive=dev)
    return batch


def _oracle_corr(oracle, xyzi, off, k, q, t, n_lines=64, min_range=5.0):
    f = [oracle.scanreg(xyzi[off[s]:off[s + 1]], n_lines, min_range) for s in (k - 1, k)]
    _, _, _, corr = oracle.odom_step(f[1]["sharp"], f[1]["flat"], f[0]["less_sharp"], f[0]["less_flat"], q, t, want_corr=True)
    return corr[0], f


def _moved(pts, q, t):
    """Feature points under the warm start (x, y, z, w quaternion and translation), as the search sees them."""
    x, y, z, w = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return pts[:, :3].astype(np.float64) @ rot.T + t


def _not_vacuous(corr, need_unmatched):
    has = corr[:, 3] != 0
    print("oracle: %d features, %d with partners, %d without" % (len(corr), has.sum(), (~has).sum()))
    assert has.sum() * 2 >= len(corr)
    if need_unmatched:
        assert (~has).any()              # no partner within 5 m: the search grew its ball to the last rung


def _check(oracle, gpu_ctx, xyzi, off, cases, n_lines=64, min_range=5.0, need_unmatched=False):
    refs = []
    for k, q, t in cases:                # the oracle first: the case is judged before the GPU is involved
        corr, _ = _oracle_corr(oracle, xyzi, off, k, q, t, n_lines, min_range)
        _not_vacuous(corr, need_unmatched)
        refs.append(corr)
    batch = _register(gpu_ctx, xyzi, off, n_lines, min_range)
    for (k, q, t), corr in zip(cases, refs):
        assert np.array_equal(batch.correspond(k, q, t), corr), "scan %d, t = %s" % (k, t)


@pytest.mark.parametrize("n_rings", [16, 32, 64])
def test_growing_windows(oracle, gpu_ctx, n_rings):
    """Warm start far from the truth: the balls grow round after round, the carried window is extended again and again and reaches
    every line of the sensor for the features without a partner."""
    w = oracle.S1World(n_az=600, n_rings=n_rings)
    xyzi, off = w.scans(w.trajectory(3))
    _check(oracle, gpu_ctx, xyzi, off, [(1, FAR_Q, FAR_T), (2, FAR_Q, FAR_T)], n_rings, 5.0, need_unmatched=True)


def test_holes_inside_a_window(oracle, gpu_ctx):
    """Every point of every third ring of the scans is dropped: the windows of the growing balls hold lines without points (their own
    range misses every ball), which the single-pass posting fills with empty requests."""
    w = oracle.S1World(n_az=600, n_rings=64)
    xyzi, off = w.scans(w.trajectory(3))
    elev = np.arctan2(xyzi[:, 2], np.hypot(xyzi[:, 0], xyzi[:, 1]))
    ring = np.abs(elev[:, None].astype(np.float64) - np.asarray(w.elev)[None, :]).argmin(axis=1)
    scan_of = np.searchsorted(off, np.arange(len(xyzi)), side="right") - 1
    keep = ~((ring % 3 == 1) & (scan_of < 2))          # scans 0 and 1 are the "last" clouds of the pairs searched below
    assert (~keep).sum() > len(xyzi) // 6
    off2 = np.concatenate([[0], np.cumsum(np.bincount(scan_of[keep], minlength=3))]).astype(off.dtype)
    xyzi2 = np.ascontiguousarray(xyzi[keep])
    _check(oracle, gpu_ctx, xyzi2, off2, [(1, FAR_Q, FAR_T), (2, FAR_Q, FAR_T), (2, NEAR_Q, NEAR_T)], need_unmatched=True)


@pytest.mark.parametrize("n_rings", [16, 64])
def test_all_azimuth_and_wrapping_arcs(oracle, gpu_ctx, n_rings):
    """Points from 0.5 m on and a warm start that moves feature points onto the sensor axis (balls that cover every azimuth), in the
    sensor frame and in one turned about the vertical, so that other features sit at the seam between the last azimuth bin and the
    first (arcs that wrap)."""
    w = oracle.S1World(n_az=600, n_rings=n_rings)
    xyzi, off = w.scans(w.trajectory(3))
    axis_t = np.array([-5.0, 2.0, 0.0])
    cases = [(1, NEAR_Q, NEAR_T), (2, IDENT_Q, axis_t)]
    for yaw in (0.0, 0.37):
        c, s = np.cos(yaw), np.sin(yaw)
        rot = xyzi.copy()
        rot[:, 0] = (c * xyzi[:, 0] - s * xyzi[:, 1]).astype(np.float32)
        rot[:, 1] = (s * xyzi[:, 0] + c * xyzi[:, 1]).astype(np.float32)
        # on the oracle's features alone, at the poses of the cases: the smallest first ball (0.25 m) of some feature already reaches
        # across the seam (azimuth +-pi), and the second warm start puts some within 1 m of the axis (their partners are metres away:
        # their balls grow past the axis)
        f = oracle.scanreg(rot[off[1]:off[2]], n_rings, 0.5)
        p1 = _moved(np.concatenate([f["sharp"], f["flat"]]), NEAR_Q, NEAR_T)
        rho = np.hypot(p1[:, 0], p1[:, 1])
        assert (np.pi - np.abs(np.arctan2(p1[:, 1], p1[:, 0])) < np.arcsin(np.minimum(1.0, 0.25 / rho))).any()
        f = oracle.scanreg(rot[off[2]:off[3]], n_rings, 0.5)
        p2 = _moved(np.concatenate([f["sharp"], f["flat"]]), IDENT_Q, axis_t)
        assert (np.hypot(p2[:, 0], p2[:, 1]) < 1.0).any()
        _check(oracle, gpu_ctx, rot, off, cases, n_rings, 0.5)


def test_pool_pressure(oracle, gpu_ctx):
    """3000 azimuth steps per ring and the identity warm start (the largest first balls): more first-round requests than the pool
    holds, features post a round late -- now with a slot reserved for every line of their window."""
    w = oracle.S1World(n_az=3000)
    xyzi, off = w.scans(w.trajectory(2))
    _check(oracle, gpu_ctx, xyzi, off, [(1, IDENT_Q, IDENT_T), (1, FAR_Q, FAR_T)])


def test_both_pool_counters(oracle, gpu_ctx):
    """The two pool counters alternate by the round's parity, through the nearest-point rounds into the walk's.  Warm starts near the
    truth (the seeded balls settle in one round), at the identity and far off give the workgroups of a scan pair short and long round
    sequences: both counters open a walk, and both are re-used after being zeroed."""
    w = oracle.S1World(n_az=600, n_rings=64)
    xyzi, off = w.scans(w.trajectory(3))
    _check(oracle, gpu_ctx, xyzi, off, [(k, q, t) for k in (1, 2) for q, t in ((NEAR_Q, NEAR_T), (IDENT_Q, IDENT_T), (FAR_Q, FAR_T))])


def test_sequential_and_chained_odometry(oracle, gpu_ctx):
    """The whole odometry through the new round: the sequential run, and a chained run with a thinned lead-in (2 chains, lead 6, the
    first 3 lead-in pairs on every fourth share of the features), whose validated boundary is repaired to the sequential result."""
    w = oracle.S1World(n_az=600)
    xyzi, off = w.scans(w.trajectory(20))
    ref = oracle.run_sequence(xyzi, off)
    batch = _register(gpu_ctx, xyzi, off)
    incr, poses = batch.odometry(1, 0)
    print("sequential: max |incr - oracle| %.3e, max |poses - oracle| %.3e" % (np.abs(incr - ref["incr"]).max(), np.abs(poses - ref["poses"]).max()))
    assert np.abs(incr - ref["incr"]).max() < 1e-9 and np.abs(poses - ref["poses"]).max() < 1e-8
    gpu_ctx.set_option(gpu_ctx.OPT_LEAD_FULL, 3)
    try:
        incr_c, poses_c = batch.odometry(2, 6)
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_LEAD_FULL, -1)
    print("2 chains, lead 6, lead_full 3: max |incr - oracle| %.3e, max |poses - oracle| %.3e" % (np.abs(incr_c - ref["incr"]).max(), np.abs(poses_c - ref["poses"]).max()))
    assert np.abs(incr_c - ref["incr"]).max() < 1e-9 and np.abs(poses_c - ref["poses"]).max() < 1e-8
