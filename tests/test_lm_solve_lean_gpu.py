"""k_lm_solve's sums and trust-region hand-over at their edges.  The kernel sums 28 doubles over a 256-thread workgroup (a reduce-scatter
inside each wave, lmono_amd/csrc/wave_sum28.hpp, then the four wave partials in fixed order), so the block counts that matter are the
wave's and the workgroup's: 0, 1, 63, 64, 65, 255, 256, 257 and more than two trips.  Every case runs through a context created under
LMONO_LM_LDS_PLANES=4 and one under the shipped value and compares increments and poses byte for byte; sequential runs are held to the
1e-9 of the oracle that tests/test_lm_solve_planes_gpu.py uses, whose builders and context pair this file shares.  Every precondition
(block counts, a solve that ends before its first iteration, a solve whose steps are all rejected, thinned pairs, a boundary that does not agree) is read
off the ORACLE's output; the builders need no GPU.

Not here: a scan that IS flagged irregular.  The oracle appends its feature clouds scan line by scan line and the device sorts rings
stably, so no raw scan through the public API sets kStatusIrregularLines (nor, at these sizes, kStatusDenseCell, the other way onto the
array-order walk of correspond_wave); tests/test_compact_index_gpu.py has the same limit."""
import numpy as np
import pytest

from tests import test_lm_solve_planes_gpu as P
from tests.test_lm_solve_planes_gpu import ctx_pair  # noqa: F401  (the module-scoped fixture: both contexts)

pytestmark = pytest.mark.gpu

IRREGULAR = 4          # kStatusIrregularLines
BLOCK_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)

_cache = {}


def _nq(oracle, pts, n_lines=16, min_range=5.0):
    f = oracle.scanreg(pts, n_lines, min_range)
    return int(f["info"].n_sharp + f["info"].n_flat)


def pair_with_blocks(oracle, target):
    """Two 16-ring scans; the second is cut down until the oracle finds exactly `target` feature points (sharp + flat) in it, which is the
    number of residual blocks of the pair: whole rings from the top down while the count stays at or below the target, then a prefix of
    the next ring in azimuth order, shortened point by point.  0: eight points of one ring (too few for a curvature)."""
    if target in _cache:
        return _cache[target]
    s = P.seq_rings16(oracle, 2)
    xyzi, off = s["xyzi"], s["off"]
    a = xyzi[off[1]:off[2]]
    ring, b = P._ring_and_bin(s["world"], a)
    keep = None
    if target == 0:
        keep = np.zeros(len(a), bool)
        keep[np.flatnonzero(ring == 8)[:8]] = True
    for start in range(15, 3, -1):
        if keep is not None:
            break
        base = np.zeros(len(a), bool)
        r = start
        while r >= 0 and _nq(oracle, a[base | (ring == r)]) <= target:
            base |= ring == r
            r -= 1
        if base.any() and _nq(oracle, a[base]) == target:
            keep = base
            break
        if r < 0:
            continue
        idx = np.flatnonzero(ring == r)
        idx = idx[np.argsort(b[idx], kind="stable")]
        for m in range(len(idx), 0, -1):
            trial = base.copy()
            trial[idx[:m]] = True
            if _nq(oracle, a[trial]) == target:
                keep = trial
                break
    assert keep is not None, "no cut of the scan has %d feature points" % target
    cut = a[keep]
    out = dict(xyzi=np.ascontiguousarray(np.concatenate([xyzi[off[0]:off[1]], cut])),
               off=np.array([0, off[1] - off[0], off[1] - off[0] + len(cut)], off.dtype), n_lines=16, min_range=5.0)
    _cache[target] = out
    return out


def pair_at_rest_in_an_exact_room(oracle):
    """The same scan twice: the room of tests/test_lm_solve_planes_gpu.py with every point moved onto its wall's (or the ground's) plane
    exactly, the ground at -1.75, and everything scaled by 1 / 16 -- the planes' coordinates have few mantissa bits, so the voxel filter's
    centroids lie on them exactly as well, every plane block's residual is exactly 0 at the identity, and the gradient is 0."""
    w = P._room(oracle, 1200)
    xyzi, _ = w.scans(P._room_poses(1))
    a = xyzi.copy()
    on_plane = np.zeros(len(a), bool)
    for axis, at, to in ((0, -18.0, -18.0), (0, 18.0, 18.0), (1, -14.0, -14.0), (1, 14.0, 14.0), (2, -1.73, -1.75)):
        m = np.abs(a[:, axis] - at) < 2e-3
        a[m, axis] = np.float32(to)
        on_plane |= m
    a = a[on_plane]
    a[:, :3] *= np.float32(1.0 / 16)
    return dict(xyzi=np.ascontiguousarray(np.concatenate([a, a])), off=np.array([0, len(a), 2 * len(a)], np.int64), n_lines=16, min_range=0.1)


def pair_with_rejected_steps(oracle):
    """The plane-only room (tests/test_lm_solve_planes_gpu.py) and the same scan shrunk to 0.9 of its size and turned by 16 degrees of
    pitch and 20 of yaw, found by a random search over such pairs on the oracle: its first outer iteration accepts steps, and in the
    second one no step of the four iterations lowers the cost (the test states that on the oracle's figures)."""
    s = P.seq_plane_only(oracle, 1)
    a = s["xyzi"]
    p, y = 0.2831145121869263, 0.3518668938409201
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    b = a.copy()
    b[:, :3] = ((a[:, :3].astype(np.float64) @ (Rz @ Ry).T) * 0.9).astype(np.float32)
    return dict(xyzi=np.ascontiguousarray(np.concatenate([a, b])), off=np.array([0, len(a), len(a) + len(b)], np.int64), n_lines=16, min_range=0.25)


def _odom_stats(oracle, s, k):
    f = [oracle.scanreg(s["xyzi"][s["off"][j]:s["off"][j + 1]], s["n_lines"], s["min_range"]) for j in (k - 1, k)]
    return oracle.odom_step(f[1]["sharp"], f[1]["flat"], f[0]["less_sharp"], f[0]["less_flat"], [0, 0, 0, 1], [0, 0, 0])[2]


def _is_irregular(oracle, pts, n_lines, min_range):
    """kStatusIrregularLines as the cloud says it: some line a >= b + 3 starts before line b ends (tests/test_compact_index_gpu.py)."""
    ref = oracle.scanreg(pts, n_lines, min_range)
    for name in ("less_sharp", "less_flat"):
        ln = np.clip(ref[name][:, 3].astype(np.int32), 0, 65)
        first = np.full(66, 1 << 30)
        last = np.full(66, -1)
        np.minimum.at(first, ln, np.arange(len(ln)))
        np.maximum.at(last, ln, np.arange(len(ln)))
        if any(first[a] < last[b] for a in range(66) for b in range(max(a - 2, 0))):
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", BLOCK_COUNTS)
def test_block_counts_at_the_wave_and_workgroup_edges(oracle, ctx_pair, target):  # noqa: F811
    s = pair_with_blocks(oracle, target)
    assert P.block_counts(oracle, s)[1][1] == target
    P._sequential_on_both(oracle, ctx_pair, s)


def test_more_than_two_trips(oracle, ctx_pair):  # noqa: F811
    s = P.seq_rings64(oracle, 2)
    assert P.block_counts(oracle, s)[1][1] > 2 * P.K_LM_T
    P._sequential_on_both(oracle, ctx_pair, s)


def test_edges_only_and_planes_only(oracle, ctx_pair):  # noqa: F811
    s = P.seq_edge_only(oracle, 2)
    assert all(e == n and n > 0 for e, n in P.block_counts(oracle, s))
    P._sequential_on_both(oracle, ctx_pair, s)
    s = P.seq_plane_only(oracle, 2)
    assert all(e == 0 and n > P.K_LM_T for e, n in P.block_counts(oracle, s))
    P._sequential_on_both(oracle, ctx_pair, s)


def test_solve_that_ends_before_its_first_iteration(oracle, ctx_pair):  # noqa: F811
    s = pair_at_rest_in_an_exact_room(oracle)
    st = _odom_stats(oracle, s, 1)
    assert list(st.lm_iters) == [0, 0] and list(st.initial_cost) == [0.0, 0.0] and min(st.n_plane_corr) > 50     # blocks, and no gradient
    ref = P._sequential_on_both(oracle, ctx_pair, s)
    assert np.array_equal(ref["incr"][1], [0, 0, 0, 1, 0, 0, 0])


def test_pair_with_rejected_steps(oracle, ctx_pair):  # noqa: F811
    """An accepted step lowers the cost strictly and every tolerance exit ends the loop, so a solve of two or more iterations whose final
    cost EQUALS its initial, non-zero cost had every step rejected: judge() kept s_cur, shrank the radius and propose() ran again on the
    sums of the first sweep, and each candidate's sums decided a rejection.  Here that is the second outer iteration; the first one
    accepts steps, so the pose the rejections must leave alone is not the identity."""
    s = pair_with_rejected_steps(oracle)
    st = _odom_stats(oracle, s, 1)
    print("oracle: iterations %s, initial cost %s, final cost %s" % (list(st.lm_iters), list(st.initial_cost), list(st.final_cost)))
    assert st.lm_iters[1] >= 2 and st.final_cost[1] == st.initial_cost[1] > 0           # every step of the second solve rejected
    assert st.lm_iters[0] >= 2 and st.final_cost[0] < st.initial_cost[0]                # and the first solve moved the pose
    ref = P._sequential_on_both(oracle, ctx_pair, s)
    assert np.abs(ref["incr"][1] - [0, 0, 0, 1, 0, 0, 0]).max() > 1e-3


def test_chains_with_thinned_lead_in_pairs(oracle, ctx_pair):  # noqa: F811
    s = P.seq_rings64(oracle, 12)
    n, n_chains, lead, lead_full = 12, 4, 3, 1
    assert len({c for c, _ in P.thinned_pairs(n, n_chains, lead, lead_full)}) >= 2
    res = []
    for c in ctx_pair:
        batch = P._register(c, s)
        c.set_option(c.OPT_LEAD_FULL, lead_full)
        try:
            res.append(batch.odometry(n_chains, lead))
        finally:
            c.set_option(c.OPT_LEAD_FULL, -1)
    assert P._same_bytes(res[0][0], res[1][0]) and P._same_bytes(res[0][1], res[1][1])
    ref = oracle.run_sequence(s["xyzi"], s["off"])
    assert np.abs(res[1][0] - ref["incr"]).max() < 1e-4            # the bound of a repaired layout in tests/test_lidar_gpu.py


def test_chains_with_flagged_boundaries(oracle, ctx_pair):  # noqa: F811
    """The repair path writes incr and rstat from the solve's thread 0."""
    s = P.seq_rings64(oracle, 12)
    seq = oracle.run_sequence(s["xyzi"], s["off"])
    plain = oracle.run_sequence(s["xyzi"], s["off"], n_chains=3, lead=1)
    assert np.abs(plain["incr"] - seq["incr"]).max() > 1e-4
    res, reps = [], []
    for c in ctx_pair:
        batch = P._register(c, s)
        res.append(batch.odometry(3, 1))
        reps.append(batch.boundary_report())
    for rep in reps:
        assert rep["flagged"] >= 1 and rep["pairs_rerun"] >= 1 and rep["unresolved"] == 0
    assert reps[0]["flagged"] == reps[1]["flagged"] and reps[0]["pairs_rerun"] == reps[1]["pairs_rerun"]
    assert P._same_bytes(res[0][0], res[1][0]) and P._same_bytes(res[0][1], res[1][1])
    assert np.abs(res[1][0] - seq["incr"]).max() < 1e-4


@pytest.mark.parametrize("every", [1, 7])
def test_records_from_the_fall_back_search(oracle, ctx_pair, every):  # noqa: F811
    """LMONO_OPT_DEFER_EVERY hands every n-th feature (1: all of them) to k_correspond_list, which then writes their records."""
    s = P.seq_rings16(oracle, 4)
    for c in ctx_pair:
        c.set_option(c.OPT_DEFER_EVERY, every)
    try:
        for c in ctx_pair:
            c.timing_reset()
        P._sequential_on_both(oracle, ctx_pair, s)
        for c in ctx_pair:
            assert c.timing()[0]["deferred_features"] > 0
    finally:
        for c in ctx_pair:
            c.set_option(c.OPT_DEFER_EVERY, 0)


def test_shuffled_scan(oracle, ctx_pair):  # noqa: F811
    """A scan whose points arrive in random order: the stable ring sort still defines the cloud, and the irregular-lines flag stays
    clear on both sides (no raw scan sets it, see the head of this file)."""
    s = P.seq_rings16(oracle, 4)
    xyzi, off = s["xyzi"].copy(), s["off"]
    np.random.default_rng(3).shuffle(xyzi[off[1]:off[2]], axis=0)
    s = dict(s, xyzi=xyzi)
    assert not _is_irregular(oracle, xyzi[off[1]:off[2]], 16, 5.0)
    P._sequential_on_both(oracle, ctx_pair, s)
    for c in ctx_pair:
        assert not P._register(c, s).counts()[1, 5] & IRREGULAR


def test_online_stream_for_three_steps(oracle, ctx_pair):  # noqa: F811
    import lmono_amd
    s = P.seq_rings16(oracle, 3)
    xyzi, off = s["xyzi"], s["off"]
    ref = oracle.run_sequence(xyzi, off, 16, 5.0)
    out = []
    for c in ctx_pair:
        st = lmono_amd.OdomStream(c, int(np.diff(off).max()) + 1000, 16, 5.0, history=2)
        out.append(np.stack([st.step(xyzi[off[k]:off[k + 1]])[0] for k in range(3)]))
        st.close()
    assert P._same_bytes(out[0], out[1])
    err = np.abs(out[1] - ref["incr"]).max()
    print("online stream: max |incr - oracle| %.3e" % err)
    assert err < 1e-9
