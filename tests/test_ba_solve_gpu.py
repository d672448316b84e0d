"""k_ba_solve (through the C ABI) against the CPU restatement of Estimator::optimization()'s solve."""
import numpy as np
import pytest

from tests import ba_cases as K

pytestmark = pytest.mark.gpu


def _solve_gpu(gpu_ctx, windows, max_iter=30):
    import lmono_amd
    b = lmono_amd.BaBatch(gpu_ctx, windows)
    b.solve(max_iter)
    return b, b.read()


def test_batch_of_windows_matches_oracle(oracle, gpu_ctx):
    windows = [K.make_window(s) for s in range(6)]
    windows[4]["use_mono"] = False          # static_status
    windows[5]["ex_constant"] = True        # ESTIMATE_LASER == 0
    windows.append(K.make_window(7, n_frames=6))   # window still filling up (frame_count < WINDOW_SIZE)
    b, (poses, ex, invd, sm) = _solve_gpu(gpu_ctx, windows)
    for k, w in enumerate(windows):
        rp, re, rd, rs = oracle.ba_solve(w)
        n = len(w["poses"])
        assert abs(sm[k, 0] - rs.initial_cost) <= 1e-9 * rs.initial_cost
        # same algorithm in fp64 with a different summation order: converged states agree far below the
        # 1e-6 m / 1e-7 rad bound of SURVEY.md 8c
        assert abs(sm[k, 1] - rs.final_cost) <= 1e-6 * rs.final_cost + 1e-9
        assert int(sm[k, 2]) == rs.iterations and int(sm[k, 3]) == rs.termination
        R1, P1 = oracle.ba_reanchor(poses[k, :n], w["gt_Rs"][0], w["gt_Ps"][0])
        R2, P2 = oracle.ba_reanchor(rp, w["gt_Rs"][0], w["gt_Ps"][0])
        assert np.abs(P1 - P2).max() < 1e-6 and np.abs(R1 - R2).max() < 1e-7
        assert np.abs(ex[k] - re).max() < 1e-6
        if w["use_mono"]:
            f0, f1 = b.feat_off[k], b.feat_off[k + 1]
            assert np.abs(invd[f0:f1] - rd).max() < 1e-6


def test_reset_and_resolve_is_repeatable(oracle, gpu_ctx):
    windows = [K.make_window(s) for s in (10, 11)]
    b, first = _solve_gpu(gpu_ctx, windows)
    b.reset(); b.solve(30)
    second = b.read()
    # every sum of k_ba_solve is formed in an order fixed by the problem (static pair schedule, turn-ordered block additions,
    # per-feature passes -- no floating-point atomics): two solves of the same problem give the same BYTES
    for a, c in zip(first, second):
        assert a.tobytes() == c.tobytes()
    # ... also from a different batch object and beside other windows (another grid position, other L2 scratch addresses)
    b2, third = _solve_gpu(gpu_ctx, [K.make_window(3)] + windows)
    assert third[0][1:].tobytes() == first[0].tobytes() and third[1][1:].tobytes() == first[1].tobytes() and third[3][1:].tobytes() == first[3].tobytes()


def test_large_batch_cost_decreases_everywhere(gpu_ctx):
    """256 windows (one per CU): a property check at bench scale -- every window's cost drops by > 1000x."""
    base = [K.make_window(s, n_landmarks=2500) for s in range(8)]
    windows = [base[k % 8] for k in range(256)]
    b, (poses, ex, invd, sm) = _solve_gpu(gpu_ctx, windows)
    assert (sm[:, 1] < 1e-3 * sm[:, 0]).all() and (sm[:, 3] <= 1).all()
    assert np.abs(np.linalg.norm(poses[:, :, 3:], axis=2) - 1).max() < 1e-12


def test_update_reuses_the_batch_and_changes_nothing(oracle, gpu_ctx):
    """lmono_ba_batch_update: the next frame's problem loaded into the previous frame's device arrays (smaller, then larger than
    what the arrays were created for, then a different number of windows) solves exactly like a freshly created batch."""
    import lmono_amd
    small = [K.make_window(21, n_landmarks=400)]
    large = [K.make_window(22, n_landmarks=2500)]
    two = [K.make_window(23), K.make_window(24, n_frames=6)]
    b = lmono_amd.BaBatch(gpu_ctx, [K.make_window(20)])
    b.solve(30)
    b.read()
    for windows in (small, large, two, small):
        b.update(windows)
        b.solve(30)
        got = b.read()
        _, want = _solve_gpu(gpu_ctx, windows)
        for a, c in zip(got, want):
            assert a.tobytes() == c.tobytes()                               # the solve is order-deterministic: same problem, same bytes
        for k, w in enumerate(windows):
            n = len(w["poses"])
            R1, P1 = oracle.ba_reanchor(got[0][k, :n], w["gt_Rs"][0], w["gt_Ps"][0])
            R2, P2 = oracle.ba_reanchor(want[0][k, :n], w["gt_Rs"][0], w["gt_Ps"][0])
            assert np.abs(P1 - P2).max() < 1e-7 and np.abs(R1 - R2).max() < 1e-8


def test_workgroups_per_window_do_not_change_a_bit(oracle, gpu_ctx):
    """K = 1, 2, 4 or 8 workgroups share a window's linearisations and candidate costs (LMONO_OPT_BA_CLUSTER; default: 4 for small batches).  Every sum
    that crosses observations is formed per 16-observation segment and the segments' results are added in segment order by the window's leader,
    so the solve is the same BYTES whatever K is -- also for a window without projection factors, with a constant extrinsic, and while the window
    still fills up -- and agrees with the CPU restatement like the one-workgroup solve."""
    windows = [K.make_window(s) for s in (30, 31, 32)]
    windows[1]["use_mono"] = False
    windows[2]["ex_constant"] = True
    windows.append(K.make_window(33, n_frames=5))
    windows.append(K.make_window(34, n_landmarks=2500))       # many multi-segment frame pairs
    got = {}
    try:
        for k in (1, 2, 4, 8):
            gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, k)
            _, got[k] = _solve_gpu(gpu_ctx, windows)
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 0)
    _, got[0] = _solve_gpu(gpu_ctx, windows)                   # the default choice for a batch of five
    for k in (2, 4, 8, 0):
        for a, c in zip(got[1], got[k]):
            assert a.tobytes() == c.tobytes(), "K = %d differs from K = 1" % k
    sm = got[4][3]
    for k, w in enumerate(windows):
        rp, re, rd, rs = oracle.ba_solve(w)
        assert abs(sm[k, 1] - rs.final_cost) <= 1e-6 * rs.final_cost + 1e-9
        assert int(sm[k, 2]) == rs.iterations and int(sm[k, 3]) == rs.termination


def test_workgroups_of_a_window_on_different_xcds(tmp_path):
    """The exchange between a window's workgroups must be right on ANY placement (HIP promises none): LMONO_BA_SPREAD=1 deals the K workgroups of a
    window to K different XCDs (other L2s: the followers then store device-coherently instead of through the shared L2).  A fresh process per
    setting solves the same windows; the bytes must equal the one-workgroup solve's."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np, lmono_amd\n"
            "from tests import ba_cases as K\n"
            "ctx = lmono_amd.Context(0)\n"
            "ws = [K.make_window(s) for s in (40, 41)] + [K.make_window(42, n_landmarks=2500)]\n"
            "b = lmono_amd.BaBatch(ctx, ws); b.solve(30); p, e, d, sm = b.read()\n"
            "np.savez(sys.argv[1], p=p, e=e, d=d, sm=sm)\n") % root
    out = {}
    for name, env in (("k1", {"LMONO_BA_CLUSTER": "1"}), ("k8", {"LMONO_BA_CLUSTER": "8"}), ("k8_spread", {"LMONO_BA_CLUSTER": "8", "LMONO_BA_SPREAD": "1"}),
                      ("k4_spread", {"LMONO_BA_CLUSTER": "4", "LMONO_BA_SPREAD": "1"})):
        f = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = np.load(f)
    for name in ("k8", "k8_spread", "k4_spread"):
        for key in ("p", "e", "d", "sm"):
            assert out[name][key].tobytes() == out["k1"][key].tobytes(), "%s: %s differs from the one-workgroup solve" % (name, key)
    assert (out["k1"]["sm"][:, 2] == 30).all()


def test_window_of_900_features_matches_the_oracle(oracle, gpu_ctx):
    """VERDICT r4 #6 (the reference sizes para_depth_inv[10000], Estimator.h:256; LMONO_BA_MAX_FEATURES = 1664 since round 6).  Up to 448 features the dogleg
    step's per-feature vectors live in LDS; a batch with a larger window runs the second instantiation of the kernels, which keeps them in an L2
    scratch.  A window of ~870 features (a dense tracker: 560 tracks per frame, 14 px apart) against oracle/lo_ba_solve.c, beside a small window in
    the same batch; for every workgroup count the same bytes; and a window above LMONO_BA_MAX_FEATURES is refused, not truncated."""
    import lmono_amd
    big = K.make_window(50, n_landmarks=20000, max_tracks=560, min_dist=14)
    assert 800 <= len(big["inv_depth"]) <= 1024
    small = K.make_window(51)
    got = {}
    try:
        for k in (1, 8):
            gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, k)
            _, got[k] = _solve_gpu(gpu_ctx, [big, small])
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 0)
    for a, c in zip(got[1], got[8]):
        assert a.tobytes() == c.tobytes()
    poses, ex, invd, sm = got[8]
    for k, w in enumerate((big, small)):
        rp, re, rd, rs = oracle.ba_solve(w)
        n = len(w["poses"])
        assert abs(sm[k, 0] - rs.initial_cost) <= 1e-9 * rs.initial_cost
        assert abs(sm[k, 1] - rs.final_cost) <= 1e-6 * rs.final_cost + 1e-9
        assert int(sm[k, 2]) == rs.iterations and int(sm[k, 3]) == rs.termination
        R1, P1 = oracle.ba_reanchor(poses[k, :n], w["gt_Rs"][0], w["gt_Ps"][0])
        R2, P2 = oracle.ba_reanchor(rp, w["gt_Rs"][0], w["gt_Ps"][0])
        assert np.abs(P1 - P2).max() < 1e-6 and np.abs(R1 - R2).max() < 1e-7
    # the small window beside the big one solves like the small window alone (LDS-resident instantiation): tolerance, not bytes -- the two
    # instantiations round the same sums the same way, but that is not promised
    _, alone = _solve_gpu(gpu_ctx, [small])
    assert np.abs(alone[0][0] - poses[1]).max() < 1e-9
    too_big = K.make_window(54, n_landmarks=60000, max_tracks=1100, min_dist=9)
    assert len(too_big["inv_depth"]) > 1664
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.BaBatch(gpu_ctx, [too_big])


def test_window_at_the_trackers_ceiling_matches_the_oracle(oracle, gpu_ctx):
    """VERDICT r5 (missing #5): the reference's tracker holds MAX_CNT = 150 tracks per frame (FeatureTracker.cc:21), so the 11 frames of a window can
    hold at most 1650; LMONO_BA_MAX_FEATURES = 1664 covers that.  A window of ~1590 features / ~8000 projection factors (a tracker far denser than the
    reference's) against oracle/lo_ba_solve.c, the same bytes with one and with eight workgroups, and the per-track calls take it as well."""
    import lmono_amd
    w = K.make_window(54, n_landmarks=40000, max_tracks=1000, min_dist=10)
    assert 1500 <= len(w["inv_depth"]) <= 1664
    got = {}
    try:
        for k in (1, 8):
            gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, k)
            _, got[k] = _solve_gpu(gpu_ctx, [w])
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 0)
    for a, c in zip(got[1], got[8]):
        assert a.tobytes() == c.tobytes()
    poses, ex, invd, sm = got[8]
    rp, re, rd, rs = oracle.ba_solve(w)
    n = len(w["poses"])
    assert abs(sm[0, 0] - rs.initial_cost) <= 1e-9 * rs.initial_cost
    assert abs(sm[0, 1] - rs.final_cost) <= 1e-6 * rs.final_cost + 1e-9
    assert int(sm[0, 2]) == rs.iterations and int(sm[0, 3]) == rs.termination
    R1, P1 = oracle.ba_reanchor(poses[0, :n], w["gt_Rs"][0], w["gt_Ps"][0])
    R2, P2 = oracle.ba_reanchor(rp, w["gt_Rs"][0], w["gt_Ps"][0])
    assert np.abs(P1 - P2).max() < 1e-6 and np.abs(R1 - R2).max() < 1e-7


def test_large_window_cluster_repeats_give_one_workgroups_bytes(gpu_ctx):
    """in the kBig instantiation a follower reads the inverse depths straight from the leader's mail box, which the leader rewrites at
    every publish of the same launch; that read must bypass the follower's L1 on every placement (a line cached during the previous linearisation would
    answer with the old state -- silently, and only when the L1 happened not to evict it).  The K = 8 solve of an ~870-feature window, repeated on one batch
    (accepted steps: the state moves 30 times per solve), must give the one-workgroup solve's bytes every time."""
    import lmono_amd
    big = K.make_window(53, n_landmarks=20000, max_tracks=560, min_dist=14)
    assert len(big["inv_depth"]) > 448
    try:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 1)
        _, want = _solve_gpu(gpu_ctx, [big])
        assert want[3][0, 4] >= 10                                     # successful steps: the inverse depths did move
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 8)
        b = lmono_amd.BaBatch(gpu_ctx, [big])
        for rep in range(12):
            b.reset(); b.solve(30)
            got = b.read()
            for a, c in zip(want, got):
                assert a.tobytes() == c.tobytes(), "repeat %d of the K = 8 solve differs from K = 1" % rep
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 0)


def test_cluster_that_gives_up_is_solved_again_with_one_workgroup(tmp_path):
    """every workgroup of a cluster must be resident while it polls; the budget (half the device's CUs, from
    hipDeviceProp_t::multiProcessorCount) is a guess about a card the context does not own.  When a poll runs out, the failure flag comes back set and
    lmono_ba_batch_read re-runs the whole solve from the state it started from with ONE workgroup per window (same bytes by construction) instead of
    failing the Estimator's frame.  LMONO_BA_TEST_FAIL=1 sets the flag before the launch; LMONO_CLUSTER_BUDGET=16 shows the budget is honoured."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np, lmono_amd\n"
            "from tests import ba_cases as K\n"
            "ctx = lmono_amd.Context(0)\n"
            "ws = [K.make_window(s) for s in (60, 61)] + [K.make_window(62, n_landmarks=2500)]\n"
            "b = lmono_amd.BaBatch(ctx, ws); b.solve(30); p, e, d, sm = b.read()\n"
            "b.solve(30); p2, e2, d2, sm2 = b.read()\n"                 # a second solve continues from the first one's result: the snapshot is per solve
            "np.savez(sys.argv[1], p=p, e=e, d=d, sm=sm, p2=p2, e2=e2, d2=d2, sm2=sm2)\n") % root
    out = {}
    for name, env in (("k1", {"LMONO_BA_CLUSTER": "1"}), ("k8_fail", {"LMONO_BA_CLUSTER": "8", "LMONO_BA_TEST_FAIL": "1"}),
                      ("budget16", {"LMONO_CLUSTER_BUDGET": "16"})):
        f = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = np.load(f)
    for name in ("k8_fail", "budget16"):
        for key in ("p", "e", "d", "sm", "p2", "e2", "d2", "sm2"):
            assert out[name][key].tobytes() == out["k1"][key].tobytes(), "%s: %s differs from the one-workgroup solve" % (name, key)
    assert (out["k1"]["sm"][:, 3] <= 1).all()


def test_clusters_beyond_the_first_eight_windows(gpu_ctx):
    """Round 6 regression: with several workgroups per window, block index != window index.  The LASERFactor chain and the extrinsic prior read their
    constants by blockIdx.x, which happened to equal the window for the leaders of windows 0..7 -- every cluster test of round 5 used at most seven
    windows -- and was another window's (or past the array's end) from window 8 on: batches of 9..64 windows (K >= 2) solved a different problem than
    K = 1.  Found by EstimatorBatch's per-stream byte comparison at 48 and 64 streams.  24 different windows, K = 1 / 2 / 4 and the default (4): same bytes."""
    base = [K.make_window(70 + s) for s in range(6)]
    windows = [base[(k * 5 + k // 6) % 6] for k in range(24)]          # neighbours in the batch are different windows
    got = {}
    try:
        for k in (1, 2, 4):
            gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, k)
            _, got[k] = _solve_gpu(gpu_ctx, windows)
    finally:
        gpu_ctx.set_option(gpu_ctx.OPT_BA_CLUSTER, 0)
    _, got[0] = _solve_gpu(gpu_ctx, windows)
    for k in (2, 4, 0):
        for a, c in zip(got[1], got[k]):
            assert a.tobytes() == c.tobytes(), "K = %d differs from K = 1 on a batch of 24 windows" % k
    # the windows really differ from one another (a block reading its neighbour's constants would show)
    assert len({got[1][0][k].tobytes() for k in range(24)}) == 6
