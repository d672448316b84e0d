"""The per-track HIP kernels (lmono_amd/csrc/feat.hip: k_triangulate_init, k_depth_refine, k_depth_refine_items, k_outlier_scores, k_shift_depth) at their
edges: against a 50-digit SVD / cost (tests/feat_ref.py), against the oracle on every case family of tests/feat_cases.py with the tolerances of
tests/test_ba_feat.py, across the dispatch between the two refinement kernels, and with malformed descriptors.  tests/test_feat_ref_cpu.py runs the
same references and builders against the oracle's C code without a GPU."""
import numpy as np
import pytest

from tests import feat_cases as K
from tests import feat_ref as R

pytestmark = pytest.mark.gpu


def _agree(got, want, tol, what):
    """|got - want| <= tol elementwise; NaN exactly where the oracle has NaN, infinities equal."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    tol = np.broadcast_to(tol, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % what
    rest = ~((got == want) | np.isnan(want))
    assert np.isfinite(got[rest]).all() and np.isfinite(want[rest]).all(), "%s: infinities differ" % what
    bad = np.nonzero(rest)[0][np.abs(got[rest] - want[rest]) > tol[rest]]
    assert len(bad) == 0, "%s: tracks %s, got %s, want %s" % (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _finite_max(a):
    a = np.abs(a[np.isfinite(a)])
    return a.max() if len(a) else 0.0


def check_against_oracle(gpu_ctx, oracle, wins, track_cnt=3, window_size=10, weight=1500.0, refine_iters=50, scores=True):
    """One batched call per entry point against the oracle window by window, tests/test_ba_feat.py's tolerances: linear depth 1e-9 of the window's largest,
    equal flags, inverse depth 1e-9 (relative above 1), scores 1e-6 of the window's largest + 1.  Returns the GPU's (depth, flag) per window."""
    depth0 = np.concatenate([w["depth0"] for w in wins]) if wins else np.zeros(0)
    kw = dict(track_cnt=track_cnt, window_size=window_size, weight=weight)
    g0, _ = gpu_ctx.triangulate(wins, depth0, refine_iters=-1, **kw)
    g1, gflag = gpu_ctx.triangulate(wins, depth0, refine_iters=refine_iters, **kw)
    gsc = gpu_ctx.outlier_scores(wins, g1, track_cnt=track_cnt, weight=weight) if scores else None
    out, o = [], 0
    for k, w in enumerate(wins):
        n = len(w["trk_start"])
        if n == 0:
            out.append((g1[o:o], gflag[o:o]))
            continue
        with np.errstate(all="ignore"):
            d0, d1, flag = K.oracle_triangulate(oracle, w, refine_iters=refine_iters, **kw)
            _agree(g0[o:o + n], d0, 1e-9 * _finite_max(d0), "window %d linear depth" % k)
            assert np.array_equal(gflag[o:o + n], flag), "window %d flags: %s" % (k, np.nonzero(gflag[o:o + n] != flag)[0][:8])
            _agree(1.0 / g1[o:o + n], 1.0 / d1, 1e-9 * np.maximum(1.0, np.abs(1.0 / d1)), "window %d inverse depth" % k)
            if scores:
                sc = K.oracle_scores(oracle, w, d1, track_cnt=track_cnt, weight=weight)
                _agree(gsc[o:o + n], sc, 1e-6 * (_finite_max(sc) + 1), "window %d scores" % k)
        out.append((g1[o:o + n].copy(), gflag[o:o + n].copy()))
        o += n
    return out


def test_linear_step_against_the_50_digit_svd(gpu_ctx):
    """k_triangulate_init takes the eigenvector of A^T A; the reference takes the SVD of A.  Per track of the parallax sweep (baselines 0.8 .. 1e-4 m per
    frame, depths 2 .. 250 m, 5e-4 noise, landmarks at z = 0.1 -+ 1e-12 .. 1e-3 and behind the camera, a pure rotation) the relative error of z against
    the 50-digit SVD must be <= 64 * 2^-52 * sigma1^2 / (sigma3^2 - sigma4^2); tracks whose bound exceeds 1e-6 are left out (at most a quarter of them),
    and z < 0.1 -> -1 is decided as the reference decides it wherever |z_ref - 0.1| exceeds the bound.  The oracle's C code (the same algorithm) stays
    at 0.075 of this bound with 1 of 153 tracks left out: tests/test_feat_ref_cpu.py.  Measured on an MI355X: the kernel gives the same figures
    (largest error / bound = 0.0748, 1 of 153 excluded, 59 decisions checked below 0.1 and 88 above)."""
    wins = K.sweep_windows()
    d0, _ = gpu_ctx.triangulate(wins, np.concatenate([w["depth0"] for w in wins]), refine_iters=-1)
    off = np.concatenate([[0], np.cumsum([len(w["trk_start"]) for w in wins])])
    rep = K.linear_step_report([d0[off[k]:off[k + 1]] for k in range(len(wins))])
    print("linear step, k_triangulate_init vs 50-digit SVD: %d tracks, %d excluded (%.1f %%), largest error / bound = %.3g, decisions checked: %d below 0.1, %d above"
          % (rep["n"], rep["excluded"], 100.0 * rep["excluded"] / rep["n"], rep["worst_ratio"], rep["below"], rep["above"]))
    assert not rep["failures"], "\n".join(rep["failures"])
    assert rep["excluded"] * 4 <= rep["n"]
    assert rep["below"] >= 5 and rep["above"] >= 5


def test_sweep_and_mixed_states_match_oracle(gpu_ctx, oracle):
    """every sweep window (low parallax, rejected and behind-the-camera tracks with depth -1 in refinement and score, pure rotation) and the mixed window
    (given depths, lengths 1 and 2, every anchor frame, tracks ending in frame 10) in one batch"""
    check_against_oracle(gpu_ctx, oracle, K.sweep_windows() + [K.mixed_window()])


def test_hostile_numerics_match_oracle(gpu_ctx, oracle):
    """A point at infinity (every shared step invalid: five of them end the loop, no depth moves, its own depth stays inf and is flagged 2), a runaway
    start 1 / d = 1e7, refined depths on both sides of 0.1 and of 300, and -- under track_cnt = 2 -- {9, 10}-only tracks whose depth goes through
    1 / (1 / d) onto exactly 0.1 (flag 1), the double below (2), exactly 300 (1) and the double above (2)."""
    res = check_against_oracle(gpu_ctx, oracle, [K.hostile_window(True), K.empty_window(), K.hostile_window(False)])
    d, flag = res[0]
    assert np.isinf(d[5]) and flag[5] == 2
    d, flag = res[2]
    assert list(flag[13:17]) == [2, 1, 1, 2] and d[13] < 0.1 < d[14] and d[15] < 300 < d[16]
    (d, flag), = check_against_oracle(gpu_ctx, oracle, [K.hostile_window(False)], track_cnt=2)
    assert d[17] == 0.1 and d[18] < 0.1 and d[19] == 300.0 and d[20] > 300.0
    assert list(flag[17:21]) == [1, 2, 1, 2]


def test_empty_windows_first_middle_last(gpu_ctx, oracle):
    """window_of (a binary search over feat_off with duplicate offsets) picks the poses of k_triangulate_init / k_outlier_scores; the refinement goes by
    blockIdx.  Every window has its own trajectory, so a track given a neighbour's poses misses the oracle."""
    e = K.empty_window
    wins = [e(1), e(2), K.plain_window(41, 40), e(3), e(4), K.mixed_window(5), K.plain_window(42, 130), e(6), e(7)]
    check_against_oracle(gpu_ctx, oracle, wins)
    check_against_oracle(gpu_ctx, oracle, [e(1), e(2)])


@pytest.mark.parametrize("kw", [dict(track_cnt=1), dict(track_cnt=2), dict(track_cnt=4), dict(window_size=5), dict(refine_iters=0), dict(refine_iters=1),
                                dict(weight=1.0), dict(track_cnt=2, window_size=5, weight=1.0, refine_iters=1)], ids=str)
def test_arguments_match_oracle(gpu_ctx, oracle, kw):
    """track_cnt 1 / 2 / 4, window_size 5 (10 is every other test's), refine_max_iter 0 / 1, weight 1 (1500 is every other test's), each against the oracle
    with the same arguments (the last case combines them).  Under track_cnt = 1 a single-observation track has no reprojection to average: its score is the 0 / 0 of the mean, NaN,
    on both sides (include/lmono_hip.h states it)."""
    wins = [K.mixed_window(), K.plain_window(43, 60)]
    if kw.get("track_cnt") == 1:
        # a single observation gives the linear step a rank-2 A^T A: which vector of its two-dimensional null space the Jacobi sweep calls the smallest
        # rests on rounding, so that z is an accident, not a property.  Those tracks get a given depth here (the linear step then skips them); what
        # the call does with them -- 1 / (1 / d), flag by the limits, NaN score -- is compared as usual.
        w = dict(wins[0])
        one = (np.diff(w["trk_off"]) == 1) & (w["depth0"] <= 0)
        assert one.any()
        w["depth0"] = np.where(one, 7.0, w["depth0"])
        wins[0] = w
    check_against_oracle(gpu_ctx, oracle, wins, **kw)
    if kw.get("track_cnt") == 1:
        w = wins[0]
        one = np.diff(w["trk_off"]) == 1
        sc = gpu_ctx.outlier_scores([w], np.where(w["depth0"] > 0, w["depth0"], 5.0), track_cnt=1)
        assert one.any() and np.isnan(sc[one]).all() and np.isfinite(sc[~one]).all()


def test_dispatch_between_the_two_refinement_kernels(gpu_ctx, oracle):
    """lmono_triangulate runs k_depth_refine_items when EVERY window has <= 1024 tracks and <= 3072 observations, else k_depth_refine (256 threads) for
    all of them.  A window of <= 256 tracks must come out byte for byte the same alone (items kernel), beside a 3072-observation window (items kernel),
    beside a 3073-observation one and beside a 1025-track one (256-thread kernel), in either order.  The big windows -- 1024 tracks x 3 observations
    (both limits at once), 1025 tracks, 3072 and 3073 observations -- agree with the oracle on whichever kernel they get.  For a 600-track window
    (a thread of the 256-thread kernel owns tracks tid, tid + 256, ...: the wave sums group differently, so equal bits are not guaranteed) the bytes are
    compared and printed; both paths must agree with the oracle at 1e-9 either way.  Measured on an MI355X: "600 tracks, items kernel vs 256-thread
    kernel: same bytes (largest |difference of inverse depth| = 0)" -- the sums only feed the accept / reject decisions and the radius, and a last-bit
    change of a radius >= 1e4 does not reach a step's bits."""
    small = K.plain_window(31, 200)
    w1024, w1025 = K.plain_window(21, 1024, nobs=3), K.plain_window(22, 1025, nobs=3)
    w3072, w3073 = K.plain_window(23, 384, nobs=8), K.plain_window(23, 384, nobs=8, n_long=1)
    (alone,) = check_against_oracle(gpu_ctx, oracle, [small], scores=False)
    for label, batch, at in (("beside 3072 observations", [small, w3072], 0), ("beside 3073 observations", [small, w3073], 0),
                             ("before 1025 tracks", [small, w1025], 0), ("behind 1025 tracks", [w1025, small], 1), ("beside 1024 tracks", [w1024, small], 1)):
        res = check_against_oracle(gpu_ctx, oracle, batch, scores=False)
        assert res[at][0].tobytes() == alone[0].tobytes() and res[at][1].tobytes() == alone[1].tobytes(), label
    w600 = K.plain_window(24, 600, nobs=4)
    (a,) = check_against_oracle(gpu_ctx, oracle, [w600], scores=False)
    b = check_against_oracle(gpu_ctx, oracle, [w600, w1025], scores=False)[0]
    same = a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    print("600 tracks, items kernel vs 256-thread kernel: %s (largest |difference of inverse depth| = %.3g)"
          % ("same bytes" if same else "bytes differ", np.abs(1.0 / a[0] - 1.0 / b[0]).max()))


@pytest.mark.parametrize("case", list(K.optimiser_cases()))
def test_refinement_as_an_optimiser(gpu_ctx, oracle, case):
    """Independent of the restated trust-region loop, on EVERY window of the case families -- the whole parallax sweep, the pure rotation (gradient
    tolerance at iteration 0), the mixed window, both hostile windows (five invalid steps; the runaway start), and the limit windows on the kernel the
    dispatch gives them, a 600-track window on both kernels:

    (1) the 50-digit Cauchy cost sum_f sum_j 1/2 log(1 + |w r_fj|^2) of the window at the returned inverse depths is <= the cost at the ones the
    refinement started from (the linear step's, or the given depths).  Only tracks whose depth is not finite (the point at infinity) are left out.

    (2) A window that stops on the function tolerance stops at an x whose trust-region candidate lowers the cost by D_LM <= 1e-6 cost.  Per track that
    candidate is s = -g / h' with g = sum rho' J.r, h' = (1 + 1 / radius) sum rho' J.J.  With H the exact second derivative of the track's cost and
    rho = H / h', the cost's quadratic model gives the candidate the decrease g^2 / h' (1 - rho / 2) and an exact Newton step -g / H the decrease
    g^2 / (2 H), so Newton gains 1 / (rho (2 - rho)) times what the candidate gains -- more when Gauss-Newton over- or under-estimates the curvature.
    Summed over tracks: D_Newton <= max_f 1 / (rho_f (2 - rho_f)) * D_LM <= K * 1e-6 * cost; the test allows 1.5 K for the model's cubic remainder and
    requires 0 < rho_f < 2 and K <= 10 so that the bound says something.  (Oracle, CPU: D_LM / cost = 3e-7 .. 9e-7, D_Newton / cost = 4e-7 .. 4e-6 with
    K = 1.3 .. 4.7.)  Which exit a window took and its final radius come from the oracle, which the GPU matches at 1e-9 in this very test.  The bound is
    applied to every window of at most K.NEWTON_MAX_TRACKS tracks whose exit is the function tolerance; test_several_windows_stop_on_the_function_tolerance
    keeps that from being none."""
    mp, mpf = R.mp, R.mpf
    batch, at = K.optimiser_cases()[case]
    w = batch[at]
    d1, flag = check_against_oracle(gpu_ctx, oracle, batch, scores=False)[at]
    g0, _ = gpu_ctx.triangulate(batch, np.concatenate([v["depth0"] for v in batch]), refine_iters=-1)
    o = sum(len(v["trk_start"]) for v in batch[:at])
    d0 = g0[o:o + len(w["trk_start"])]
    info = np.zeros(3)
    with np.errstate(all="ignore"):
        K.oracle_triangulate(oracle, w, info=info)
    cams = R.cameras(w)
    n = np.diff(w["trk_off"])
    used = [f for f in range(len(n)) if n[f] >= 3 and np.isfinite(d0[f]) and np.isfinite(d1[f])]
    assert len(used) >= (n >= 3).sum() - 1
    c0 = {f: R.cauchy_cost(w, f, 1.0 / d0[f], cams=cams) for f in used}
    c1 = {f: R.cauchy_cost(w, f, 1.0 / d1[f], cams=cams) for f in used}
    cost0, cost1 = sum(c0.values()), sum(c1.values())
    print("%s: cost %.6g -> %.6g, oracle exit %d after %d iterations" % (case, float(cost0), float(cost1), info[0], info[1]))
    assert cost1 <= cost0
    if info[0] != 4 or len(n) > K.NEWTON_MAX_TRACKS:
        return
    d_lm = d_newton = mpf(0)
    k_max = mpf(1)
    for f in used:
        x = mpf(1.0 / d1[f])
        g, h = R.gauss_newton_terms(w, f, x, cams=cams)
        if h == 0:
            continue                                        # no residual block (only frame window_size beside the anchor)
        hp = h * (1 + 1 / mpf(info[2]))
        H = mp.diff(lambda t: R.cauchy_cost(w, f, t, cams=cams), x, 2)
        rho = H / hp
        assert 0 < rho < 2, (f, rho)
        k_max = max(k_max, 1 / (rho * (2 - rho)))
        d_lm += c1[f] - R.cauchy_cost(w, f, x - g / hp, cams=cams)
        d_newton += max(mpf(0), c1[f] - R.cauchy_cost(w, f, x - g / H, cams=cams))
    print("%s: D_LM / cost = %.3g, D_Newton / cost = %.3g, K = %.3g" % (case, float(d_lm / cost1), float(d_newton / cost1), float(k_max)))
    assert k_max <= 10
    assert d_lm <= 1e-6 * cost1 * (1 + 1e-6)
    assert d_newton <= 1.5 * k_max * 1e-6 * cost1


def test_several_windows_stop_on_the_function_tolerance(oracle):
    """the Newton-step bound of test_refinement_as_an_optimiser applies to the windows of <= K.NEWTON_MAX_TRACKS tracks that leave the loop on the function
    tolerance: at least five of the cases do, low-parallax ones among them, and the other exits (gradient tolerance, five invalid steps) occur too"""
    exits = {}
    for name, (batch, at) in K.optimiser_cases().items():
        if len(batch[at]["trk_start"]) <= K.NEWTON_MAX_TRACKS:
            info = np.zeros(3)
            with np.errstate(all="ignore"):
                K.oracle_triangulate(oracle, batch[at], info=info)
            exits[name] = int(info[0])
    assert sum(e == 4 for e in exits.values()) >= 5, exits
    assert exits["parallax 0.001"] == 4 and exits["parallax 0.0001"] == 4 and exits["rotation"] == 0 and exits["hostile with infinity"] == 2, exits


def test_outlier_scores_with_bad_depths(gpu_ctx, oracle):
    """depth -1 (a rejected track), 0, negative, tiny and huge depths, and a depth that puts the reprojected z of one observation at ~0: the score is
    whatever the division gives, equal to the oracle's (1e-6 relative), NaN where it has NaN, inf where it has inf."""
    w = K.plain_window(44, 48)
    dep = np.tile([-1.0, 0.0, -7.5, 1e-9, 1e9, 12.0], 8)
    (Ra, ta), (Rb, tb) = K.camera(w, int(w["trk_start"][5])), K.camera(w, int(w["trk_start"][5]) + 1)
    p = np.append(w["trk_pts"][w["trk_off"][5]], 1.0)
    dep[5] = -(Rb.T @ (ta - tb))[2] / (Rb.T @ Ra @ p)[2]               # z in the next frame = 0 up to rounding
    with np.errstate(all="ignore"):
        sc = K.oracle_scores(oracle, w, dep)
    got = gpu_ctx.outlier_scores([K.empty_window(), w], dep)
    assert np.array_equal(np.isnan(got), np.isnan(sc)) and np.array_equal(np.isinf(got), np.isinf(sc))
    fin = np.isfinite(sc)
    assert (np.abs(got[fin] - sc[fin]) <= 1e-6 * np.maximum(1.0, np.abs(sc[fin]))).all()
    # and against the plain reference where it is defined
    cams = R.cameras(w)
    for f in (0, 2, 3, 4, 11):
        ref = float(R.outlier_score(w, f, dep[f], cams=cams))
        assert abs(got[f] - ref) <= 1e-6 * max(1.0, abs(ref))


def test_shift_depth_edges(gpu_ctx, oracle):
    """negative input depths, shifted z on both sides of 0 and at 0 up to rounding (-1 for every z <= 0), n == 0, and a batch with empty first and last
    windows whose bytes equal the single calls'"""
    a = K.shift_case()
    got, want = gpu_ctx.shift_depth(*a), oracle.shift_depth(*a)
    assert (want == -1.0).sum() >= 4 and (want > 0).sum() >= 10
    for k in range(len(want)):
        if k in (4, 5):
            assert got[k] == -1.0 or 0 < got[k] < 1e-12
        else:
            assert abs(got[k] - want[k]) <= 1e-12 * np.abs(want).max()
            ref = float(R.shifted_depth(*a[:5], a[5][k], a[6][k]))
            assert abs(got[k] - ref) <= 1e-12 * max(1.0, abs(ref))
    assert len(gpu_ctx.shift_depth(*a[:5], np.zeros((0, 2)), np.zeros(0))) == 0
    b = K.shift_case(seed=6, n=150)
    frame = lambda c: np.concatenate([np.ravel(v) for v in c[:5]])
    z = np.zeros((0, 2))
    got = gpu_ctx.shift_depth_batch([frame(a), frame(a), frame(b), frame(b), frame(a)], [z, a[5], z, b[5], z], [z[:, 0], a[6], z[:, 0], b[6], z[:, 0]])
    assert [len(g) for g in got] == [0, len(a[6]), 0, len(b[6]), 0]
    assert got[1].tobytes() == gpu_ctx.shift_depth(*a).tobytes() and got[3].tobytes() == gpu_ctx.shift_depth(*b).tobytes()
    assert all(len(g) == 0 for g in gpu_ctx.shift_depth_batch([frame(a), frame(b)], [z, z], [z[:, 0], z[:, 0]]))


def test_malformed_descriptors_are_refused(gpu_ctx):
    """LMONO_EINVAL, a message, and untouched outputs for every structural error (include/lmono_hip.h lists them).  Host-side: the library validates before
    it uploads or launches anything, so nothing malformed reaches a kernel; the same calls go through the CPU twin in tests/test_feat_ref_cpu.py."""
    K.check_malformed_refused(gpu_ctx.L, gpu_ctx.h, [K.mixed_window(), K.hostile_window(False)])
    assert "offsets" in gpu_ctx.last_error()
    p = K.pack([K.mixed_window(), K.hostile_window(False)])
    F = int(p["feat_off"][-1])
    depth = np.full(F, -1.0); flag = np.zeros(F, np.int32)
    assert K.raw_triangulate(gpu_ctx.L, gpu_ctx.h, p, depth, flag, refine_iters=1001) == K.EINVAL and "refine_max_iter" in gpu_ctx.last_error()
    assert K.raw_triangulate(gpu_ctx.L, gpu_ctx.h, p, depth, flag, refine_iters=1000) == 0
