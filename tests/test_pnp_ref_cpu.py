"""The restatement of the loop verification (tests/pnp_ref.py) against things that are not the restatement: a synthetic
scene with known outliers, scipy's least squares, the sample stream's stated properties, degenerate inputs, the gates at their
boundaries, a direct computation of loop_info -- and the host build of the kernel file's arithmetic (pnp_test) by bytes.  No GPU."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pnp_cases as S
from tests import pnp_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNP_TEST = os.path.join(ROOT, "lmono_amd", "host", "pnp_test")

RETENTION_MIN = 1.0          # the lowest inlier retention over the 80 scenes below
RETENTION_MARGIN = 0.05
REFIT_RECORD = 2.4e-9        # the largest |pose - scipy's| over the refit scenes below


@pytest.mark.parametrize("share", [0.25, 0.5])
@pytest.mark.parametrize("m", [4, 5, 26, 150, 512])
def test_outliers_dropped_and_inliers_kept(m, share):
    """Seeds 0..7, none skipped.  m = 4 has one distinct sample, so nothing rescues a sample outside the iteration's basin (about one
    sample in five lies outside it at the full 30 degrees / 20 m): its guess is drawn within a quarter of the gates
    (seed 6 of this scene fails at half of them).  m <= 5 has no outliers at either share: one outlier among five leaves one all-inlier sample,
    which a contaminated sample that fits its own four points can tie (measured)."""
    for seed in range(8):
        p3, p2, g, truth, out = S.scene(m, 1000 * m + seed, share, gate_share=0.25 if m == 4 else 1.0)
        st, pose, stats = P.pnp_ransac(p3, p2, g, seed, P.PnPParams(seed=seed))
        st = st.astype(bool)
        retention = st[~out].mean()
        print("m %d share %.2f seed %d: stats %s, outliers kept %d, retention %.3f, |t - truth| %.3g" %
              (m, share, seed, stats.tolist(), int((st & out).sum()), retention, np.abs(pose[:3] - truth[:3]).max()))
        assert stats[0] > 0 and stats[2] == st.sum() >= 4 and stats[3] == P.ITERS
        assert not (st & out).any(), "an outlier was kept"
        assert retention >= RETENTION_MIN - RETENTION_MARGIN


def _residual(x, pd, t0, q0):
    t, q = P.update(t0.copy(), q0.copy(), list(x))
    p = pd[:, :3] @ P.rot_matrix(q).T + t
    return np.concatenate([p[:, 0] / p[:, 2] - pd[:, 3], p[:, 1] / p[:, 2] - pd[:, 4]])


def _least_squares(pd, t0, q0):
    """scipy.optimize.least_squares on the same residual, or, without scipy, numpy Gauss-Newton (finite-difference Jacobian, lstsq) run
    to stagnation.  -> (t, q, which ran)"""
    try:
        from scipy.optimize import least_squares
        r = least_squares(_residual, np.zeros(6), args=(pd, t0, q0), xtol=1e-15, ftol=1e-15, gtol=1e-15)
        t, q = P.update(t0.copy(), q0.copy(), list(r.x))
        return t, q, "scipy"
    except ImportError:
        t, q = t0.copy(), q0.copy()
        for _ in range(50):
            r0 = _residual(np.zeros(6), pd, t, q)
            J = np.stack([(_residual(np.eye(6)[k] * 1e-7, pd, t, q) - r0) / 1e-7 for k in range(6)], 1)
            dx = np.linalg.lstsq(J, -r0, rcond=None)[0]
            t, q = P.update(t, q, list(dx))
            if np.abs(dx).max() < 1e-13:
                break
        return t, q, "numpy Gauss-Newton"


@pytest.mark.parametrize("m", [26, 150, 512])
def test_refit_against_least_squares(m):
    worst, which = 0.0, ""
    for seed in range(8):
        p3, p2, g, _, _ = S.scene(m, 1000 * m + seed, 0.25)
        st, pose, stats = P.pnp_ransac(p3, p2, g, seed, P.PnPParams(seed=seed))
        pd = np.concatenate([p3.astype(np.float64), p2.astype(np.float64)], 1)
        idx, _ = P.sample(seed, seed, 256, m)
        t, q, _ = P.solve4(pd, idx, g)
        ts, qs, which = _least_squares(pd[st.astype(bool)], t[stats[1]], q[stats[1]])      # the same inliers, the same start
        if qs @ pose[3:] < 0:
            qs = -qs
        worst = max(worst, np.abs(ts - pose[:3]).max(), np.abs(qs - pose[3:]).max())
    print("m %d: max |pose - %s| = %.3g" % (m, which, worst))
    assert worst < 10 * REFIT_RECORD


@pytest.mark.parametrize("m", [4, 5, 65, 512])
def test_sampler(m):
    idx, ok = P.sample(7, 99, 1024, m)
    assert ok.all() and (idx >= 0).all() and (idx < m).all()
    assert all(len(set(row)) == 4 for row in idx.tolist()), "indices of a sample repeat"
    # the redraw rule, hypothesis by hypothesis: draws in order, a repeat is skipped
    keys = P.hyp_keys(7, 99, 1024)
    for h in (0, 1, 511, 1023):
        want, d = [], 0
        while len(want) < 4:
            c = int((int(P.mix(np.uint64(int(keys[h]) ^ d))) * m) >> 32)
            d += 1
            if c not in want:
                want.append(c)
        assert idx[h].tolist() == want
    # reproducible, and a function of (seed, key, h) alone: a shorter run is a prefix, another key or seed another stream
    again, _ = P.sample(7, 99, 100, m)
    assert (again == idx[:100]).all()
    if m > 4:
        assert (P.sample(7, 98, 1024, m)[0] != idx).any() and (P.sample(8, 99, 1024, m)[0] != idx).any()
    assert P.caller_key(3, 5) == (3 << 16 | 5) and P.caller_key(65535, 65535) == 0xFFFFFFFF


def test_result_does_not_depend_on_anything_but_the_problem_and_its_key():
    p3, p2, g, _, _ = S.scene(65, 3, 0.25)
    a = P.pnp_ransac(p3, p2, g, 12, P.PnPParams(seed=2)); b = P.pnp_ransac(p3.copy(), p2.copy(), g.copy(), 12, P.PnPParams(seed=2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = P.pnp_ransac(p3, p2, g, 13, P.PnPParams(seed=2))
    assert c[2][1] != a[2][1] or c[1].tobytes() != a[1].tobytes(), "another key drew the same samples"


@pytest.mark.parametrize("name", list(S.degenerate_cases()))
def test_degenerate_inputs(name):
    p3, p2, g = S.degenerate_cases()[name]
    st, pose, stats = P.pnp_ransac(p3, p2, g, 1)
    print(name, stats.tolist())
    assert not st.any() and pose.tobytes() == g.tobytes(), "the failure output is status all 0 and the guess unchanged"
    if len(p3) < 4:
        assert (stats == -1).all()
    else:
        assert stats[3] == 0 and (stats[0] == 0 or stats[2] < 4)


def test_one_nan_observation_is_no_inlier():
    p3, p2, g, _, _ = S.scene(65, 11, 0.0)
    p2[7, 0] = np.nan
    st, pose, stats = P.pnp_ransac(p3, p2, g, 1)
    assert st[7] == 0 and st.sum() == 64 and np.isfinite(pose).all() and stats[0] < 256


def _direct(pose, vio, ex, old, cur):
    """loop_info and the 15-value channel straight from KeyFrame.cc:341-350, :572-575, :658-682 with 3 x 3 matrices."""
    def Rq(q):
        x, y, z, w = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    R_wc_old = Rq(pose[3:]).T
    T_wc_old = R_wc_old @ (-pose[:3])
    R_old = R_wc_old @ Rq(ex[3:]).T
    T_old = T_wc_old - R_old @ ex[:3]
    rel_t = R_old.T @ (vio[:3] - T_old); rel_R = R_old.T @ Rq(vio[3:])
    yaw = lambda R: math.degrees(math.atan2(R[1, 0], R[0, 0]))
    rel_yaw = (yaw(Rq(vio[3:])) - yaw(R_old) + 180.0) % 360.0 - 180.0
    return T_old, R_old, rel_t, rel_R, rel_yaw, Rq(old[3:]) @ rel_t + old[:3], Rq(old[3:]) @ rel_R


def test_loop_info_and_channel_against_direct_computation():
    rng = np.random.default_rng(3)
    for _ in range(20):
        mk = lambda a, t: np.concatenate([rng.uniform(-t, t, 3), S.quat_axis_angle(rng.normal(size=3), rng.uniform(0, a))])
        pose, vio, ex, old = mk(3.0, 30), mk(3.0, 30), mk(1.0, 1), mk(3.0, 30)
        r = P.after_pnp(pose, 30, 10, vio, ex, old, cur_index=41)
        T_old, R_old, rel_t, rel_R, rel_yaw, cT, cR = _direct(pose, vio, ex, old, 41)
        assert np.abs(r["pnp_t_old"] - T_old).max() < 1e-12 and np.abs(P.rot_matrix(r["pnp_q_old"]) - R_old).max() < 1e-12
        li, ch = r["loop_info"], r["channel"]
        assert np.abs(li[:3] - rel_t).max() < 1e-12
        assert np.abs(P.rot_matrix([li[4], li[5], li[6], li[3]]) - rel_R).max() < 1e-12, "relative_q is stored w x y z"
        assert abs((li[7] - rel_yaw + 180.0) % 360.0 - 180.0) < 1e-9 and -180.0 <= li[7] <= 180.0
        assert np.abs(ch[:3] - old[:3]).max() == 0 and np.abs(ch[3:7] - old[[6, 3, 4, 5]]).max() == 0 and ch[14] == 41.0
        assert np.abs(ch[7:10] - cT).max() < 1e-11 and np.abs(P.rot_matrix([ch[11], ch[12], ch[13], ch[10]]) - cR).max() < 1e-12


def test_gates_at_their_boundaries():
    ident = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    vio = np.concatenate([[3.0, -4.0, 1.0], S.quat_axis_angle([0.2, 0.3, 1.0], math.radians(12.0))])
    pose = P.guess_from_vio(ident, ident)
    go = lambda nb, ni, **kw: P.after_pnp(pose, nb, ni, vio, ident, params=P.PnPParams(**kw))["has_loop"]
    assert go(26, 6) and not go(26, 5) and not go(25, 6), "both count gates are strict"
    assert go(11, 3, min_brief_loop_num=10, min_pnp_loop_num=2) and not go(10, 3, min_brief_loop_num=10, min_pnp_loop_num=2)
    r = P.after_pnp(pose, 26, 6, vio, ident)
    tn = math.sqrt(float(r["relative_t"] @ r["relative_t"])); en = math.sqrt(float(r["relative_euler"] @ r["relative_euler"]))
    assert abs(tn - math.sqrt(26.0)) < 1e-12 and 11.0 < en < 13.0
    assert go(26, 6, trans_threshold=tn * (1 + 1e-12)) and not go(26, 6, trans_threshold=tn), "|relative_t| < TRANS_THRESHOLD is strict"
    assert go(26, 6, angle_threshold=en * (1 + 1e-12)) and not go(26, 6, angle_threshold=en), "|relative_euler| < ANGLE_THRESHOLD is strict"


def test_guess_is_the_inverse_of_the_camera_pose():
    vio = np.concatenate([[3.0, -4.0, 1.0], S.quat_axis_angle([0.2, 0.3, 1.0], 0.4)]); ex = np.concatenate([[0.1, 0.2, -0.3], S.quat_axis_angle([1.0, 0.1, 0.0], 1.2)])
    g = P.guess_from_vio(vio, ex)
    R_wc = P.rot_matrix(vio[3:]) @ P.rot_matrix(ex[3:]); T_wc = vio[:3] + P.rot_matrix(vio[3:]) @ ex[:3]
    assert np.abs(P.rot_matrix(g[3:]) - R_wc.T).max() < 1e-14 and np.abs(g[:3] + R_wc.T @ T_wc).max() < 1e-14
    # and after_pnp of the guess gives the VIO pose back: relative_t = 0, relative_q = identity
    r = P.after_pnp(g, 30, 10, vio, ex)
    assert np.abs(r["relative_t"]).max() < 1e-13 and abs(abs(r["relative_q"][3]) - 1.0) < 1e-14 and abs(r["relative_yaw"]) < 1e-10


def write_problems(path, problems):
    """The input format of lmono_amd/host/pnp_test: (points_3d, points_2d, guess, key, n_hyp, seed, threshold) each."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(problems)))
        for p3, p2, g, key, n_hyp, seed, thr in problems:
            f.write(struct.pack("<iIiId", len(p3), key, n_hyp, seed, thr))
            f.write(np.asarray(g, np.float64).tobytes()); f.write(np.asarray(p3, np.float32).tobytes()); f.write(np.asarray(p2, np.float32).tobytes())


def read_results(path, problems):
    buf, at, out = open(path, "rb").read(), 0, []
    for p in problems:
        m = len(p[0])
        st = np.frombuffer(buf, np.uint8, m, at); at += m
        stats = np.frombuffer(buf, np.int32, 4, at); at += 16
        pose = np.frombuffer(buf, np.float64, 7, at); at += 56
        out.append((st, pose, stats))
    assert at == len(buf)
    return out


def test_host_build_equals_restatement(tmp_path):
    """pnp_test (g++ -ffp-contract=off over lmono_amd/csrc/pnp.hip, built by build()) equals the restatement byte for byte."""
    assert os.path.exists(PNP_TEST), "lmono_amd/host/pnp_test is built by build()"
    problems = []
    for m in (4, 5, 65, 512):
        for n_hyp in (1, 100, 1024):
            p3, p2, g, _, _ = S.scene(m, 31 * m + n_hyp, 0.25)
            problems.append((p3, p2, g, 7 * m + n_hyp, n_hyp, 3, P.THRESHOLD))
    for name, (p3, p2, g) in S.degenerate_cases().items():
        problems.append((p3, p2, g, 1, 256, 0, P.THRESHOLD))
    write_problems(tmp_path / "problems.bin", problems)
    subprocess.run([PNP_TEST, str(tmp_path / "problems.bin"), str(tmp_path / "results.bin")], check=True, timeout=120)
    for (p3, p2, g, key, n_hyp, seed, thr), (st, pose, stats) in zip(problems, read_results(tmp_path / "results.bin", problems)):
        rs, rp, rstats = P.pnp_ransac(p3, p2, g, key, P.PnPParams(n_hyp=n_hyp, seed=seed))
        what = "m %d n_hyp %d" % (len(p3), n_hyp)
        assert stats.tolist() == rstats.tolist(), what
        assert st.tobytes() == rs.tobytes(), what + ": status"
        assert pose.tobytes() == rp.tobytes(), what + ": pose bytes"


def test_host_code_after_the_pose_equals_restatement(tmp_path):
    """pnp_test --after runs the C ABI's host code behind the pose (pnp_after, pnp_loop_info, pnp_channel of lmono_amd/csrc/pnp.hip):
    equal to after_pnp within 1e-9 (atan2 / sin / cos: no byte comparison), the threshold test included."""
    assert os.path.exists(PNP_TEST), "lmono_amd/host/pnp_test is built by build()"
    rng = np.random.default_rng(8)
    mk = lambda a, t: np.concatenate([rng.uniform(-t, t, 3), S.quat_axis_angle(rng.normal(size=3), rng.uniform(0, a))])
    recs = [(mk(3.0, 30), mk(3.0, 30), mk(1.0, 1), mk(3.0, 30), rng.uniform(5, 200), rng.uniform(1, 60), float(k)) for k in range(40)]
    with open(tmp_path / "records.bin", "wb") as f:
        f.write(struct.pack("<i", len(recs)))
        for pose, vio, ex, old, ang, tr, cur in recs:
            f.write(np.concatenate([pose, vio, ex, old, [ang, tr, cur]]).tobytes())
    subprocess.run([PNP_TEST, "--after", str(tmp_path / "records.bin"), str(tmp_path / "results.bin")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "results.bin", np.float64).reshape(len(recs), 34)
    seen = set()
    for (pose, vio, ex, old, ang, tr, cur), o in zip(recs, got):
        r = P.after_pnp(pose, 30, 10, vio, ex, old, int(cur), P.PnPParams(angle_threshold=ang, trans_threshold=tr))
        want = np.concatenate([r["pnp_t_old"], r["pnp_q_old"], r["loop_info"], r["relative_euler"], [1.0 if r["has_loop"] else 0.0], r["channel"]])
        assert np.abs(o - want).max() < 1e-9
        seen.add(r["has_loop"])
    assert seen == {True, False}, "the records exercise both sides of the threshold test"


def test_settling_row_of_the_definition():
    """The row of DESIGN.md 6g's settling table that fixes 12 steps, six of them damped (scripts/pnp_settling.py prints the whole table):
    at the full 30 degrees / 20 m, 0.799 of the samples are valid and 0.798 within 1 mm; four more steps gain nothing, undamped loses 0.09."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pnp_settling", os.path.join(ROOT, "scripts", "pnp_settling.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    valid, close = mod.settle(P.ITERS, P.DAMP)
    print("K %d damped %d: valid %.4f within 1 mm %.4f" % (P.ITERS, P.DAMP, valid, close))
    assert abs(valid - 0.799) < 0.0015 and abs(close - 0.798) < 0.0015
    assert mod.settle(16, P.DAMP)[1] - close < 0.002, "more steps would settle more samples"
    assert mod.settle(P.ITERS, 0)[1] < close - 0.05, "the damping buys nothing"
