"""The restatement of the tracker's epipolar rejection (tests/track_reject_ref.py) pinned to things that are
not the restatement: synthetic 3-D correspondences with known outliers, numpy's SVD 8-point fit, the definition of the sample
stream, degenerate inputs and the movers of workloads/s6.py.  No GPU."""
import numpy as np
import pytest

from tests import track_ref as R
from tests import track_reject_ref as RR
from workloads import s6

W, H, FX = 1241, 376, 718.0
DIST = (-0.28, 0.07, 2e-4, -3e-4)
LOOSE, TIGHT = (1.0, 0.5), (0.15, 0.15)

# Recorded on the restatement: inlier retention with (0.15, 0.15) over seeds 0..7, both cameras, forward motion;
# the assertion is the recorded minimum minus 5 points
TIGHT_RETENTION_MIN = {30: 1.0, 150: 0.9917, 512: 0.9805}
# Recorded on the restatement over the 20-frame s6 sequence with (1.0, 0.5); the assertion is 2 x the recorded miss / loss share
S6_MOVER_MISS = 0.2308
S6_STATIC_LOSS = 0.0135
S6_BOUNDARY_CAP = 0.30


def camera(dist):
    return R.Camera(W, H, FX, FX, 620.5, 188.0, *(dist if dist else (0.0, 0.0, 0.0, 0.0)))


def project(cam, xn):
    """Normalised points [n, 2] -> pixels through the camera's own distortion (PinholeCamera::spaceToPlane)."""
    out = np.zeros_like(xn)
    for i, (x, y) in enumerate(xn):
        dx, dy = cam._distortion(x, y) if cam.distort else (0.0, 0.0)
        out[i] = (cam.fx * (x + dx) + cam.cx, cam.fy * (y + dy) + cam.cy)
    return out


def correspondences(m, seed, dist=None, sideways=False, outlier_share=0.2, noise=0.03):
    """-> (cam, prev_px [m, 2] fp32, cur_px [m, 2] fp32, outlier [m] bool).  Points at 6-50 m seen from two poses: 0.8 m forward
    plus 0.01 rad yaw, or 0.8 m sideways.  Every outlier is displaced perpendicular to its true epipolar line by 3-30 px (a
    displacement along the line cannot be detected by any epipolar test)."""
    rng = np.random.default_rng(seed)
    cam = camera(dist)
    Z = rng.uniform(6.0, 50.0, m)
    xn = np.stack([rng.uniform(-0.78, 0.78, m), rng.uniform(-0.22, 0.22, m)], 1)
    X = np.hstack([xn * Z[:, None], Z[:, None]])
    yaw = 0.0 if sideways else 0.01
    t = np.array([0.8, 0.0, 0.0]) if sideways else np.array([0.0, 0.0, 0.8])
    Rm = np.array([[np.cos(yaw), 0.0, np.sin(yaw)], [0.0, 1.0, 0.0], [-np.sin(yaw), 0.0, np.cos(yaw)]])

    def cur_of(P):
        Q = (P - t) @ Rm
        return Q[:, :2] / Q[:, 2:3]
    cn = cur_of(X)
    line = cur_of(np.hstack([xn * 3.0, np.full((m, 1), 3.0)])) - cur_of(np.hstack([xn * 500.0, np.full((m, 1), 500.0)]))   # along the epipolar line
    perp = np.stack([-line[:, 1], line[:, 0]], 1) / np.sqrt((line * line).sum(1))[:, None]
    n_out = int(round(outlier_share * m))
    outlier = np.zeros(m, bool)
    outlier[rng.permutation(m)[:n_out]] = True
    off = rng.uniform(3.0, 30.0, m) * rng.choice([-1.0, 1.0], m) / FX
    cn = cn + np.where(outlier[:, None], perp * off[:, None], 0.0)
    prev_px = project(cam, xn) + rng.normal(0.0, noise, (m, 2))
    cur_px = project(cam, cn) + rng.normal(0.0, noise, (m, 2))
    return cam, prev_px.astype(np.float32), cur_px.astype(np.float32), outlier


def run(m, seed, dist, sideways, thr, n_hyp=256):
    cam, p, c, outlier = correspondences(m, seed, dist, sideways)
    inlier = ~outlier
    assert outlier.sum() + inlier.sum() == m and not (outlier & inlier).any()           # one class each, none left out
    status, stats, F = RR.reject(cam, p, c, RR.RejectParams(thr[0], thr[1], n_hyp=n_hyp, seed=seed), seed)
    kept = status.astype(bool)
    return int((kept & outlier).sum()), float((kept & inlier).sum()) / float(inlier.sum()), stats, F


@pytest.mark.parametrize("dist", [None, DIST])
@pytest.mark.parametrize("sideways", [False, True])
@pytest.mark.parametrize("m", [30, 150, 512])
def test_loose_thresholds_drop_every_outlier(m, dist, sideways):
    for seed in range(3):
        out_kept, retention, stats, _ = run(m, seed, dist, sideways, LOOSE)
        print("m %d dist %s sideways %s seed %d: outliers kept %d, inlier retention %.4f, stats %s" % (m, bool(dist), sideways, seed, out_kept, retention, stats))
        assert out_kept == 0
        assert retention >= 0.95


@pytest.mark.parametrize("dist", [None, DIST])
@pytest.mark.parametrize("m", [30, 150, 512])
def test_tight_thresholds_retention(m, dist):
    worst = 1.0
    for seed in range(8):
        out_kept, retention, stats, _ = run(m, seed, dist, False, TIGHT)
        print("m %d dist %s seed %d: outliers kept %d, inlier retention %.4f, stats %s" % (m, bool(dist), seed, out_kept, retention, stats))
        assert out_kept == 0
        worst = min(worst, retention)
    print("m %d dist %s: minimum retention %.4f (recorded %.4f)" % (m, bool(dist), worst, TIGHT_RETENTION_MIN[m]))
    assert worst >= TIGHT_RETENTION_MIN[m] - 0.05


def _numpy_eight_point(P):
    """Hartley-normalised 8-point fit with np.linalg.svd and the SVD rank-2 projection, prev^T F cur = 0."""
    def norm(x):
        mu = x.mean(0); s = np.sqrt(2.0) / np.sqrt(((x - mu) ** 2).sum(1)).mean()
        return (x - mu) * s, np.array([[s, 0, -s * mu[0]], [0, s, -s * mu[1]], [0, 0, 1.0]])
    p, Tp = norm(P[:, :2]); c, Tc = norm(P[:, 2:])
    A = np.stack([p[:, 0] * c[:, 0], p[:, 0] * c[:, 1], p[:, 0], p[:, 1] * c[:, 0], p[:, 1] * c[:, 1], p[:, 1], c[:, 0], c[:, 1], np.ones(len(P))], 1)
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return Tp.T @ Fn @ Tc


@pytest.mark.parametrize("dist", [None, DIST])
@pytest.mark.parametrize("sideways", [False, True])
@pytest.mark.parametrize("m", [30, 150, 512])
def test_refit_against_numpy_svd(m, dist, sideways):
    cam, p, c, outlier = correspondences(m, 11, dist, sideways)
    prm = RR.RejectParams(*LOOSE)
    Pd = np.hstack([RR.lift_virtual(cam, p, prm.focal_length), RR.lift_virtual(cam, c, prm.focal_length)])
    P1 = RR.g1(Pd)[~outlier]
    info = {}
    F = RR.refit(P1, info=info).reshape(3, 3)
    Fnp = _numpy_eight_point(P1)
    cosine = abs((F / np.linalg.norm(F) * Fnp / np.linalg.norm(Fnp)).sum())
    sv = np.linalg.svd(F, compute_uv=False)
    print("m %d dist %s sideways %s: |<F, F_np>| = 1 - %.3e, sigma_min / sigma_max %.3e, Jacobi off-diagonal / trace %.3e after %d sweeps"
          % (m, bool(dist), sideways, 1.0 - cosine, sv[2] / sv[0], info["offdiag"] / info["trace"], RR.SWEEPS))
    assert info["offdiag"] <= 1e-14 * info["trace"]
    assert cosine >= 1.0 - 1e-9
    assert sv[2] <= 1e-12 * sv[0]


@pytest.mark.parametrize("m", [8, 9, 150, 512])
def test_sampler(m):
    idx, ok = RR.sample(5, 3, 256, m)
    assert ok.all()
    assert idx.min() >= 0 and idx.max() < m
    assert all(len(set(row)) == 8 for row in idx.tolist())
    again, _ = RR.sample(5, 3, 256, m)
    assert np.array_equal(idx, again)
    nxt, _ = RR.sample(5, 4, 256, m)
    assert not np.array_equal(idx, nxt)
    if m > 8:
        assert (np.sort(idx, 1) != np.sort(nxt, 1)).any()
    # the generator as written in DESIGN.md 6e, on Python integers
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; x ^= x >> 16
        return x
    for h in (0, 17, 255):
        key = mix(mix(mix(5 ^ 0x9e3779b9) ^ 3) ^ h)
        want, d = [], 0
        while len(want) < 8:
            c = (mix(key ^ d) * m) >> 32
            d += 1
            if c not in want:
                want.append(c)
        assert idx[h].tolist() == want


def test_degenerate_inputs():
    cam = camera(None)
    prm = RR.RejectParams(*LOOSE)
    # all points identical: no hypothesis has a non-zero mean distance -> all dropped, nothing undefined in the status
    p = np.tile(np.array([[300.0, 200.0]], np.float32), (20, 1))
    status, stats, F = RR.reject(cam, p, p + np.float32(1.0), prm, 0)
    assert status.dtype == np.uint8 and (status == 0).all() and stats.tolist() == [0, -1, 0, 0] and np.isfinite(F).all()
    # seven pairs: the step does not run
    cam2, pp, cc, _ = correspondences(7, 0)
    status, stats, _ = RR.reject(cam2, pp, cc, prm, 0)
    assert (status == 1).all() and stats.tolist() == [-1, -1, -1, -1]
    # a planar scene: F is not unique, and all this documents is that the inliers of the plane are kept
    rng = np.random.default_rng(3)
    xn = np.stack([rng.uniform(-0.7, 0.7, 120), rng.uniform(-0.2, 0.2, 120)], 1)
    X = np.hstack([xn * 12.0, np.full((120, 1), 12.0)])
    Q = X - np.array([0.3, 0.0, 0.8])
    pp = (project(cam, xn) + rng.normal(0, 0.03, (120, 2))).astype(np.float32)
    cc = (project(cam, Q[:, :2] / Q[:, 2:3]) + rng.normal(0, 0.03, (120, 2))).astype(np.float32)
    status, stats, _ = RR.reject(cam, pp, cc, prm, 0)
    print("planar scene: kept %d of 120, stats %s" % (status.sum(), stats))
    assert status.sum() >= 0.95 * 120


def s6_sequence():
    return s6.Sequence(640, 480, 20, seed=2)


def s6_camera():
    return R.Camera(640, 480, 460.0, 460.0, 319.5, 239.5)


def s6_rates(seq, tracker_factory):
    """Runs a tracker with rejection on over the sequence.  -> dict of counts: points entering the step per class, static
    interior points kept by it, mover interior tracks that appeared and how many of them were gone two frames later."""
    trk = tracker_factory()
    entering = {s6.STATIC: 0, s6.MOVER: 0, s6.BOUNDARY: 0}
    static_kept = 0
    born = {}                                   # id -> (frame of appearance, class there)
    alive = {}                                  # id -> last frame seen
    prev = None
    for k in range(seq.n_frames):
        rec = trk.track(0.1 * k, seq.frames[k])
        ids = set(int(i) for i in rec["id"])
        if prev is not None:
            # the points entering the step at frame k are the previous frame's points that passed the KLT tests; the restatement
            # exposes them through last_status; the classes are taken at the previous frame's positions
            cls = seq.class_of(k - 1, np.stack([prev["u"], prev["v"]], 1))
            entered = trk.last_entered
            for i, r in enumerate(prev):
                if not entered[i]:
                    continue
                entering[int(cls[i])] += 1
                if cls[i] == s6.STATIC and int(r["id"]) in ids:
                    static_kept += 1
        for r in rec:
            i = int(r["id"])
            if i not in born:
                born[i] = (k, int(seq.class_of(k, [[r["u"], r["v"]]])[0]))
            alive[i] = k
        prev = rec
    movers = [i for i, (k, c) in born.items() if c == s6.MOVER and k + 2 < seq.n_frames]
    gone = [i for i in movers if alive[i] < born[i][0] + 2]
    return dict(entering=entering, static_kept=static_kept, movers=len(movers), movers_gone=len(gone))


class _Entered(RR.TrackerRejectRef):
    """TrackerRejectRef that also remembers which of the previous frame's points reached the rejection step."""

    def track(self, time, image):
        rec = super().track(time, image)
        self.last_entered = self.last_status if self.last_status is not None else np.zeros(0, bool)
        return rec


def test_s6_movers_are_dropped_and_static_points_kept():
    seq = s6_sequence()
    r = s6_rates(seq, lambda: _Entered(s6_camera(), 150, 15, reject=RR.RejectParams(*LOOSE)))
    total = sum(r["entering"].values())
    boundary_share = r["entering"][s6.BOUNDARY] / float(total)
    miss = 1.0 - r["movers_gone"] / float(r["movers"])
    # static points can also leave through setMask; the loss asserted here is the loss of the frame as a whole, an upper bound
    loss = 1.0 - r["static_kept"] / float(r["entering"][s6.STATIC])
    print("s6: entering %s, boundary share %.3f, mover interior tracks %d, gone within two frames %d (miss %.4f), static interior loss %.4f"
          % (r["entering"], boundary_share, r["movers"], r["movers_gone"], miss, loss))
    assert r["movers"] >= 10 and r["entering"][s6.STATIC] >= 500
    assert boundary_share <= S6_BOUNDARY_CAP
    assert miss <= 2.0 * S6_MOVER_MISS
    assert loss <= 2.0 * S6_STATIC_LOSS
    # without the step the movers stay: the forward-backward test does not see them
    r0 = s6_rates(seq, lambda: _Entered(s6_camera(), 150, 15, reject=None))
    print("s6 without the step: mover interior tracks %d, gone within two frames %d" % (r0["movers"], r0["movers_gone"]))
    assert r0["movers_gone"] <= 0.5 * r0["movers"]
