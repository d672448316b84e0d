"""tests/track_reject_ref.py -- CPU restatement of the tracker's epipolar outlier rejection (rejectWithF),
numpy only.  Test infrastructure: k_trk_reject (lmono_amd/csrc/track_reject.hip) and this file implement one written definition,
every step one IEEE fp64 operation in the order written here, so "equal" means equal bytes.  Vectorised over hypotheses,
elementwise only: no np.linalg and no np.sum in the decision path.  TrackerRejectRef is track_ref.TrackerRef.track with the
step inserted where FeatureTracker.cc:259-262 has it."""
import math

import numpy as np

from tests import track_ref as R

F32 = np.float32
M32 = np.uint64(0xFFFFFFFF)
MAX_HYP = 1024
MAX_DRAWS = 256
SWEEPS = 7
SQRT2 = 1.4142135623730951
FOCAL_LENGTH = 460.0


class RejectParams:
    def __init__(self, f_threshold, f_dis, focal_length=FOCAL_LENGTH, n_hyp=256, seed=0):
        self.f_threshold, self.f_dis = float(f_threshold), float(f_dis)
        self.focal_length = float(focal_length) if focal_length else FOCAL_LENGTH
        self.n_hyp = int(n_hyp) if n_hyp else 256
        self.seed = int(seed) & 0xFFFFFFFF


# ---- the sample stream ----------------------------------------------------------------------------------------------------
def mix(x):
    """32-bit integer multiply / xor / shift hash of uint32 values held in uint64 arrays."""
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def hyp_keys(seed, frame, n_hyp):
    h = np.arange(n_hyp, dtype=np.uint64)
    base = mix(mix(np.uint64((seed ^ 0x9e3779b9) & 0xFFFFFFFF)) ^ np.uint64(frame & 0xFFFFFFFF))
    return mix(base ^ h)


def sample(seed, frame, n_hyp, m):
    """-> (idx [n_hyp, 8], ok [n_hyp]): 8 distinct indices below m per hypothesis; draw d is mix(key ^ d), index (r * m) >> 32,
    a repeat is redrawn with the next d; a sample still incomplete after MAX_DRAWS draws is not ok."""
    keys = hyp_keys(seed, frame, n_hyp)
    idx = np.full((n_hyp, 8), -1, np.int64)
    have = np.zeros(n_hyp, np.int64)
    for d in range(MAX_DRAWS):
        todo = have < 8
        if not todo.any():
            break
        r = mix(keys ^ np.uint64(d))
        c = ((r * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
        dup = (idx == c[:, None]).any(1)
        take = todo & ~dup
        rows = np.nonzero(take)[0]
        idx[rows, have[rows]] = c[rows]
        have[rows] += 1
    return idx, have == 8


# ---- points ---------------------------------------------------------------------------------------------------------------
def lift_virtual(cam, px, focal):
    """pixels [n, 2] fp32 -> virtual-camera points [n, 2] fp64: PINHOLE liftProjective in fp64 (not rounded), then
    focal * x + width / 2.0, focal * y + height / 2.0 (FeatureTracker.cc:441-453)."""
    px = np.asarray(px, np.float32).reshape(-1, 2)
    out = np.zeros((len(px), 2))
    for i in range(len(px)):
        mx_d = cam.ik11 * float(px[i, 0]) + cam.ik13; my_d = cam.ik22 * float(px[i, 1]) + cam.ik23
        mx_u, my_u = mx_d, my_d
        if cam.distort:
            for _ in range(8):
                dx, dy = cam._distortion(mx_u, my_u)
                mx_u, my_u = mx_d - dx, my_d - dy
        out[i, 0] = focal * mx_u + float(cam.width) / 2.0
        out[i, 1] = focal * my_u + float(cam.height) / 2.0
    return out


def g1(v):
    """What gate 1 sees: rounded once to fp32 (cv::Point2f)."""
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


# ---- F from normalised coordinates ------------------------------------------------------------------------------------------
def denorm(Fn, sp, mpx, mpy, sc, mcx, mcy):
    """F = Tp^T Fn Tc; Fn [..., 9] row-major, the rest broadcastable scalars / arrays."""
    tp0 = -(mpx * sp); tp1 = -(mpy * sp); tc0 = -(mcx * sc); tc1 = -(mcy * sc)
    G = [None] * 9
    for i in range(3):
        G[3 * i] = Fn[..., 3 * i] * sc
        G[3 * i + 1] = Fn[..., 3 * i + 1] * sc
        G[3 * i + 2] = (Fn[..., 3 * i] * tc0 + Fn[..., 3 * i + 1] * tc1) + Fn[..., 3 * i + 2]
    F = [None] * 9
    for j in range(3):
        F[j] = sp * G[j]
        F[3 + j] = sp * G[3 + j]
        F[6 + j] = (tp0 * G[j] + tp1 * G[3 + j]) + G[6 + j]
    return np.stack(np.broadcast_arrays(*F), -1)


def epi(F, px, py, cx, cy):
    """-> r^2, |l|^2 (l = F cur), |l'|^2 (l' = F^T prev); F [..., 9] broadcast against the points."""
    f = [F[..., k] for k in range(9)]
    l0 = (f[0] * cx + f[1] * cy) + f[2]; l1 = (f[3] * cx + f[4] * cy) + f[5]; l2 = (f[6] * cx + f[7] * cy) + f[8]
    r = (px * l0 + py * l1) + l2
    m0 = (f[0] * px + f[3] * py) + f[6]; m1 = (f[1] * px + f[4] * py) + f[7]
    return r * r, l0 * l0 + l1 * l1, m0 * m0 + m1 * m1


def inliers(F, P, thr2):
    """F [H, 9], P [m, 4] (gate-1 points) -> [H, m] bool: max(r^2 / |l|^2, r^2 / |l'|^2) <= thr2 (a NaN is no inlier)."""
    with np.errstate(all="ignore"):
        r2, lc, lp = epi(F[:, None, :], P[None, :, 0], P[None, :, 1], P[None, :, 2], P[None, :, 3])
        return (r2 / lc <= thr2) & (r2 / lp <= thr2)


def solve(P):
    """The minimal solve of every hypothesis at once.  P [H, 8, 4]: the sampled gate-1 points (prev X, prev Y, cur X, cur Y).
    -> (F [H, 9], valid [H])."""
    H = len(P)
    ar = np.arange(H)
    with np.errstate(all="ignore"):
        mean = np.zeros((H, 4))
        for k in range(8):
            mean = mean + P[:, k, :]
        mean = mean / 8.0
        dp = np.zeros(H); dc = np.zeros(H)
        for k in range(8):
            d = P[:, k, :] - mean
            dp = dp + np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            dc = dc + np.sqrt(d[:, 2] * d[:, 2] + d[:, 3] * d[:, 3])
        dp = dp / 8.0; dc = dc / 8.0
        valid = (dp > 0.0) & (dc > 0.0)
        sp = SQRT2 / dp; sc = SQRT2 / dc
        A = np.zeros((H, 8, 9))
        for k in range(8):
            a = (P[:, k, 0] - mean[:, 0]) * sp; b = (P[:, k, 1] - mean[:, 1]) * sp
            c = (P[:, k, 2] - mean[:, 2]) * sc; d = (P[:, k, 3] - mean[:, 3]) * sc
            A[:, k, :] = np.stack([a * c, a * d, a, b * c, b * d, b, c, d, np.ones(H)], 1)
        # Gaussian elimination with complete pivoting; rows and columns are marked, not swapped
        row_used = np.zeros((H, 8), bool); col_used = np.zeros((H, 9), bool)
        prs = np.zeros((8, H), np.int64); pcs = np.zeros((8, H), np.int64)
        for k in range(8):
            V = np.abs(A)
            V = np.where(np.isnan(V), -1.0, V)
            V = np.where(row_used[:, :, None] | col_used[:, None, :], -2.0, V).reshape(H, 72)
            flat = V.argmax(1)                          # the first maximum: ties to the lowest (row, column)
            pr, pc = flat // 9, flat % 9
            valid &= V[ar, flat] >= 1e-12
            piv = A[ar, pr, pc]
            row_used[ar, pr] = True; col_used[ar, pc] = True
            prs[k], pcs[k] = pr, pc
            f = A[ar, :, pc] / piv[:, None]
            upd = (~row_used)[:, :, None] & (~col_used)[:, None, :]
            A = np.where(upd, A - f[:, :, None] * A[ar, pr, :][:, None, :], A)
        cf = (~col_used).argmax(1)
        x = np.zeros((H, 9))
        x[ar, cf] = 1.0
        for k in range(7, -1, -1):
            acc = A[ar, prs[k], cf]
            for q in range(k + 1, 8):
                acc = acc + A[ar, prs[k], pcs[q]] * x[ar, pcs[q]]
            x[ar, pcs[k]] = -acc / A[ar, prs[k], pcs[k]]
        F = denorm(x, sp, mean[:, 0], mean[:, 1], sc, mean[:, 2], mean[:, 3])
    return F, valid


# ---- refit ------------------------------------------------------------------------------------------------------------------
def jacobi(A, sweeps=SWEEPS):
    """Cyclic Jacobi on a symmetric matrix given as a list of lists of Python floats (modified in place) -> V (columns =
    eigenvectors).  Fixed sweep count, fixed (p, q) order, a rotation is skipped iff a_pq == 0."""
    n = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                app, aqq = A[p][p], A[q][q]
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    if k == p or k == q:
                        continue
                    akp, akq = A[k][p], A[k][q]
                    n1 = c * akp - s * akq; n2 = s * akp + c * akq
                    A[k][p] = n1; A[p][k] = n1; A[k][q] = n2; A[q][k] = n2
                A[p][p] = app - t * apq; A[q][q] = aqq + t * apq
                A[p][q] = 0.0; A[q][p] = 0.0
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq
    return V


def smallest(A):
    b = 0
    for i in range(1, len(A)):
        if A[i][i] < A[b][b]:
            b = i
    return b


def normal_matrix(P):
    """Hartley normalisation over P [k, 4] and M = A^T A summed sequentially in ascending point index.
    -> (M [9, 9], (sp, mpx, mpy, sc, mcx, mcy)) or None when the mean distance is zero in one image."""
    n = float(len(P))
    acc = np.zeros(4)
    for k in range(len(P)):
        acc = acc + P[k]
    mean = acc / n
    dp = 0.0; dc = 0.0
    for k in range(len(P)):
        d = P[k] - mean
        dp = dp + math.sqrt(d[0] * d[0] + d[1] * d[1])
        dc = dc + math.sqrt(d[2] * d[2] + d[3] * d[3])
    dp = dp / n; dc = dc / n
    if not (dp > 0.0 and dc > 0.0):
        return None
    sp = SQRT2 / dp; sc = SQRT2 / dc
    a = (P[:, 0] - mean[0]) * sp; b = (P[:, 1] - mean[1]) * sp; c = (P[:, 2] - mean[2]) * sc; d = (P[:, 3] - mean[3]) * sc
    rows = np.stack([a * c, a * d, a, b * c, b * d, b, c, d, np.ones(len(P))], 1)
    M = np.zeros((9, 9))
    for k in range(len(P)):
        M = M + rows[k][:, None] * rows[k][None, :]
    return M, (sp, float(mean[0]), float(mean[1]), sc, float(mean[2]), float(mean[3]))


def refit(P, sweeps=SWEEPS, info=None):
    """Least-squares F over P [k, 4]: smallest eigenvector of M by Jacobi, rank 2 by deflation with the smallest eigenvector of
    F^T F, denormalised.  -> F [9] or None."""
    nm = normal_matrix(P)
    if nm is None:
        return None
    M, nrm = nm
    A = [[float(M[i, j]) for j in range(9)] for i in range(9)]
    V = jacobi(A, sweeps)
    if info is not None:
        info["offdiag"] = math.sqrt(sum(A[i][j] ** 2 for i in range(9) for j in range(9) if i != j))
        info["trace"] = sum(A[i][i] for i in range(9))
    b = smallest(A)
    Fn = [V[e][b] for e in range(9)]
    G = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for c in range(a, 3):
            g = (Fn[a] * Fn[c] + Fn[3 + a] * Fn[3 + c]) + Fn[6 + a] * Fn[6 + c]
            G[a][c] = g; G[c][a] = g
    V3 = jacobi(G, sweeps)
    b3 = smallest(G)
    v = [V3[0][b3], V3[1][b3], V3[2][b3]]
    for i in range(3):
        w = (Fn[3 * i] * v[0] + Fn[3 * i + 1] * v[1]) + Fn[3 * i + 2] * v[2]
        for j in range(3):
            Fn[3 * i + j] = Fn[3 * i + j] - w * v[j]
    return denorm(np.array(Fn), *nrm)


# ---- the step ---------------------------------------------------------------------------------------------------------------
def reject_points(Pd, prm, frame_key):
    """The step on m virtual-camera point pairs Pd [m, 4] fp64.  -> (status [m] uint8, stats [4] int32, F [9] fp64);
    stats = valid hypotheses, best hypothesis, gate-1 inliers, kept after gate 2, all -1 when the step does not run (m < 8)."""
    m = len(Pd)
    status = np.ones(m, np.uint8); stats = np.full(4, -1, np.int32); F = np.zeros(9)
    if m < 8:
        return status, stats, F
    P1 = g1(Pd)
    n_hyp = min(prm.n_hyp, MAX_HYP)
    idx, ok = sample(prm.seed, frame_key, n_hyp, m)
    Fh, valid = solve(P1[np.where(ok[:, None], idx, 0)])
    valid &= ok
    thr2 = prm.f_threshold * prm.f_threshold
    inl = inliers(Fh, P1, thr2)
    cnt = np.where(valid, inl.astype(np.int64).sum(1), -1)          # an integer count: its order does not matter
    best = int(cnt.argmax())                                         # the first maximum: ties to the lowest h
    n_valid = int(valid.sum())
    if n_valid == 0 or cnt[best] < 8:
        status[:] = 0
        stats[:] = (n_valid, best if n_valid else -1, max(int(cnt[best]), 0), 0)
        return status, stats, F
    mask = inl[best]
    Fr = refit(P1[mask])
    if Fr is None:
        status[:] = 0
        stats[:] = (n_valid, best, int(cnt[best]), 0)
        return status, stats, F
    with np.errstate(all="ignore"):
        r2, lc, lp = epi(Fr, Pd[:, 0], Pd[:, 1], Pd[:, 2], Pd[:, 3])
        s = r2 / (lc + lp)
        keep = mask & ~(s > prm.f_dis)
    status = keep.astype(np.uint8)
    stats[:] = (n_valid, best, int(cnt[best]), int(keep.sum()))
    return status, stats, Fr


def reject(cam, prev_px, cur_px, prm, frame_key):
    """The step on pixel pairs (what lmono_tracker_reject_f runs)."""
    Pd = np.hstack([lift_virtual(cam, prev_px, prm.focal_length), lift_virtual(cam, cur_px, prm.focal_length)])
    return reject_points(Pd, prm, frame_key)


class TrackerRejectRef(R.TrackerRef):
    """track_ref.TrackerRef with rejectWithF after the forward-backward / inBorder compaction and before setMask."""

    def __init__(self, cam, max_cnt=150, min_dist=30, reject=None):
        self.reject_prm = reject
        super().__init__(cam, max_cnt, min_dist)

    def set_reject_f(self, prm):
        self.reject_prm = prm

    def reset(self):
        super().reset()
        self.frames = 0
        self.last_stats = np.full(4, -1, np.int32)
        self.last_F = np.zeros(9)

    def track(self, time, image):
        image = np.asarray(image, np.uint8)
        grey = R.bgr_to_grey(image) if image.ndim == 3 else image
        h, w = grey.shape
        assert (w, h) == (self.cam.width, self.cam.height)
        self.cur_pyr = R.build_pyramid(grey)
        pts, ids, cnt, pun = self.pts, self.ids, self.cnt, self.un
        has_prev = np.ones(len(pts), bool)
        self.last_stats = np.full(4, -1, np.int32); self.last_F = np.zeros(9)
        prev_kept = np.zeros((0, 2), np.float32)
        if len(pts):
            cur, st = R.lk_track(self.prev_pyr, self.cur_pyr, pts, R.MAX_LEVEL)
            rev = pts.copy(); rst = np.zeros(len(pts), np.uint8)
            live = np.nonzero(st)[0]
            if len(live):
                rev[live], rst[live] = R.lk_track(self.cur_pyr, self.prev_pyr, cur[live], 1, init=pts[live])
            keep = np.zeros(len(pts), bool)
            for i in range(len(pts)):
                if not (st[i] and rst[i]):
                    continue
                dx = float(F32(pts[i, 0] - rev[i, 0])); dy = float(F32(pts[i, 1] - rev[i, 1]))
                if not np.sqrt(dx * dx + dy * dy) <= 0.5:
                    continue
                rx, ry = np.rint(cur[i, 0]), np.rint(cur[i, 1])
                keep[i] = bool(1 <= rx and rx < w - 1 and 1 <= ry and ry < h - 1)
            self.last_status = keep.copy()
            prev_kept = pts[keep]
            pts, ids, cnt, pun = cur[keep], ids[keep], cnt[keep], pun[keep]
            has_prev = has_prev[keep]
        cnt = cnt + 1
        if self.reject_prm is not None:                                # rejectWithF (:259-262)
            status, self.last_stats, self.last_F = reject(self.cam, prev_kept, pts, self.reject_prm, self.frames)
            ok = status.astype(bool)
            pts, ids, cnt, pun, has_prev = pts[ok], ids[ok], cnt[ok], pun[ok], has_prev[ok]
        order, mask = R.set_mask(pts, ids, cnt, self.min_dist, w, h)
        pts, ids, cnt, pun, has_prev = pts[order], ids[order], cnt[order], pun[order], has_prev[order]
        quota = self.max_cnt - len(pts)
        if quota > 0:
            self.last_resp = R.response(grey)
            new = R.detect(self.last_resp, mask, quota, self.min_dist)
            if new:
                k = len(new)
                pts = np.vstack([pts, np.array(new, np.float32).reshape(-1, 2)])
                ids = np.concatenate([ids, np.arange(self.n_id, self.n_id + k, dtype=np.int32)]); self.n_id += k
                cnt = np.concatenate([cnt, np.ones(k, np.int32)])
                pun = np.vstack([pun, np.zeros((k, 2), np.float32)])
                has_prev = np.concatenate([has_prev, np.zeros(k, bool)])
        n = len(pts)
        rec = np.zeros(n, R.RECORD)
        un = np.zeros((n, 2), np.float32)
        dt = float(time) - self.prev_time
        for i in range(n):
            un[i] = self.cam.lift(pts[i, 0], pts[i, 1])
            if has_prev[i]:
                with np.errstate(divide="ignore", invalid="ignore"):
                    rec["vx"][i] = F32(np.float64(F32(un[i, 0] - pun[i, 0])) / np.float64(dt))
                    rec["vy"][i] = F32(np.float64(F32(un[i, 1] - pun[i, 1])) / np.float64(dt))
        rec["id"] = ids; rec["track_cnt"] = cnt
        rec["x_n"] = un[:, 0]; rec["y_n"] = un[:, 1]; rec["u"] = pts[:, 0]; rec["v"] = pts[:, 1]
        self.pts, self.ids, self.cnt, self.un = pts.astype(np.float32), ids.astype(np.int32), cnt.astype(np.int32), un
        self.prev_pyr = self.cur_pyr
        self.prev_time = float(time)
        self.frames += 1
        return rec
