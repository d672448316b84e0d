"""tests/pnp_ref.py -- CPU restatement of the loop verification (KeyFrame::PnPRANSAC and the gates of findConnection),
numpy only.  Test infrastructure: k_pnp_ransac (lmono_amd/csrc/pnp.hip) and this file implement one written definition, every step
one IEEE fp64 operation in the order written here, so "equal" means equal bytes up to the pose.  Vectorised over hypotheses and over
points, elementwise only: no np.linalg and no np.sum in the decision path.  What follows the pose (R2ypr, the gates, loop_info, the
15-value channel) uses atan2 / sin / cos and is compared to a tolerance."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
T = 256                 # threads of the workgroup: the shape of the refit's summation tree
WAVE = 64
MAX_POINTS = 512
MAX_HYP = 1024
MAX_DRAWS = 256
ITERS = 12
DAMP = 6
PIVOT = 1e-12
THRESHOLD = 10.0 / 460.0
MIN_BRIEF_LOOP_NUM = 25
MIN_PNP_LOOP_NUM = 5
ANGLE_THRESHOLD = 30.0
TRANS_THRESHOLD = 20.0


class PnPParams:
    def __init__(self, threshold=0.0, n_hyp=0, seed=0, min_brief_loop_num=0, min_pnp_loop_num=0, angle_threshold=0.0, trans_threshold=0.0):
        self.threshold = float(threshold) if threshold else THRESHOLD
        self.n_hyp = int(n_hyp) if n_hyp else 256
        self.seed = int(seed) & 0xFFFFFFFF
        self.min_brief_loop_num = int(min_brief_loop_num) if min_brief_loop_num else MIN_BRIEF_LOOP_NUM
        self.min_pnp_loop_num = int(min_pnp_loop_num) if min_pnp_loop_num else MIN_PNP_LOOP_NUM
        self.angle_threshold = float(angle_threshold) if angle_threshold else ANGLE_THRESHOLD
        self.trans_threshold = float(trans_threshold) if trans_threshold else TRANS_THRESHOLD


# ---- the sample stream (6e item 4a's mix and draw rule) -----------------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def hyp_keys(seed, key, n_hyp):
    h = np.arange(n_hyp, dtype=np.uint64)
    base = mix(mix(np.uint64((seed ^ 0x9e3779b9) & 0xFFFFFFFF)) ^ np.uint64(key & 0xFFFFFFFF))
    return mix(base ^ h)


def sample(seed, key, n_hyp, m):
    """-> (idx [n_hyp, 4], ok [n_hyp]): 4 distinct indices below m per hypothesis; draw d is mix(key ^ d), index (r * m) >> 32, a
    repeat is redrawn with the next d; a sample still incomplete after MAX_DRAWS draws is not ok."""
    keys = hyp_keys(seed, key, n_hyp)
    idx = np.full((n_hyp, 4), -1, np.int64)
    have = np.zeros(n_hyp, np.int64)
    for d in range(MAX_DRAWS):
        todo = have < 4
        if not todo.any():
            break
        r = mix(keys ^ np.uint64(d))
        c = ((r * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
        dup = (idx == c[:, None]).any(1)
        rows = np.nonzero(todo & ~dup)[0]
        idx[rows, have[rows]] = c[rows]
        have[rows] += 1
    return idx, have == 4


def caller_key(cur_index, old_index):
    return ((int(cur_index) << 16) | int(old_index)) & 0xFFFFFFFF


# ---- quaternions (x y z w), arrays [..., 4] ----------------------------------------------------------------------------------
def qmul(a, b):
    a0, a1, a2, a3 = (a[..., k] for k in range(4)); b0, b1, b2, b3 = (b[..., k] for k in range(4))
    x = ((a3 * b0 + a0 * b3) + a1 * b2) - a2 * b1
    y = ((a3 * b1 - a0 * b2) + a1 * b3) + a2 * b0
    z = ((a3 * b2 + a0 * b1) - a1 * b0) + a2 * b3
    w = ((a3 * b3 - a0 * b0) - a1 * b1) - a2 * b2
    return np.stack(np.broadcast_arrays(x, y, z, w), -1)


def qnormalise(q):
    n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    return q / n[..., None]


def rot(q):
    """-> the 9 entries of R(q), row-major, each an array of q's leading shape."""
    x, y, z, w = (q[..., k] for k in range(4))
    xx = x * x; yy = y * y; zz = z * z; xy = x * y; xz = x * z; yz = y * z; wx = w * x; wy = w * y; wz = w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def apply(R, t, X):
    """p = R X + t; R: 9 arrays, t: 3 arrays, X: 3 arrays, all broadcastable."""
    return [((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0],
            ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1],
            ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2]]


def guess_from_vio(vio_tq, ex_tq):
    """The initial guess of KeyFrame.cc:308-312 as [7] = t, q (camera from world)."""
    vio = np.asarray(vio_tq, np.float64); ex = np.asarray(ex_tq, np.float64)
    qwc = qmul(vio[3:], ex[3:])
    q = qnormalise(np.array([-qwc[0], -qwc[1], -qwc[2], qwc[3]]))
    twc = apply(rot(vio[3:]), vio[:3], ex[:3])
    p = apply(rot(q), [0.0, 0.0, 0.0], twc)
    return np.array([-p[0], -p[1], -p[2], q[0], q[1], q[2], q[3]])


# ---- the iteration ---------------------------------------------------------------------------------------------------------------
def inlier(R, t, X, u, v, thr2):
    with np.errstate(all="ignore"):
        p = apply(R, t, X)
        dx = p[0] / p[2] - u; dy = p[1] / p[2] - v
        return (p[2] > 0.0) & (dx * dx + dy * dy <= thr2)


def contrib(R, t, X, u, v):
    """-> (c: list of 27 arrays, front: p.z > 0).  H (upper triangle, row-major) then g."""
    with np.errstate(all="ignore"):
        p = apply(R, t, X)
        front = p[2] > 0.0
        iz = 1.0 / p[2]; nx = p[0] / p[2]; ny = p[1] / p[2]; rx = nx - u; ry = ny - v; gx = nx * iz; gy = ny * iz
        D = [None] * 9
        for r in range(3):
            D[3 * r] = R[3 * r + 2] * X[1] - R[3 * r + 1] * X[2]
            D[3 * r + 1] = R[3 * r] * X[2] - R[3 * r + 2] * X[0]
            D[3 * r + 2] = R[3 * r + 1] * X[0] - R[3 * r] * X[1]
        zero = np.zeros_like(iz)
        Jx = [iz, zero, -gx] + [iz * D[k] - gx * D[6 + k] for k in range(3)]
        Jy = [zero, iz, -gy] + [iz * D[3 + k] - gy * D[6 + k] for k in range(3)]
        c = []
        for a in range(6):
            for b in range(a, 6):
                c.append(Jx[a] * Jx[b] + Jy[a] * Jy[b])
        for a in range(6):
            c.append(Jx[a] * rx + Jy[a] * ry)
    return c, front


def solve6(s, lam):
    """(H + lam diag H) delta = -g, natural order, diagonal pivots -> (delta: 6 arrays, ok)."""
    with np.errstate(all="ignore"):
        A = {}
        e = 0
        for a in range(6):
            for c in range(a, 6):
                A[a, c] = s[e]; e += 1
        b = [None] * 6
        for a in range(6):
            A[a, a] = A[a, a] + lam * A[a, a]; b[a] = -s[21 + a]
        ok = np.ones(np.shape(A[0, 0]), bool)
        for k in range(6):
            d = A[k, k]
            ok = ok & (d >= PIVOT)
            for i in range(k + 1, 6):
                l = A[k, i] / d
                for j in range(i, 6):
                    A[i, j] = A[i, j] - l * A[k, j]
                b[i] = b[i] - l * b[k]
        delta = [None] * 6
        for k in range(5, -1, -1):
            acc = b[k]
            for j in range(k + 1, 6):
                acc = acc - A[k, j] * delta[j]
            delta[k] = acc / A[k, k]
    return delta, ok


def update(t, q, delta):
    with np.errstate(all="ignore"):
        t = np.stack([t[..., 0] + delta[0], t[..., 1] + delta[1], t[..., 2] + delta[2]], -1)
        dq = np.stack(np.broadcast_arrays(delta[3] * 0.5, delta[4] * 0.5, delta[5] * 0.5, np.ones_like(delta[3])), -1)
        return t, qnormalise(qmul(q, dq))


def lam_of(k, damp=DAMP):
    lam = 1.0
    for _ in range(k):
        lam = lam * 0.25
    return lam if k < damp else 0.0


def solve4(pd, idx, guess, iters=ITERS, damp=DAMP):
    """The minimal solve of every hypothesis at once: pd [m, 5] fp64, idx [nh, 4] -> (t [nh, 3], q [nh, 4], ok [nh])."""
    nh = len(idx)
    t = np.tile(np.asarray(guess[:3], np.float64), (nh, 1)); q = np.tile(np.asarray(guess[3:], np.float64), (nh, 1))
    ok = np.ones(nh, bool)
    P = pd[np.maximum(idx, 0)]                    # [nh, 4, 5]
    for it in range(iters):
        R = rot(q)
        s = [np.zeros(nh) for _ in range(27)]
        for k in range(4):
            c, front = contrib(R, [t[:, 0], t[:, 1], t[:, 2]], [P[:, k, 0], P[:, k, 1], P[:, k, 2]], P[:, k, 3], P[:, k, 4])
            ok &= front
            s = [s[e] + c[e] for e in range(27)]
        delta, good = solve6(s, lam_of(it, damp))
        ok &= good
        t, q = update(t, q, delta)
    R = rot(q)
    for k in range(4):
        p = apply(R, [t[:, 0], t[:, 1], t[:, 2]], [P[:, k, 0], P[:, k, 1], P[:, k, 2]])
        with np.errstate(all="ignore"):
            ok &= p[2] > 0.0
    return t, q, ok


def tree_sum(c, part):
    """The refit's sum of one quantity: c [MAX_POINTS] per-point values (0.0 where the point does not take part).  Thread t adds the
    points t and t + 256 to 0.0, a butterfly over the 64 lanes of each wave, then (w0 + w1) + (w2 + w3)."""
    v = (0.0 + np.where(part[:T], c[:T], 0.0))
    v = np.where(part[T:], v + c[T:], v)
    lane = np.arange(T)
    o = 32
    while o > 0:
        v = v + v[lane ^ o]
        o >>= 1
    return (v[0] + v[64]) + (v[128] + v[192])


def refit(pd, mask, t, q, iters=ITERS):
    """-> (t, q, steps done).  A step with an inlier at p.z <= 0 or a pivot below PIVOT ends the refit at the pose before it."""
    m = len(pd)
    part = np.zeros(MAX_POINTS, bool); part[:m] = mask
    X = np.zeros((MAX_POINTS, 5)); X[:m] = pd
    done = 0
    for it in range(iters):
        R = rot(q)
        c, front = contrib(R, list(t), [X[:, 0], X[:, 1], X[:, 2]], X[:, 3], X[:, 4])
        if (part & ~front).any():
            break
        s = [tree_sum(np.broadcast_to(c[e], (MAX_POINTS,)), part) for e in range(27)]
        delta, ok = solve6(s, lam_of(it))
        if not ok:
            break
        t, q = update(t, q, delta)
        done += 1
    return t, q, done


def pnp_ransac(p3, p2, guess_tq, key=0, params=None, iters=ITERS):
    """-> (status [m] uint8, pose [7] fp64, stats [4] int32: valid hypotheses, best h, the winner's inliers, refit steps done)."""
    prm = params or PnPParams()
    p3 = np.asarray(p3, np.float32).reshape(-1, 3); p2 = np.asarray(p2, np.float32).reshape(-1, 2)
    m = len(p3)
    guess = np.asarray(guess_tq, np.float64).copy()
    status = np.zeros(m, np.uint8)
    if m < 4 or m > MAX_POINTS:
        return status, guess, np.full(4, -1, np.int32)
    pd = np.concatenate([p3.astype(np.float64), p2.astype(np.float64)], 1)
    thr2 = prm.threshold * prm.threshold
    nh = min(prm.n_hyp, MAX_HYP)
    idx, ok = sample(prm.seed, key, nh, m)
    t, q, good = solve4(pd, idx, guess, iters)
    ok = ok & good
    R = rot(q[:, None, :])
    inl = inlier(R, [t[:, None, 0], t[:, None, 1], t[:, None, 2]], [pd[None, :, 0], pd[None, :, 1], pd[None, :, 2]], pd[None, :, 3], pd[None, :, 4], thr2)
    cnt = inl.sum(1)                            # integers
    nvalid = int(ok.sum())
    if nvalid == 0:
        return status, guess, np.array([0, -1, 0, 0], np.int32)
    score = np.where(ok, cnt * 65536 + (0xFFFF - np.arange(nh)), 0)
    bh = int(np.argmax(score)); bcnt = int(cnt[bh])
    if bcnt < 4:
        return status, guess, np.array([nvalid, bh, bcnt, 0], np.int32)
    status = inl[bh].astype(np.uint8)
    tt, qq, done = refit(pd, inl[bh], t[bh].copy(), q[bh].copy(), iters)
    return status, np.concatenate([tt, qq]), np.array([nvalid, bh, bcnt, done], np.int32)


# ---- after PnP: tolerance territory (atan2, sin, cos) ----------------------------------------------------------------------------
def rot_matrix(q):
    return np.array([float(v) for v in rot(np.asarray(q, np.float64))]).reshape(3, 3)


def quat_conj(q):
    q = np.asarray(q, np.float64)
    return np.array([-q[0], -q[1], -q[2], q[3]])


def r2ypr(R):
    """math_utils.h:187-202, degrees."""
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = math.atan2(n[1], n[0])
    p = math.atan2(-n[2], n[0] * math.cos(y) + n[1] * math.sin(y))
    r = math.atan2(a[0] * math.sin(y) - a[1] * math.cos(y), -o[0] * math.sin(y) + o[1] * math.cos(y))
    return np.array([y, p, r]) / math.pi * 180.0


def normalize_angle(a):
    """math_utils.h:252-260."""
    if a > 0:
        return a - 360.0 * math.floor((a + 180.0) / 360.0)
    return a + 360.0 * math.floor((-a + 180.0) / 360.0)


def after_pnp(pose_tq, n_brief, n_inliers, vio_tq, ex_tq, old_tq=None, cur_index=0, params=None):
    """KeyFrame.cc:341-350, :570-588, :636-682 -> dict: pnp_t_old [3], pnp_q_old [4] (x y z w), relative_t, relative_q (x y z w),
    relative_yaw, relative_euler [3], has_loop, loop_info [8], channel [15] (None without old_tq)."""
    prm = params or PnPParams()
    pose = np.asarray(pose_tq, np.float64); vio = np.asarray(vio_tq, np.float64); ex = np.asarray(ex_tq, np.float64)
    q_wc_old = quat_conj(pose[3:])
    T_wc_old = rot_matrix(q_wc_old) @ (-pose[:3])
    q_old = qmul(q_wc_old, quat_conj(ex[3:]))
    R_old = rot_matrix(q_old)
    T_old = T_wc_old - R_old @ ex[:3]
    R_vio = rot_matrix(vio[3:])
    rel_t = R_old.T @ (vio[:3] - T_old)
    rel_q = qmul(quat_conj(q_old), vio[3:])
    e_vio, e_old = r2ypr(R_vio), r2ypr(R_old)
    rel_yaw = normalize_angle(e_vio[0] - e_old[0])
    rel_euler = e_vio - e_old
    ran = n_brief > prm.min_brief_loop_num
    has_loop = bool(ran and n_inliers > prm.min_pnp_loop_num and
                    abs(math.sqrt(float(rel_euler @ rel_euler))) < prm.angle_threshold and math.sqrt(float(rel_t @ rel_t)) < prm.trans_threshold)
    loop_info = np.array([rel_t[0], rel_t[1], rel_t[2], rel_q[3], rel_q[0], rel_q[1], rel_q[2], rel_yaw])
    channel = None
    if old_tq is not None:
        old = np.asarray(old_tq, np.float64)
        cT = rot_matrix(old[3:]) @ rel_t + old[:3]
        cQ = qmul(old[3:], rel_q)
        channel = np.array([old[0], old[1], old[2], old[6], old[3], old[4], old[5], cT[0], cT[1], cT[2], cQ[3], cQ[0], cQ[1], cQ[2], float(cur_index)])
    return dict(pnp_t_old=T_old, pnp_q_old=q_old, relative_t=rel_t, relative_q=rel_q, relative_yaw=rel_yaw, relative_euler=rel_euler,
                has_loop=has_loop, loop_info=loop_info, channel=channel)
