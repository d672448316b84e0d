"""tests/excalib_ref.py -- CPU restatement of the camera-LiDAR rotation calibration (ESTIMATE_LASER == 2), numpy only.
Test infrastructure: k_excalib_step (lmono_amd/csrc/excalib.hip) and this file implement one written definition, every step one IEEE
fp64 operation in the order written here, so "equal" means equal bytes (the one exception is atan2 in the Huber weight, which the
device rounds differently; it matters only where a weight is below 1).  No np.linalg and no np.sum in the decision path: the sums are
sequential, the eigenvectors come from the fixed-sweep cyclic Jacobi of tests/track_reject_ref.py (the 9 x 9 refit) and its
elementwise batch form below (3 x 3, 4 x 4)."""
import math

import numpy as np

from tests import track_reject_ref as RR

MAX_PAIRS = 512
MIN_PAIRS = 9
SWEEPS3 = 6
SWEEPS4 = 7
DEG = 57.295779513082323


def jacobi_batch(A, sweeps):
    """RR.jacobi on a stack A [T, n, n] of symmetric matrices at once, elementwise (a skipped rotation keeps the old values).
    -> (A after the sweeps, V [T, n, n], columns = eigenvectors)."""
    A = np.array(A, np.float64)
    T, n, _ = A.shape
    V = np.zeros((T, n, n)); V[:, range(n), range(n)] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[:, p, q].copy()
                    on = apq != 0.0
                    app = A[:, p, p].copy(); aqq = A[:, q, q].copy()
                    theta = (aqq - app) / (2.0 * apq)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0.0, -t, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    for k in range(n):
                        if k == p or k == q:
                            continue
                        akp = A[:, k, p].copy(); akq = A[:, k, q].copy()
                        n1 = np.where(on, c * akp - s * akq, akp); n2 = np.where(on, s * akp + c * akq, akq)
                        A[:, k, p] = n1; A[:, p, k] = n1; A[:, k, q] = n2; A[:, q, k] = n2
                    A[:, p, p] = np.where(on, app - t * apq, app); A[:, q, q] = np.where(on, aqq + t * apq, aqq)
                    A[:, p, q] = np.where(on, 0.0, apq); A[:, q, p] = np.where(on, 0.0, A[:, q, p])
                    for k in range(n):
                        vkp = V[:, k, p].copy(); vkq = V[:, k, q].copy()
                        V[:, k, p] = np.where(on, c * vkp - s * vkq, vkp); V[:, k, q] = np.where(on, s * vkp + c * vkq, vkq)
    return A, V


def smallest_batch(A):
    """The index of the smallest diagonal entry, the first on a tie (a NaN never wins, as in `<`)."""
    T, n, _ = A.shape
    b = np.zeros(T, np.int64)
    ar = np.arange(T)
    for i in range(1, n):
        with np.errstate(all="ignore"):
            b = np.where(A[:, i, i] < A[ar, b, b], i, b)
    return b


def jacobi1(M, sweeps):
    """One matrix (array-like [n, n]) -> (diagonal [n], V [n, n], the off-diagonal Frobenius residue)."""
    A, V = jacobi_batch(np.asarray(M, np.float64)[None], sweeps)
    off = A[0] - np.diag(np.diag(A[0]))
    return np.diag(A[0]).copy(), V[0], float(np.sqrt((off * off).sum())), int(smallest_batch(A)[0])


# ---- stages 1-3 ---------------------------------------------------------------------------------------------------------------------------
def essential(P, info=None):
    """P [m, 4] finite pairs (prev x, prev y, cur x, cur y), m >= 9 -> E [9] with cur^T E prev = 0 (the transposed refit), or None."""
    F = RR.refit(P, RR.SWEEPS, info)
    if F is None:
        return None
    return np.asarray(F, np.float64).reshape(3, 3).T.reshape(9).copy()


def decompose(E, info=None):
    """E [9] -> (R12 [2, 3, 3], t [3])."""
    E = [float(e) for e in E]
    G = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for c in range(a, 3):
            g = (E[a] * E[c] + E[3 + a] * E[3 + c]) + E[6 + a] * E[6 + c]
            G[a][c] = g; G[c][a] = g
    d, V, off, b = jacobi1(G, SWEEPS3)
    if info is not None:
        info["off3"] = off; info["G"] = np.array(G); info["d3"] = d
    i1 = 1 if b == 0 else 0
    i2 = 1 if b == 2 else 2
    if d[i2] > d[i1]:
        i1, i2 = i2, i1
    v = [[float(V[r, i1]) for r in range(3)], [float(V[r, i2]) for r in range(3)], None]
    u = [None, None, None]
    with np.errstate(all="ignore"):
        for i in range(2):
            a0 = (E[0] * v[i][0] + E[1] * v[i][1]) + E[2] * v[i][2]
            a1 = (E[3] * v[i][0] + E[4] * v[i][1]) + E[5] * v[i][2]
            a2 = (E[6] * v[i][0] + E[7] * v[i][1]) + E[8] * v[i][2]
            nrm = np.sqrt(np.float64((a0 * a0 + a1 * a1) + a2 * a2))
            u[i] = [float(np.float64(a0) / nrm), float(np.float64(a1) / nrm), float(np.float64(a2) / nrm)]

        def cross(a, b):
            return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        u[2] = cross(u[0], u[1]); v[2] = cross(v[0], v[1])
        R12 = np.zeros((2, 3, 3))
        for i in range(3):
            for j in range(3):
                R12[0, i, j] = (u[1][i] * v[0][j] - u[0][i] * v[1][j]) + u[2][i] * v[2][j]
                R12[1, i, j] = (u[0][i] * v[1][j] - u[1][i] * v[0][j]) + u[2][i] * v[2][j]
    return R12, np.array(u[2])


def front(R, t, P, info=None):
    """-> [m] bool: the DLT point of each pair of P [m, 4] lies in front of [I | 0] and [R | t]."""
    m = len(P)
    px, py, cx, cy = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    one = np.ones(m); zero = np.zeros(m)
    with np.errstate(all="ignore"):
        A = [[-one, zero, px, zero], [zero, -one, py, zero],
             [cx * R[2, 0] - R[0, 0], cx * R[2, 1] - R[0, 1], cx * R[2, 2] - R[0, 2], cx * t[2] - t[0]],
             [cy * R[2, 0] - R[1, 0], cy * R[2, 1] - R[1, 1], cy * R[2, 2] - R[1, 2], cy * t[2] - t[1]]]
        B = np.zeros((m, 4, 4))
        for a in range(4):
            for c in range(a, 4):
                g = ((A[0][a] * A[0][c] + A[1][a] * A[1][c]) + A[2][a] * A[2][c]) + A[3][a] * A[3][c]
                B[:, a, c] = g; B[:, c, a] = g
        D, V = jacobi_batch(B, SWEEPS4)
        if info is not None:
            off = D - D * np.eye(4)[None]
            info.setdefault("off4_dlt", []).append(float(np.sqrt((off * off).sum((1, 2))).max()))
        b = smallest_batch(D)
        ar = np.arange(m)
        w = V[ar, 3, b]
        good = (w != 0.0) & np.isfinite(w)
        X = V[ar, 0, b] / w; Y = V[ar, 1, b] / w; Z = V[ar, 2, b] / w
        zr = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
        return good & (Z > 0.0) & (zr > 0.0)


def relative_rotation(pairs, info=None):
    """Stages 1-3 on pairs [m, 4] -> (R [9] row-major: the camera's rotation increment, stats [6] int32 = pairs used, the four front
    counts, the winner: 0 R1, 1 R2, -1 the identity by rule)."""
    P = np.asarray(pairs, np.float64).reshape(-1, 4)[:MAX_PAIRS]
    P = P[np.isfinite(P).all(1)]
    m = len(P)
    R = np.eye(3).reshape(9)
    stats = np.array([m, 0, 0, 0, 0, -1], np.int32)
    if m < MIN_PAIRS:
        return R, stats
    E = essential(P, info)
    if E is None:
        return R, stats
    R12, t = decompose(E, info)
    cnt = [int(front(R12[c >> 1], -t if c & 1 else t, P, info).sum()) for c in range(4)]
    stats[1:5] = cnt
    win = 0 if max(cnt[0], cnt[1]) > max(cnt[2], cnt[3]) else 1
    if not np.isfinite(R12[win]).all():
        return R, stats
    stats[5] = win
    return R12[win].T.reshape(9).copy(), stats


# ---- stage 4 ------------------------------------------------------------------------------------------------------------------------------
def q2m(q):
    """Eigen's toRotationMatrix; q = (x, y, z, w), not normalised -> [3, 3]."""
    x, y, z, w = (float(v) for v in q)
    tx = 2.0 * x; ty = 2.0 * y; tz = 2.0 * z
    twx = tx * w; twy = ty * w; twz = tz * w; txx = tx * x; txy = ty * x; txz = tz * x; tyy = ty * y; tyz = tz * y; tzz = tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def m2q(R):
    """Eigen's Quaterniond(Matrix3d) -> [x, y, z, w]."""
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    q = [0.0] * 4
    tr = (R[0][0] + R[1][1]) + R[2][2]
    if tr > 0.0:
        tr = math.sqrt(tr + 1.0)
        q[3] = 0.5 * tr
        tr = 0.5 / tr
        q[0] = (R[2][1] - R[1][2]) * tr; q[1] = (R[0][2] - R[2][0]) * tr; q[2] = (R[1][0] - R[0][1]) * tr
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        s = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k][j] - R[j][k]) * s
        q[j] = (R[j][i] + R[i][j]) * s
        q[k] = (R[k][i] + R[i][k]) * s
    return q


def mul33(A, B):
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]
    return C


def angle_deg(a, b):
    """Quaterniond::angularDistance in degrees: 2 atan2(|vec|, |w|) of a b*."""
    cx, cy, cz, cw = -b[0], -b[1], -b[2], b[3]
    w = ((a[3] * cw - a[0] * cx) - a[1] * cy) - a[2] * cz
    x = ((a[3] * cx + a[0] * cw) + a[1] * cz) - a[2] * cy
    y = ((a[3] * cy + a[1] * cw) + a[2] * cx) - a[0] * cz
    z = ((a[3] * cz + a[2] * cw) + a[0] * cy) - a[1] * cx
    nv = math.sqrt((x * x + y * y) + z * z)
    return DEG * (2.0 * math.atan2(nv, abs(w)))


def block(r1, rl, huber):
    """huber (L(r1) - R(rl)) [4, 4]; quaternions x y z w."""
    x, y, z, w = r1
    a, b, c, d = rl
    L = np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])
    Rm = np.array([[d, c, -b, a], [-c, d, a, b], [b, -a, d, c], [-a, -b, -c, d]])
    return huber * (L - Rm)


class Calibrator:
    """One stream's state (the running sum M [4, 4], rlc [3, 3], frame_count) and the step on it."""

    def __init__(self, count=10):
        self.count = int(count)
        self.reset()

    def reset(self):
        self.M = np.zeros((4, 4)); self.rlc = np.eye(3); self.frame_count = 0
        self.blocks = []            # the reference's stacked rows, for the test of observation A
        self.info = {}

    def push(self, q_cam, q_lidar):
        """Stage 4 -> (rlc [9], sv [4] descending, huber, ok)."""
        self.frame_count += 1
        Rc = q2m(q_cam); Rl = q2m(q_lidar)
        Rg = mul33(mul33(self.rlc.T, Rl), self.rlc)
        r1 = m2q(Rc); r2 = m2q(Rg); rl = m2q(Rl)
        deg = angle_deg(r1, r2)
        huber = 5.0 / deg if deg > 5.0 else 1.0
        D = block(r1, rl, huber)
        self.blocks.append(D.copy())
        for a in range(4):
            for c in range(a, 4):
                g = ((D[0, a] * D[0, c] + D[1, a] * D[1, c]) + D[2, a] * D[2, c]) + D[3, a] * D[3, c]
                s = self.M[a, c] + g
                self.M[a, c] = s; self.M[c, a] = s
        d, V, off, b = jacobi1(self.M, SWEEPS4)
        self.info = {"off4": off, "deg": deg, "eig": np.sort(d), "x": V[:, b].copy()}
        self.rlc = q2m(V[:, b]).T.copy()
        sv = [math.sqrt(l) if l > 0.0 else 0.0 for l in d]
        for i in range(1, 4):
            k = i
            while k > 0 and sv[k] > sv[k - 1]:
                sv[k], sv[k - 1] = sv[k - 1], sv[k]
                k -= 1
        ok = self.frame_count >= self.count and sv[2] > 0.25
        return self.rlc.reshape(9).copy(), np.array(sv), huber, bool(ok)

    def step(self, pairs, q_lidar, info=None):
        """Stages 1-4 -> (R_cam [9], stats [6], rlc [9], sv [4], huber, ok)."""
        R, stats = relative_rotation(pairs, info)
        return (R, stats) + self.push(m2q(R.reshape(3, 3)), q_lidar)

    def state(self):
        return self.frame_count, self.M.reshape(16).copy(), self.rlc.reshape(9).copy()
