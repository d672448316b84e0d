"""An independent statement of the loop-closure pose graph (numpy, CPU), written from the definition in the header comment of
lmono_amd/csrc/posegraph.hip and not from the kernel or from oracle/lo_posegraph.c:

  state      per keyframe (yaw in degrees, t); pitch and roll of the input pose stay fixed; R = Rz(yaw) Ry(pitch) Rx(roll)
  edge a->b  r[0:3] = R_a^T (t_b - t_a) - meas_t,  r[3] = wy NormalizeAngle(yaw_b - yaw_a - meas_yaw)
  odometry   every keyframe to its (up to) four predecessors, measured from the input poses (full rotation of a), wy = 1
  loops      one edge per loop from loop_info (relative_t = [0:3], relative_yaw = [7]), wy = 0.1, Huber(0.1) over s = |r|^2
  cost       sum over edges of rho(s) / 2,  rho(s) = s for s <= 0.01 and 0.2 sqrt(s) - 0.01 beyond
  gauge      keyframe 0 is constant

Jacobians come from a complex step (h = 1e-30; NormalizeAngle and the Huber test branch on the real part), so they are exact to
rounding and need no finite-difference tolerance.  The normal equations are Gauss-Newton with the Ceres corrector for a loss with
rho'' <= 0: residual and Jacobian of an edge are scaled by sqrt(rho'(s))."""
import numpy as np

H_STEP = 1e-30
HUBER_A = 0.1


class Graph:
    """n keyframes; edge k goes a[k] -> b[k] (loop[k] marks a loop edge) with meas[k] = (t, yaw); x0 [n,4] = (yaw, t)."""


def _rotation_of_quaternion(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _yaw_pitch_roll_deg(R):
    """Angles of R = Rz(y) Ry(p) Rx(r): R[:,0] = (cy cp, sy cp, -sp), R[2,1:] = (cp sr, cp cr)."""
    return np.rad2deg([np.arctan2(R[1, 0], R[0, 0]), np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0])), np.arctan2(R[2, 1], R[2, 2])])


def edges(poses, loops, loop_info):
    P = np.asarray(poses, np.float64).reshape(-1, 7)
    lp = np.asarray(loops, np.int64).reshape(-1, 2)
    li = np.asarray(loop_info, np.float64).reshape(-1, 8)
    n = len(P)
    g = Graph()
    g.n = n
    Rs = [_rotation_of_quaternion(P[i, 3:]) for i in range(n)]
    ypr = np.array([_yaw_pitch_roll_deg(R) for R in Rs])
    g.x0 = np.concatenate([ypr[:, :1], P[:, :3]], 1)
    g.pitch, g.roll = ypr[:, 1].copy(), ypr[:, 2].copy()
    a, b, loop, meas = [], [], [], []
    for i in range(1, n):
        for j in range(1, 5):
            if i - j < 0:
                continue
            k = i - j
            a.append(k); b.append(i); loop.append(False)
            meas.append(np.concatenate([Rs[k].T @ (P[i, :3] - P[k, :3]), [ypr[i, 0] - ypr[k, 0]]]))
    for k in range(len(lp)):
        a.append(int(lp[k, 0])); b.append(int(lp[k, 1])); loop.append(True)
        meas.append(np.concatenate([li[k, :3], [li[k, 7]]]))
    g.a, g.b, g.loop = np.array(a, np.int64), np.array(b, np.int64), np.array(loop, bool)
    g.meas = np.array(meas, np.float64).reshape(-1, 4)
    return g


def normalize_angle(d):
    """NormalizeAngle: one wrap by 360, decided on the real part."""
    re = np.real(d)
    return np.where(re > 180.0, d - 360.0, np.where(re < -180.0, d + 360.0, d))


def raw_yaw_difference(g, x):
    """yaw_b - yaw_a - meas_yaw before NormalizeAngle, per edge."""
    x = np.asarray(x).reshape(-1, 4)
    return np.real(x[g.b, 0] - x[g.a, 0] - g.meas[:, 3])


def _edge_residuals(g, xa, xb, sel=slice(None)):
    """Residuals [E,4] (before the robust scaling) of the selected edges from their own end states xa, xb [E,4] (may be complex)."""
    rad = np.pi / 180.0
    y, p, r = xa[:, 0] * rad, g.pitch[g.a[sel]] * rad, g.roll[g.a[sel]] * rad
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    # Rz(y) Ry(p) Rx(r), rows
    R = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
         [-sp + 0 * y, cp * sr + 0 * y, cp * cr + 0 * y]]
    d = xb[:, 1:] - xa[:, 1:]
    out = np.zeros((len(xa), 4), dtype=np.result_type(xa.dtype, xb.dtype))
    for k in range(3):                                                  # R^T d
        out[:, k] = R[0][k] * d[:, 0] + R[1][k] * d[:, 1] + R[2][k] * d[:, 2] - g.meas[sel, k]
    wy = np.where(g.loop[sel], 0.1, 1.0)
    out[:, 3] = wy * normalize_angle(xb[:, 0] - xa[:, 0] - g.meas[sel, 3])
    return out


def residual(g, x, edge=None):
    """Residual(s) before the robust scaling: [4] of one edge, or [E,4] of all."""
    x = np.asarray(x).reshape(-1, 4)
    if edge is None:
        return _edge_residuals(g, x[g.a], x[g.b])
    sel = slice(edge, edge + 1)
    return _edge_residuals(g, x[g.a[sel]], x[g.b[sel]], sel)[0]


def squared_norms(g, x):
    r = residual(g, x)
    return np.real(np.sum(r * r, 1))


def _edge_costs(g, r):
    s = np.sum(r * r, 1)
    act = g.loop & (np.real(s) > HUBER_A * HUBER_A)
    safe = np.where(act, s, 1.0)
    return np.where(act, 0.5 * (2.0 * HUBER_A * np.sqrt(safe) - HUBER_A * HUBER_A), 0.5 * s)


def edge_costs(g, x):
    return np.real(_edge_costs(g, residual(g, x)))


def cost(g, x):
    return float(np.sum(edge_costs(g, x)))


def _perturbed(xe, k):
    xp = xe.astype(np.complex128)
    xp[:, k] += 1j * H_STEP
    return xp


def jacobians(g, x):
    """(Ja, Jb) [E,4,4]: d residual / d (yaw, tx, ty, tz) of the older and of the newer keyframe, before the robust scaling."""
    x = np.asarray(x, np.float64).reshape(-1, 4)
    xa, xb = x[g.a], x[g.b]
    Ja, Jb = np.zeros((len(xa), 4, 4)), np.zeros((len(xa), 4, 4))
    for k in range(4):
        Ja[:, :, k] = np.imag(_edge_residuals(g, _perturbed(xa, k), xb.astype(np.complex128))) / H_STEP
        Jb[:, :, k] = np.imag(_edge_residuals(g, xa.astype(np.complex128), _perturbed(xb, k))) / H_STEP
    return Ja, Jb


def gradient(g, x):
    """Complex-step gradient [n,4] of cost(x) itself (the loss differentiated directly, no corrector involved)."""
    x = np.asarray(x, np.float64).reshape(-1, 4)
    xa, xb = x[g.a], x[g.b]
    out = np.zeros((g.n, 4))
    for k in range(4):
        da = np.imag(_edge_costs(g, _edge_residuals(g, _perturbed(xa, k), xb.astype(np.complex128)))) / H_STEP
        db = np.imag(_edge_costs(g, _edge_residuals(g, xa.astype(np.complex128), _perturbed(xb, k)))) / H_STEP
        np.add.at(out[:, k], g.a, da)
        np.add.at(out[:, k], g.b, db)
    return out


def dense_system(g, x):
    """-> (H [4n,4n], g [4n], cost) in keyframe order: Gauss-Newton with the corrector; keyframe 0 is an identity block without
    coupling and without gradient."""
    x = np.asarray(x, np.float64).reshape(-1, 4)
    r = residual(g, x)
    s = np.sum(r * r, 1)
    Ja, Jb = jacobians(g, x)
    act = g.loop & (s > HUBER_A * HUBER_A)
    wr = np.where(act, np.sqrt(HUBER_A / np.sqrt(np.where(act, s, 1.0))), 1.0)          # sqrt(rho')
    r = r * wr[:, None]; Ja = Ja * wr[:, None, None]; Jb = Jb * wr[:, None, None]
    n4 = 4 * g.n
    H, grad = np.zeros((n4, n4)), np.zeros(n4)
    for e in range(len(g.a)):
        J = np.zeros((4, n4))
        a, b = int(g.a[e]), int(g.b[e])
        J[:, 4 * a:4 * a + 4] = Ja[e]; J[:, 4 * b:4 * b + 4] = Jb[e]
        idx = np.r_[4 * a:4 * a + 4, 4 * b:4 * b + 4]
        Je = J[:, idx]
        H[np.ix_(idx, idx)] += Je.T @ Je
        grad[idx] += Je.T @ r[e]
    H[:4, :] = 0.0; H[:, :4] = 0.0; H[:4, :4] = np.eye(4); grad[:4] = 0.0
    return H, grad, cost(g, x)
