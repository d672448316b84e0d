"""tests/pnp_cases.py -- synthetic PnP problems shared by the CPU and GPU tests of the loop verification."""
import math

import numpy as np

from tests import pnp_ref as P

NOISE = 0.5 / 460.0          # sigma of the observation noise: half a pixel at FOCAL_LENGTH 460


def quat_axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    s = math.sin(0.5 * angle)
    return np.array([axis[0] * s, axis[1] * s, axis[2] * s, math.cos(0.5 * angle)])


def scene(m, seed, outliers, noise=NOISE, angle_deg=None, trans=None, gate_share=1.0):
    """m points at 5..50 m in a KITTI-shaped field of view (+-40 x +-12 degrees) of the old camera, whose camera-from-world pose is
    known; Gaussian noise on the normalised observations; a share of outliers (none while m <= 5: a sample needs 4 inliers, and at m = 5 one outlier leaves a single all-inlier sample that a
    self-consistent contaminated sample can tie), each
    displaced by 6..40 thresholds; a guess whose camera is displaced from the truth by up to gate_share of 30 degrees and 20 m.
    -> (points_3d f32 [m, 3], points_2d f32 [m, 2], guess [7], truth [7], outlier mask [m])"""
    rng = np.random.default_rng(seed)
    q_true = quat_axis_angle(rng.normal(size=3), rng.uniform(0, 0.3))
    t_true = rng.uniform(-2, 2, 3)
    z = rng.uniform(5, 50, m)
    pc = np.stack([z * np.tan(np.radians(rng.uniform(-40, 40, m))), z * np.tan(np.radians(rng.uniform(-12, 12, m))), z], 1)
    R = P.rot_matrix(q_true)
    xw = (pc - t_true) @ R
    uv = pc[:, :2] / pc[:, 2:3] + rng.normal(size=(m, 2)) * noise
    n_out = int(round(outliers * m)) if m > 5 else 0
    out = np.zeros(m, bool); out[rng.permutation(m)[:n_out]] = True
    d = rng.normal(size=(m, 2)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    uv[out] += d[out] * rng.uniform(6, 40, (int(out.sum()), 1)) * P.THRESHOLD
    ang = np.radians(rng.uniform(0, 30 * gate_share) if angle_deg is None else angle_deg)
    tr = rng.uniform(0, 20 * gate_share) if trans is None else trans
    dq = quat_axis_angle(rng.normal(size=3), ang); dv = rng.normal(size=3); dv = dv / np.linalg.norm(dv) * tr
    q_wc = P.qmul(P.quat_conj(q_true), dq); t_wc = -(R.T @ t_true) + dv
    q_g = P.qnormalise(P.quat_conj(q_wc)); t_g = -(P.rot_matrix(q_g) @ t_wc)
    return xw.astype(np.float32), uv.astype(np.float32), np.concatenate([t_g, q_g]), np.concatenate([t_true, q_true]), out


def degenerate_cases():
    """name -> (points_3d, points_2d, guess): inputs on which the step must report failure (or, for few points, not run)."""
    rng = np.random.default_rng(5)
    ident = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    cases = {}
    for m in range(4):
        p3, p2, g, _, _ = scene(max(m, 1), 40 + m, 0.0)
        cases["m=%d" % m] = (p3[:m], p2[:m], g)
    uv = rng.uniform(-0.3, 0.3, (40, 2)).astype(np.float32)
    cases["identical 3-D points"] = (np.tile(np.float32([1.0, -0.5, 12.0]), (40, 1)), uv, ident)
    s = np.linspace(-1.0, 1.0, 40)
    line = np.stack([3.0 * s, 1.0 * s + 0.2, 10.0 + 4.0 * s], 1).astype(np.float32)
    cases["collinear points"] = (line, (line[:, :2] / line[:, 2:3]).astype(np.float32), ident)
    p3, p2, g, _, _ = scene(40, 77, 0.0)
    back = g.copy(); back[3:] = P.qnormalise(P.qmul(g[3:], np.array([0.0, 1.0, 0.0, 0.0])))      # half a turn about y: everything is behind
    back[:3] = -back[:3]
    cases["every point behind the guess camera"] = (p3, p2, back)
    nan = p2.copy(); nan[:] = np.nan
    cases["NaN in every observation"] = (p3, nan, g)
    return cases
