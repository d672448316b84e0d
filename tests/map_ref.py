"""An independent numpy reference of the scan-to-map refine step (lmono_map_refine; oracle/lo_mapping.c lo_map_refine).

It restates the OPERATION, not the kernel's algorithm: the 5-NN search is brute force over the whole cloud (no grid, no 27 cells), the line test
takes its eigenvalues from numpy.linalg.eigh (no Jacobi sweeps), the plane fit is numpy.linalg.lstsq (no Householder code), the Jacobians of the
solve are closed forms summed by numpy.  Only what the operation itself fixes is shared with the kernel and the oracle: the float32 distance
((dx*dx) + (dy*dy)) + (dz*dz) ordered by (distance, index), the float32 query point (a double transform stored in a float point, Eigen's
quaternion-times-vector), the gates' constants and the trust-region loop of ceres::Solve with its constants.

Test infrastructure: imported by tests/map_cases.py, tests/test_map_ref_cpu.py and tests/test_map_refine_edges_gpu.py only."""
import collections

import numpy as np

_WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


# ---- search ----------------------------------------------------------------------------------------------------------------
def knn5_many(cloud, Q):
    """Rows of the five nearest cloud points of every query of Q [m,3] float32 by (float32 squared distance, index); a row of -1 where fewer than
    five points exist or the fifth squared distance is not < 1.0."""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    Q = np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    out = np.full((len(Q), 5), -1, np.int32)
    if len(cloud) < 5:
        return out
    cx, cy, cz = cloud[:, 0][None], cloud[:, 1][None], cloud[:, 2][None]
    for c0 in range(0, len(Q), 256):
        q = Q[c0:c0 + 256]
        dx = cx - q[:, 0:1]; dy = cy - q[:, 1:2]; dz = cz - q[:, 2:3]
        d = ((dx * dx) + (dy * dy)) + (dz * dz)
        assert d.dtype == np.float32
        fifth = np.partition(d, 4, axis=1)[:, 4]
        for r in np.nonzero(fifth.astype(np.float64) < 1.0)[0]:
            cand = np.nonzero(d[r] <= fifth[r])[0]                     # ascending indices
            out[c0 + r] = cand[np.argsort(d[r, cand], kind="stable")[:5]]
    return out


def knn5(cloud, q):
    """The five nearest points of one query, or None when the search refuses it."""
    row = knn5_many(cloud, np.asarray(q, np.float32).reshape(1, 3))[0]
    return None if row[0] < 0 else row


def associate(x, pts):
    """pointAssociateToMap: q * p + t in double (Eigen: v + w uv + u x uv, uv = 2 u x v), stored in a float point."""
    v = np.asarray(pts, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    u, w = np.asarray(x[:3], np.float64), float(x[3])
    uv = 2.0 * np.cross(u[None], v)
    r = v + w * uv + np.cross(u[None], uv)
    return (r + np.asarray(x[4:7], np.float64)[None]).astype(np.float32)


# ---- gates -----------------------------------------------------------------------------------------------------------------
LineGate = collections.namedtuple("LineGate", "ok margin direction ev centre")
PlaneGate = collections.namedtuple("PlaneGate", "ok margin normal d max_dist")


def line_gate(P5):
    """The line test on five points [5,3]: covariance about the mean (a sum, not a mean, as in laserMapping), ascending eigenvalues, accepted when
    ev2 > 3 ev1.  margin = |ev2 - 3 ev1| / ev2 (0 when ev2 is 0)."""
    P = np.asarray(P5, np.float64).reshape(5, 3)
    Pw = P.astype(_WIDE)
    c = Pw.sum(axis=0) / _WIDE(5)
    Z = Pw - c
    cov = (Z.T @ Z).astype(np.float64)
    ev, vec = np.linalg.eigh(cov)
    ev = np.maximum(ev, 0.0)
    ok = bool(ev[2] > 3.0 * ev[1])
    margin = float(abs(ev[2] - 3.0 * ev[1]) / ev[2]) if ev[2] > 0 else 0.0
    return LineGate(ok, margin, vec[:, 2].copy(), ev, c.astype(np.float64))


def plane_gate(P5):
    """The plane fit on five points: x = argmin |P x + 1| (minimum norm where P is rank deficient), unit normal x / |x|, offset 1 / |x|; accepted
    when no point is farther than 0.2 from the plane.  margin = |max distance - 0.2|."""
    P = np.asarray(P5, np.float64).reshape(5, 3)
    x = np.linalg.lstsq(P, -np.ones(5), rcond=None)[0]
    # one round of iterative refinement, the residual in the widest type at hand (a fit of five points a few centimetres apart, metres from the
    # origin, has a condition number of some hundreds)
    res = (P.astype(_WIDE) @ x.astype(_WIDE) + _WIDE(1)).astype(np.float64)
    x = x - np.linalg.lstsq(P, res, rcond=None)[0]
    nn = float(np.sqrt((x * x).sum()))
    n, d = x / nn, 1.0 / nn
    dist = np.abs(P @ n + d)
    md = float(dist.max())
    return PlaneGate(bool(md <= 0.2), abs(md - 0.2), n, d, md)


# ---- solve -----------------------------------------------------------------------------------------------------------------
Blocks = collections.namedtuple("Blocks", "kind cp a b")       # kind 1 edge (a, b line points), 3 plane-norm (b normal, a[0] offset)


def empty_blocks():
    return Blocks(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))


def _rot(x):
    ux, uy, uz, w = x[:4]
    return np.array([[1 - 2 * (uy * uy + uz * uz), 2 * (ux * uy - w * uz), 2 * (ux * uz + w * uy)],
                     [2 * (ux * uy + w * uz), 1 - 2 * (ux * ux + uz * uz), 2 * (uy * uz - w * ux)],
                     [2 * (ux * uz - w * uy), 2 * (uy * uz + w * ux), 1 - 2 * (ux * ux + uy * uy)]])


def _plus(x, delta):
    """EigenQuaternionParameterization::Plus (delta_q * q) and the identity on t."""
    out = np.array(x, np.float64)
    nd = float(np.sqrt((delta[:3] ** 2).sum()))
    if nd > 0.0:
        s = np.sin(nd) / nd
        a = np.array([s * delta[0], s * delta[1], s * delta[2], np.cos(nd)]); b = x[:4]
        out[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
        out[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
        out[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
        out[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    out[4:] = x[4:] + delta[3:]
    return out


def evaluate(blocks, x, want_jac=True):
    """Huber(0.1)-corrected cost and, optionally, H = J^T J, g = J^T r over the local parameters (rotation: x <- exp(delta) x, so a point moves by
    2 delta x (R v); translation: identity)."""
    if len(blocks.kind) == 0:
        return 0.0, np.zeros((6, 6)), np.zeros(6)
    rv = blocks.cp @ _rot(x).T
    lp = rv + x[4:7][None]
    edge = blocks.kind == 1
    rows_r, rows_d, rows_rv, rows_blk = [], [], [], []
    sq = np.zeros(len(blocks.kind))
    if edge.any():
        A = lp[edge] - blocks.a[edge]; B = lp[edge] - blocks.b[edge]
        E = blocks.a[edge] - blocks.b[edge]
        den = np.sqrt((E * E).sum(axis=1))[:, None]
        r = np.cross(A, B) / den
        sq[edge] = (r * r).sum(axis=1)
        e = E / den
        z = np.zeros(len(e))
        D = [np.stack([z, e[:, 2], -e[:, 1]], 1), np.stack([-e[:, 2], z, e[:, 0]], 1), np.stack([e[:, 1], -e[:, 0], z], 1)]   # r = u x e
        for k in range(3):
            rows_r.append(r[:, k]); rows_d.append(D[k]); rows_rv.append(rv[edge]); rows_blk.append(np.nonzero(edge)[0])
    pl = ~edge
    if pl.any():
        r0 = (blocks.b[pl] * lp[pl]).sum(axis=1) + blocks.a[pl, 0]
        sq[pl] = r0 * r0
        rows_r.append(r0); rows_d.append(blocks.b[pl]); rows_rv.append(rv[pl]); rows_blk.append(np.nonzero(pl)[0])
    out = sq > 0.01
    root = np.sqrt(np.where(out, sq, 1.0))
    rho0 = np.where(out, 0.2 * root - 0.01, sq)
    rho1 = np.where(out, np.maximum(0.1 / root, np.finfo(np.float64).tiny), 1.0)
    cost = float(0.5 * rho0.sum())
    if not want_jac:
        return cost, None, None
    r = np.concatenate(rows_r); d = np.concatenate(rows_d); rvr = np.concatenate(rows_rv); blk = np.concatenate(rows_blk)
    sr = np.sqrt(rho1[blk])
    J = np.concatenate([2.0 * np.cross(rvr, d), d], axis=1) * sr[:, None]
    rs = r * sr
    return cost, J.T @ J, J.T @ rs


def huber_linear_share(blocks, x):
    """Share of the residual blocks that sit in Huber's linear part at x."""
    if len(blocks.kind) == 0:
        return 0.0
    rv = blocks.cp @ _rot(x).T + x[4:7][None]
    edge = blocks.kind == 1
    sq = np.zeros(len(blocks.kind))
    if edge.any():
        E = blocks.a[edge] - blocks.b[edge]
        r = np.cross(rv[edge] - blocks.a[edge], rv[edge] - blocks.b[edge]) / np.sqrt((E * E).sum(axis=1))[:, None]
        sq[edge] = (r * r).sum(axis=1)
    if (~edge).any():
        sq[~edge] = ((blocks.b[~edge] * rv[~edge]).sum(axis=1) + blocks.a[~edge, 0]) ** 2
    return float((sq > 0.01).mean())


def lm_solve(blocks, x0):
    """ceres::Solve as laserMapping configures it (trust region, Levenberg-Marquardt, four iterations, Huber 0.1), restated in float64 from
    oracle/lo_odometry.c lo_lm_solve and the comments of k_map_solve.  Returns (pose, iterations, trace): the trace lists, in order, every way the
    loop took out of or around an iteration."""
    max_iter = 4
    function_tol, gradient_tol, parameter_tol = 1e-6, 1e-10, 1e-8
    min_rel_decrease, min_diag, max_diag, max_radius, min_radius = 1e-3, 1e-6, 1e32, 1e16, 1e-32
    radius, decrease_factor = 1e4, 2.0
    reuse_diagonal, invalid_steps = False, 0
    x = np.array(x0, np.float64)
    trace = []
    if len(blocks.kind) == 0:
        return x, 0, ["n_used_zero"]
    x_cost, H, g = evaluate(blocks, x)
    x_norm = float(np.sqrt((x * x).sum()))
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    if np.abs(g).max() <= gradient_tol:
        return x, 0, ["grad_exit_start"]
    diag = np.zeros(6)
    it = 0
    while it < max_iter:
        it += 1
        gs = g * scale
        Hs = H * scale[:, None] * scale[None, :]
        if not reuse_diagonal:
            diag = np.clip(np.diag(Hs), min_diag, max_diag)
        elif "reuse_diagonal" not in trace:
            trace.append("reuse_diagonal")
        ok, model_change = True, 0.0
        try:
            L = np.linalg.cholesky(Hs + np.diag(diag / radius))
            step = -np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.isfinite(step).all())
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            model_change = -(float(step @ gs) + 0.5 * float(step @ Hs @ step))
        if not ok or not model_change > 0.0:
            trace.append("invalid")
            invalid_steps += 1
            if invalid_steps >= 5:
                trace.append("invalid_limit")
                break
            radius *= 0.5; reuse_diagonal = True
            continue
        invalid_steps = 0
        cand = _plus(x, step * scale)
        last = it == max_iter
        if last:
            trace.append("cost_only_last")           # the candidate of the last iteration is never linearised: its cost alone decides
        cand_cost, Hc, gc = evaluate(blocks, cand, want_jac=not last)
        if float(np.sqrt(((x - cand) ** 2).sum())) <= parameter_tol * (x_norm + parameter_tol):
            trace.append("param_tol")
            break
        if abs(x_cost - cand_cost) <= function_tol * x_cost:
            trace.append("func_tol")
            break
        rel = (x_cost - cand_cost) / model_change
        if rel > min_rel_decrease:
            trace.append("accept")
            x = cand
            if last:
                break
            x_norm = float(np.sqrt((x * x).sum()))
            x_cost, H, g = cand_cost, Hc, gc
            t = 2.0 * rel - 1.0
            radius = min(radius / max(1.0 - t * t * t, 1.0 / 3.0), max_radius)
            decrease_factor, reuse_diagonal = 2.0, False
            if np.abs(g).max() <= gradient_tol:
                trace.append("grad_exit_step")
                break
        else:
            trace.append("reject")
            radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = True
        if radius <= min_radius:
            trace.append("min_radius")
            break
    else:
        trace.append("max_iter")
    return x, it, trace


# ---- the whole step --------------------------------------------------------------------------------------------------------
Refined = collections.namedtuple("Refined", "pose stats nn traces x_mid")


def build_blocks(cmap, smap, cstack, sstack, x):
    """One outer iteration's search and gates at pose x: (Blocks, nn table [n_cs + n_ss, 5] with -1 rows for points without a block, n_edge,
    n_plane, margins of the corner queries that reached the line gate {query: LineGate}, the same for the plane gate)."""
    cmap = np.ascontiguousarray(cmap, np.float32).reshape(-1, 4); smap = np.ascontiguousarray(smap, np.float32).reshape(-1, 4)
    cstack = np.ascontiguousarray(cstack, np.float32).reshape(-1, 4); sstack = np.ascontiguousarray(sstack, np.float32).reshape(-1, 4)
    ncs = len(cstack)
    nn = np.full((ncs + len(sstack), 5), -1, np.int32)
    kind, cp, a, b = [], [], [], []
    lg, pg = {}, {}
    rows = knn5_many(cmap, associate(x, cstack))
    for i in np.nonzero(rows[:, 0] >= 0)[0]:
        gate = line_gate(cmap[rows[i], :3])
        lg[int(i)] = gate
        if gate.ok:
            nn[i] = rows[i]
            kind.append(1); cp.append(cstack[i, :3].astype(np.float64)); a.append(gate.centre + 0.1 * gate.direction); b.append(gate.centre - 0.1 * gate.direction)
    n_edge = len(kind)
    rows = knn5_many(smap, associate(x, sstack))
    for i in np.nonzero(rows[:, 0] >= 0)[0]:
        gate = plane_gate(smap[rows[i], :3])
        pg[int(i)] = gate
        if gate.ok:
            nn[ncs + i] = rows[i]
            kind.append(3); cp.append(sstack[i, :3].astype(np.float64)); a.append(np.array([gate.d, 0.0, 0.0])); b.append(gate.normal)
    if not kind:
        return empty_blocks(), nn, 0, 0, lg, pg
    return Blocks(np.array(kind, np.int32), np.array(cp), np.array(a), np.array(b)), nn, n_edge, len(kind) - n_edge, lg, pg


def refine(cmap, smap, cstack, sstack, x0):
    """Two outer iterations of [search, gates, solve].  Returns Refined(pose, the six stats n_edge[2] n_plane[2] lm_iters[2], the neighbour table
    of the last outer iteration, the two solve traces, the pose between the two)."""
    x = np.array(x0, np.float64)
    n_q = len(np.asarray(cstack).reshape(-1, 4)) + len(np.asarray(sstack).reshape(-1, 4))
    if not (len(np.asarray(cmap).reshape(-1, 4)) > 10 and len(np.asarray(smap).reshape(-1, 4)) > 50):
        return Refined(x, [0] * 6, np.full((n_q, 5), -1, np.int32), [["skipped"], ["skipped"]], x.copy())
    stats = [0] * 6
    traces = []
    x_mid = x.copy()
    for outer in range(2):
        if outer == 1:
            x_mid = x.copy()
        blocks, nn, ne, npl, lg, pg = build_blocks(cmap, smap, cstack, sstack, x)
        x, it, tr = lm_solve(blocks, x)
        stats[outer], stats[2 + outer], stats[4 + outer] = ne, npl, it
        traces.append(tr)
    return Refined(x, stats, nn, traces, x_mid)
