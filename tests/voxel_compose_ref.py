"""Composing voxel maps under rigid transforms restated in numpy from the definition, not from the kernel, on top of
tests/voxel_map_ref.py: Python floats (IEEE doubles, one operation at a time) for the transform, Python integers for the sums.
The checker of the compose tests."""
import numpy as np

from tests import voxel_map_ref as R

F32 = np.float32


def move_points(p, T):
    """T (3 x 4 fp64) applied to float32 points p: per row ((T0 x + T1 y) + T2 z) + T3 in fp64, in this order, then one cast."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    out = p.copy()
    for n in range(len(p)):
        x, y, z = float(p["x"][n]), float(p["y"][n]), float(p["z"][n])
        for a, name in enumerate(("x", "y", "z")):
            t = [float(v) for v in T[a]]
            with np.errstate(all="ignore"):
                out[name][n] = F32(((t[0] * x + t[1] * y) + t[2] * z) + t[3])
    return out


def compose(dst_ref, src_refs, transforms):
    """Fold the VoxelMapRefs `src_refs`, each moved by its transform, into dst_ref.  Returns [source voxels moved, source voxels rejected,
    points moved, points rejected, voxels new, voxels afterwards]."""
    T = np.asarray(transforms, np.float64).reshape(len(src_refs), 12)
    st = [0, 0, 0, 0, 0, 0]
    before = len(dst_ref.table)
    for s, src in enumerate(src_refs):
        keys = sorted(src.table)
        if not keys:
            continue
        moved = move_points(src.read(), T[s])                      # read(): the float32 point of each voxel, ascending key order
        ok, i, q = R.cell_of(moved, dst_ref.leaf)
        dkeys = R.key_of(i)
        for n, k in enumerate(keys):
            r = src.table[k]
            c = r[0]
            if not ok[n]:
                st[1] += 1; st[3] += c
                continue
            st[0] += 1; st[2] += c
            d = dst_ref.table.setdefault(int(dkeys[n]), [0] * 7)
            d[0] += c
            for a in range(3):
                d[1 + a] += c * int(q[n, a])
                d[4 + a] += r[4 + a]
    st[4] = len(dst_ref.table) - before
    st[5] = len(dst_ref.table)
    return st


def text(dst_ref, st):
    """What lmono_amd/host/voxel_compose_test prints."""
    return "rejected %d %d\n" % (st[1], st[3]) + dst_ref.text().split("\n", 1)[1]


def _pose_matrix(tq):
    tq = np.asarray(tq, np.float64).reshape(7)
    x, y, z, w = tq[3:] / np.sqrt((tq[3:] * tq[3:]).sum())
    Rm = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                   [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                   [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]], np.float64)
    return Rm, tq[:3].copy()


def pose_delta(inserted_tq, corrected_tq):
    """T_corrected * T_inserted^-1 as [12] fp64 from two (x y z, qx qy qz qw) poses: D_R = R_c R_i^T, D_t = t_c - D_R t_i, sums left to right."""
    Ri, ti = _pose_matrix(inserted_tq)
    Rc, tc = _pose_matrix(corrected_tq)
    D = np.zeros((3, 4), np.float64)
    for a in range(3):
        for b in range(3):
            D[a, b] = (Rc[a, 0] * Ri[b, 0] + Rc[a, 1] * Ri[b, 1]) + Rc[a, 2] * Ri[b, 2]
        D[a, 3] = tc[a] - ((D[a, 0] * ti[0] + D[a, 1] * ti[1]) + D[a, 2] * ti[2])
    return D.reshape(12)


def rigid(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """[12] fp64: Rz(yaw) Ry(pitch) Rx(roll) and a translation."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]); Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]); Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(t, np.float64).reshape(3, 1)], 1).reshape(12)


IDENTITY = rigid()


def pose_tq(xyz, yaw):
    """(x y z, qx qy qz qw) of a pose at xyz turned by yaw about z."""
    return np.array([xyz[0], xyz[1], xyz[2], 0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)], np.float64)


def transform_points(p, tq):
    """Sensor-frame float32 points into the world of pose tq, in fp64 with one cast (how the corridor frames below are made)."""
    Rm, t = _pose_matrix(tq)
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64) @ Rm.T + t
    return R.points(xyz.astype(np.float32), p["bgra"])


# ---- the small synthetic world of the end-to-end bound: a 40 m corridor of two walls and a floor, 18 000 points ----
CORRIDOR = dict(length=40.0, half_width=2.0, height=3.0, n=18000, frames=6, radius=8.0, per_submap=2, leaf_sub=0.05, leaf=0.1,
                drift_t=0.9, drift_yaw=0.03)


def corridor_world(seed=3):
    c = CORRIDOR
    rng = np.random.default_rng(seed)
    n = c["n"] // 3
    x = rng.uniform(0.0, c["length"], (3, n))
    left = np.stack([x[0], np.full(n, c["half_width"]), rng.uniform(0.0, c["height"], n)], 1)
    right = np.stack([x[1], np.full(n, -c["half_width"]), rng.uniform(0.0, c["height"], n)], 1)
    floor = np.stack([x[2], rng.uniform(-c["half_width"], c["half_width"], n), np.zeros(n)], 1)
    xyz = np.concatenate([left, right, floor]).astype(np.float32)
    return R.points(xyz, rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))


def corridor_case(seed=3):
    """world, true poses [6][7], drifted poses [6][7], frames: per frame the world points within radius of the true position, expressed in the
    sensor frame of the TRUE pose and then mapped with the DRIFTED pose -- what a mapper with drifting odometry inserts.  Drift jumps by
    drift_t / drift_yaw at submap boundaries only, so every submap is rigid."""
    c = CORRIDOR
    world = corridor_world(seed)
    wxyz = np.stack([world["x"], world["y"], world["z"]], 1).astype(np.float64)
    true, drifted, frames = [], [], []
    for f in range(c["frames"]):
        pos = np.array([4.0 + 6.4 * f, 0.0, 1.0])
        yaw = 0.02 * f
        tq = pose_tq(pos, yaw)
        k = f // c["per_submap"]                                    # accumulated jumps: the world of submap k is turned by k drift_yaw about its
        anchor = np.array([4.0 + 6.4 * k * c["per_submap"], 0.0, 1.0])                              # anchor and shifted by k drift_t along y
        dy = c["drift_yaw"] * k
        rel = pos - anchor
        turned = np.array([np.cos(dy) * rel[0] - np.sin(dy) * rel[1], np.sin(dy) * rel[0] + np.cos(dy) * rel[1], rel[2]])
        dq = pose_tq(anchor + turned + np.array([0.0, c["drift_t"] * k, 0.0]), yaw + dy)
        sel = np.linalg.norm(wxyz - pos, axis=1) <= c["radius"]
        Rm, t = _pose_matrix(tq)
        local = (wxyz[sel] - t) @ Rm                                # R^T (w - t)
        lp = R.points(local.astype(np.float32), world["bgra"][sel])
        true.append(tq); drifted.append(dq); frames.append(transform_points(lp, dq))
    return world, np.array(true), np.array(drifted), frames


def corridor_bound():
    """sqrt(3) (leaf_sub + leaf) + 1e-3 m: a voxel's point is a mean of points of its cell, twice over (two cell diagonals); the 1e-3 covers the
    2^-16-leaf steps and the float32 roundings below 50 m."""
    return np.sqrt(3.0) * (CORRIDOR["leaf_sub"] + CORRIDOR["leaf"]) + 1e-3


def distance_to_world(points, world):
    """Per point: distance to the nearest world point (brute force in blocks)."""
    a = np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float64)
    w = np.stack([world["x"], world["y"], world["z"]], 1).astype(np.float64)
    out = np.empty(len(a))
    for s in range(0, len(a), 1024):
        b = a[s:s + 1024]
        near = ((b * b).sum(1)[:, None] + (w * w).sum(1)[None, :] - 2.0 * (b @ w.T)).argmin(1)     # |a|^2 + |w|^2 - 2 a.w picks the candidate ...
        out[s:s + 1024] = np.sqrt(((b - w[near]) ** 2).sum(1))                                       # ... its distance is computed directly
    return out


def corridor_reference():
    """The corridor case through the restatement: (world, true, drifted, frames, submaps, composed map, its stats, the uncomposed map)."""
    c = CORRIDOR
    world, true, drifted, frames = corridor_case()
    subs = []
    plain = R.VoxelMapRef(c["leaf"])
    for f, p in enumerate(frames):
        if f % c["per_submap"] == 0:
            subs.append(R.VoxelMapRef(c["leaf_sub"]))
        subs[-1].insert(p)
        plain.insert(p)
    T = [pose_delta(drifted[k * c["per_submap"]], true[k * c["per_submap"]]) for k in range(len(subs))]
    dst = R.VoxelMapRef(c["leaf"])
    st = compose(dst, subs, T)
    return dict(world=world, true=true, drifted=drifted, frames=frames, subs=subs, dst=dst, stats=st, plain=plain)
