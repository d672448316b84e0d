"""workloads/s7.py -- synthetic workload S7: a hand-held camera-LiDAR rig whose extrinsic rotation is unknown (ESTIMATE_LASER == 2,
DESIGN.md 6i).  The rig turns by a chosen angle range per frame about changing axes -- the motion hand-eye calibration needs; a car that
only yaws cannot calibrate -- among landmarks that lie in a shell of 5-40 m around the path, in all directions.  Input plumbing for tests
and scripts/excalib_bench.py; the frame stream has the layout of workloads/s2.make_stream and is written by s2.write_stream."""
import numpy as np

from workloads import s2


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def true_extrinsic():
    """kitti_extrinsic() with its 3 x 3 block made an exact rotation the way the Estimator does (Quaterniond, normalised) -> 4 x 4."""
    T = s2.kitti_extrinsic()
    q = s2.R_to_q(T[:3, :3])
    T[:3, :3] = s2.quat_R(q / np.linalg.norm(q))
    return T


def make_stream(n_frames=25, seed=0, angle_deg=(8.0, 12.0), yaw_only=False, n_landmarks=8000, max_tracks=150, pix_sigma=0.0, death=0.02, min_dist=30.0,
                speed=0.3):
    """-> the dict of s2.make_stream: headers [n], L0 [n, 4, 4] (the LiDAR poses, exact), feats (list of {id: (x_n, y_n, u, v)}), gt_R, gt_P
    in the Estimator world of the TRUE extrinsic, tlc: the extrinsic the run starts from -- the true translation with the IDENTITY rotation --
    and tlc_true [4, 4].  angle_deg: the range of the rotation per frame; yaw_only: every rotation is about the LiDAR's z."""
    rng = np.random.default_rng(70001 + 7919 * seed)
    T = true_extrinsic()
    Rlc, tlc = T[:3, :3], T[:3, 3]
    L0_R, L0_P = [np.eye(3)], [np.zeros(3)]
    for k in range(1, n_frames):
        axis = np.array([0.0, 0.0, 1.0]) if yaw_only else rng.normal(size=3)
        ang = np.deg2rad(rng.uniform(*angle_deg)) * (1.0 if yaw_only else rng.choice([-1.0, 1.0]))
        step = np.array([speed, 0.0, 0.0]) + rng.normal(0.0, 0.25 * speed, 3)
        L0_P.append(L0_P[-1] + L0_R[-1] @ step)
        U, _, Vt = np.linalg.svd(L0_R[-1] @ rodrigues(axis, ang))
        L0_R.append(U @ Vt)
    Rs = [Rlc.T @ R for R in L0_R]; Ps = [Rlc.T @ (P - tlc) for P in L0_P]
    cam_R = [Rs[k] @ Rlc for k in range(n_frames)]; cam_P = [Ps[k] + Rs[k] @ tlc for k in range(n_frames)]
    # landmarks: a shell of 5-40 m around points of the path, in all directions (Estimator world)
    d = rng.normal(size=(n_landmarks, 3)); d = d / np.linalg.norm(d, axis=1)[:, None]
    lm = np.array(cam_P)[rng.integers(0, n_frames, n_landmarks)] + d * rng.uniform(5.0, 40.0, n_landmarks)[:, None]
    feats, alive, seen = [], [], set()
    for k in range(n_frames):
        pc = (cam_R[k].T @ (lm - cam_P[k]).T).T
        z = pc[:, 2]
        zs = np.where(z > 1e-6, z, 1.0)
        u = s2.FX * pc[:, 0] / zs + s2.CX; v = s2.FY * pc[:, 1] / zs + s2.CY
        vis = (z > 1.0) & (u > 0) & (u < s2.W_IMG) & (v > 0) & (v < s2.H_IMG)
        alive = [t for t in alive if vis[t] and rng.uniform() > death]
        cand = [t for t in np.nonzero(vis)[0] if t not in seen]
        rng.shuffle(cand)
        taken = np.array([(u[t], v[t]) for t in alive]).reshape(-1, 2)
        for t in cand[:500]:
            if len(alive) >= max_tracks:
                break
            if len(taken) == 0 or ((taken[:, 0] - u[t]) ** 2 + (taken[:, 1] - v[t]) ** 2).min() > min_dist ** 2:
                alive.append(t); seen.add(t); taken = np.concatenate([taken, [[u[t], v[t]]]])
        fr = {}
        for t in alive:
            uu = u[t] + (rng.normal(0, pix_sigma) if pix_sigma > 0 else 0.0); vv = v[t] + (rng.normal(0, pix_sigma) if pix_sigma > 0 else 0.0)
            fr[int(t)] = ((uu - s2.CX) / s2.FX, (vv - s2.CY) / s2.FY, uu, vv)
        feats.append(fr)
    L0 = np.zeros((n_frames, 4, 4))
    for k in range(n_frames):
        L0[k] = np.eye(4); L0[k, :3, :3] = L0_R[k]; L0[k, :3, 3] = L0_P[k]
    start = np.eye(4); start[:3, 3] = tlc
    return dict(headers=0.1 * np.arange(n_frames), L0=L0, feats=feats, gt_R=np.array(Rs), gt_P=np.array(Ps), tlc=start, tlc_true=T)


def frame_pairs(st, k):
    """What FeatureManager::getCorresponding(k - 1, k) returns while no track has been removed: the tracks seen in both frames, in the
    feature list's order (a frame's new tracks are appended in ascending id) -> [m, 4]."""
    first = {}
    for f in range(k + 1):
        for i in st["feats"][f]:
            first.setdefault(i, f)
    a, b = st["feats"][k - 1], st["feats"][k]
    ids = sorted((i for i in a if i in b), key=lambda i: (first[i], i))
    return np.array([[a[i][0], a[i][1], b[i][0], b[i][1]] for i in ids], np.float64).reshape(-1, 4)
