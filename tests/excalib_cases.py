"""tests/excalib_cases.py -- scenes with known truth for the camera-LiDAR rotation calibration, and the case-file writer
of lmono_amd/host/excalib_test.  A scene is a rig that moves through points at 5-40 m depth: per frame the pairs of normalised image
points before and after a known camera motion, and the LiDAR's rotation increment of the same motion under the true extrinsic.  The
true extrinsic is far from the identity: camera z forward against LiDAR x forward."""
import struct

import numpy as np

from tests import excalib_ref as X
from workloads.s7 import rodrigues

# rlc: camera coordinates -> LiDAR coordinates (camera x = LiDAR -y, camera y = LiDAR -z, camera z = LiDAR x), turned a little so that
# it is no axis permutation
FOCAL = 460.0


def proper(R):
    """The nearest rotation (the products above are rotations to rounding only)."""
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


RLC_TRUE = proper(np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ rodrigues([0.3, -0.5, 0.8], np.deg2rad(7.0)))


def angle_between(A, B):
    """Radians between two rotations [3, 3] (atan2 form: accurate near zero)."""
    D = np.asarray(A).reshape(3, 3).T @ np.asarray(B).reshape(3, 3)
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def frame(rng, m, angle, axis, noise_px=0.0):
    """One frame: m pairs [m, 4] of points at 5-40 m seen before and after the camera turns by `angle` about `axis` and moves 0.3-1 m;
    -> (pairs, R_c: the camera's rotation increment R_{c,k-1}^T R_{c,k}, q_lidar x y z w of rlc R_c rlc^T)."""
    Rc = proper(rodrigues(axis, angle))
    p = rng.normal(size=3); p = p / np.linalg.norm(p) * rng.uniform(0.3, 1.0)
    pts = []
    while len(pts) < m:
        z = rng.uniform(5.0, 40.0)
        Xp = np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.4, 0.4) * z, z])
        Xc = Rc.T @ (Xp - p)
        if Xc[2] > 1.0:
            pts.append((Xp, Xc))
    pairs = np.array([[a[0] / a[2], a[1] / a[2], b[0] / b[2], b[1] / b[2]] for a, b in pts])
    if noise_px > 0.0:
        pairs = pairs + rng.normal(0.0, noise_px / FOCAL, pairs.shape)
    Rl = proper(RLC_TRUE @ Rc @ RLC_TRUE.T)
    return pairs, Rc, np.array(X.m2q(Rl))


def scene(seed, m, n_frames, ang_lo_deg, ang_hi_deg, noise_px=0.0, yaw_only=False):
    """-> list of (pairs, R_c, q_lidar).  Axes change from frame to frame (yaw_only: every turn is about the LiDAR's z)."""
    rng = np.random.default_rng(9100 + seed)
    out = []
    for _ in range(n_frames):
        axis = RLC_TRUE.T @ np.array([0.0, 0.0, 1.0]) if yaw_only else rng.normal(size=3)
        ms = m if np.isscalar(m) else int(rng.choice(m))
        out.append(frame(rng, ms, np.deg2rad(rng.uniform(ang_lo_deg, ang_hi_deg)), axis, noise_px))
    return out


def rotation_pairs(seed, n_frames, ang_lo_deg=8.0, ang_hi_deg=12.0, outlier_at=None, outlier_deg=20.0, small_first=0):
    """Consistent (q_cam, q_lidar) pairs for the stage-4 tests; at frame index `outlier_at` the camera rotation is turned by outlier_deg.
    The first `small_first` frames turn by 2.3-2.49 degrees only: two rotations of angle t are at most 2 t apart, so their Huber weights
    are exactly 1 whatever rlc is."""
    rng = np.random.default_rng(9500 + seed)
    out = []
    for k in range(n_frames):
        lo, hi = (2.3, 2.49) if k < small_first else (ang_lo_deg, ang_hi_deg)
        Rc = proper(rodrigues(rng.normal(size=3), np.deg2rad(rng.uniform(lo, hi))))
        Rl = proper(RLC_TRUE @ Rc @ RLC_TRUE.T)
        if outlier_at is not None and k == outlier_at:
            Rc = proper(Rc @ rodrigues(rng.normal(size=3), np.deg2rad(outlier_deg)))
        out.append((np.array(X.m2q(Rc)), np.array(X.m2q(Rl))))
    return out


M_MIX = [0, 8, 9, 150, 512, 33, 64, 65, 10, 100]


def batch_scenes(n, n_frames=3):
    """The streams of the batching test: n scenes of mixed m (0, 8, 9, 150 and 512 among them; one stream: 150)."""
    return [scene(500 + 7 * s, M_MIX[(s + n) % len(M_MIX)] if n > 1 else 150, n_frames, 4.0, 9.0) for s in range(n)]


def degenerate_cases():
    """Named stage 1-3 inputs that are no scene: -> dict name -> pairs [m, 4]."""
    rng = np.random.default_rng(77)
    base, Rc, _ = frame(rng, 40, np.deg2rad(6.0), [0.2, 1.0, -0.3])
    ident = np.tile(base[:1], (20, 1))
    # pure rotation: the second view is the first turned, no translation
    P = np.column_stack([base[:, 0], base[:, 1], np.ones(len(base))])
    Q = (Rc.T @ P.T).T
    pure = np.column_stack([base[:, :2], Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2]])
    s = np.linspace(-0.4, 0.4, 30)
    coll = np.column_stack([s, 0.5 * s + 0.1, s + 0.02, 0.5 * s + 0.13])
    nan = base.copy(); nan[7, 2] = np.nan
    return {"identical": ident, "pure_rotation": pure, "collinear": coll, "one_nan": nan, "empty": np.zeros((0, 4))}


def write_cases(path, sequences):
    """sequences: list of (count, frames), a frame = (kind, pairs [m, 4], q_cam [4] or None, q_lidar [4] or None) -> the file excalib_test reads."""
    with open(str(path), "wb") as f:
        f.write(struct.pack("<i", len(sequences)))
        for count, frames in sequences:
            f.write(struct.pack("<ii", int(count), len(frames)))
            for kind, pairs, q_cam, q_lidar in frames:
                P = np.ascontiguousarray(pairs, np.float64).reshape(-1, 4)
                f.write(struct.pack("<ii", int(kind), len(P)))
                f.write(P.tobytes())
                f.write(np.asarray([0, 0, 0, 1] if q_cam is None else q_cam, np.float64).tobytes())
                f.write(np.asarray([0, 0, 0, 1] if q_lidar is None else q_lidar, np.float64).tobytes())


def parse_results(text):
    """excalib_test's stdout -> list of ("REL", R [9], stats [6]) / ("CAL", rlc [9], sv [4], huber, ok, frame_count, M [16])."""
    out = []
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "REL":
            out.append(("REL", np.array([float(v) for v in w[1:10]]), np.array([int(v) for v in w[10:16]], np.int32)))
        elif w[0] == "CAL":
            v = [float(t) for t in w[1:]]
            out.append(("CAL", np.array(v[0:9]), np.array(v[9:13]), v[13], bool(int(v[14])), int(v[15]), np.array(v[16:32])))
    return out
