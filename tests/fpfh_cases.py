"""The cases of the FPFH tests: name -> (points, keyword arguments of normals_ref.run / SurfaceNormals, keypoints [m][3] float32,
keyword arguments of fpfh_ref.run / FpfhDescriptors).  Shared by the CPU test (restatement against host/fpfh_test, and what each case claims to be)
and the GPU test (device against the restatement).  Every case has at most about 1500 points and 200 keypoints."""
import numpy as np

from tests import icp_cases as IC
from tests import normals_cases as NC

F32 = np.float32
pts = IC.pts
SCENE_R = IC.rotation((0.2, -0.1, 1.0), 40.0)
SCENE_T = np.array([0.8, -0.5, 0.33])              # 1 m


def xyz_of(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def _every(p, step, first=0):
    return xyz_of(p)[first::step].copy()


def _scene_xyz(seed):
    """A floor, a wall, a sloped roof on one side and a quarter cylinder on the other: no symmetry.  About 1100 points at 0.125 m with 5 mm of jitter."""
    g = 0.125
    floor = np.array([(g * i, g * j, 0.0) for i in range(25) for j in range(25)])
    wall = np.array([(0.0, g * j, g * k) for j in range(25) for k in range(1, 13)])
    roof = np.array([(1.0 + g * i, 0.5 + g * j, 0.2 + 0.5 * g * i + 0.25 * g * j) for i in range(10) for j in range(8)])
    a = np.linspace(0.0, np.pi / 2, 9)
    cyl = np.array([(2.2 + 0.6 * np.cos(t), 2.0 + g * j, 0.6 * np.sin(t) + 0.02) for t in a for j in range(8)])
    xyz = np.concatenate([floor, wall, roof, cyl])
    return xyz + np.random.default_rng(seed).normal(0.0, 0.005, xyz.shape)


SCENE_KW = (dict(radius=0.3, viewpoint=(1.5, 1.5, 5.0)), dict(radius=0.5))


def scene():
    p = pts(_scene_xyz(21), 21)
    return p, SCENE_KW[0], _every(p, 10), SCENE_KW[1]


def _moved(xyz):
    return xyz @ SCENE_R.T + SCENE_T


def scene_rigid():
    """The scene's own points moved 40 degrees and 1 m (rounded to float32 after the move); the viewpoint moves along."""
    p = pts(_moved(xyz_of(scene()[0]).astype(np.float64)), 21)
    vp = tuple(float(F32(v)) for v in _moved(np.array(SCENE_KW[0]["viewpoint"])))
    return p, dict(SCENE_KW[0], viewpoint=vp), _every(p, 10), SCENE_KW[1]


def scene_resampled():
    """The same surfaces under another jitter seed, cropped to 85 % along x, moved the same way."""
    xyz = _scene_xyz(22)
    xyz = xyz[xyz[:, 0] <= np.quantile(xyz[:, 0], 0.85)]
    p = pts(_moved(xyz), 22)
    vp = tuple(float(F32(v)) for v in _moved(np.array(SCENE_KW[0]["viewpoint"])))
    return p, dict(SCENE_KW[0], viewpoint=vp), _every(p, 8, 3), SCENE_KW[1]


def keypoint_on_point():
    """Every keypoint is a point of the cloud: d2 == 0 meets the clamp of the weight."""
    p, kw = NC.tail_1000()
    return p, kw, _every(p, 9), dict(radius=0.3)


def keypoint_alone():
    """Keypoints 5 m and more away from every point, between keypoints that have neighbours; one no cell accepts."""
    p, kw = NC.tail_1000()
    k = _every(p, 50)
    k[1::3] += F32(5.0)
    k[4] = (1e7, 0.0, 0.0)
    return p, kw, k, dict(radius=0.3)


def neighbours_without_normals():
    """A dense blob and a sparse halo whose points have fewer than min_neighbours neighbours: keypoints in the halo see points without normals."""
    rng = np.random.default_rng(31)
    blob = rng.uniform(-0.3, 0.3, (500, 3))
    halo = rng.uniform(-1.5, 1.5, (250, 3))
    p = pts(np.concatenate([blob, halo]), 31)
    k = np.concatenate([xyz_of(p)[500::5], xyz_of(p)[:500:25]])
    return p, dict(radius=0.15, min_neighbours=6), k, dict(radius=0.4)


def duplicates():
    """Every third point of a random cloud twice more: pairs at d2 == 0 are no pairs, and a duplicate is a neighbour of its twin's neighbours."""
    p, kw = NC.tail_257()
    x = xyz_of(p)
    p2 = pts(np.concatenate([x, x[::3], x[::3]]), 32)
    return p2, kw, _every(p2, 11), dict(radius=0.3)


def normal_along_dp():
    """Two layers of the axis plane 0.5 m apart, normals radius 0.3: every normal is exactly (0, 0, 1) from its own layer, and the point straight above
    or below has dp along the normal, |dp x n1| == 0."""
    g = NC._axis_grid()
    p = pts(np.concatenate([g, g + np.array([0.0, 0.0, 0.5])]), 33)
    return p, dict(radius=0.3), _every(p, 4), dict(radius=0.6)


def dense_cell():
    """More points in one cell than a workgroup has threads (normals_cases.dense_cell), keypoints inside and outside the dense cell."""
    p, kw = NC.dense_cell()
    return p, kw, np.concatenate([_every(p[:600], 60), _every(p[600:], 20)]), dict(radius=0.3)


def invalid_and_span():
    """normals_cases.invalid_and_span: rejected points never count; keypoints beside the out-of-span points and at the lone in-span one."""
    p, kw = NC.invalid_and_span()
    k = np.concatenate([_every(p[:100], 5), np.array([[2047.9, 0.5, 0.5], [5000.0, 0.0, 0.0], [0.5, 0.5, 2100.0]], np.float32)])
    return p, kw, k, dict(radius=1.0)


def far_from_origin():
    """A tilted plane 1500 m away on each axis."""
    p, kw = NC.tilted_plane_far()
    return p, kw, _every(p, 7), dict(radius=0.35)


def m0():
    p, kw = NC.tail_257()
    return p, kw, np.zeros((0, 3), np.float32), dict(radius=0.3)


def m1():
    p, kw = NC.tail_257()
    return p, kw, _every(p, 300), dict(radius=0.3)


def m65():
    p, kw = NC.tail_257()
    return p, kw, _every(p, 4)[:65], dict(radius=0.3)


def radius_differs_from_normals():
    """The sphere with normals at 0.2 m and descriptors at 0.45 m."""
    p, kw = NC.sphere_in()
    return p, kw, _every(p, 12), dict(radius=0.45)


CASES = {f.__name__: f for f in (scene, scene_rigid, scene_resampled, keypoint_on_point, keypoint_alone, neighbours_without_normals, duplicates, normal_along_dp,
                                 dense_cell, invalid_and_span, far_from_origin, m0, m1, m65, radius_differs_from_normals)}
