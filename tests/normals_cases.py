"""The cases of the surface-normal tests: name -> (points, keyword arguments of normals_ref.run / SurfaceNormals).  Shared by the
CPU test (restatement against host/normals_test, and what each case claims to be) and the GPU test (device against the restatement).  Every case
has at most about 2000 points."""
import numpy as np

from tests import icp_cases as IC

F32 = np.float32
pts = IC.pts
PLANE_NORMAL = np.array([0.3, -0.5, 0.8]) / np.sqrt(0.3 * 0.3 + 0.5 * 0.5 + 0.8 * 0.8)
SPHERE_CENTRE = np.array([2.0, -1.0, 3.0])


def _line(n, step=0.1):
    return pts([(step * i, 0.0, 0.0) for i in range(n)], 3)


def one():
    return pts([(1.0, 2.0, 3.0)], 1), dict(radius=0.5)


def two():
    return _line(2), dict(radius=0.5)


def three():
    """Exactly min_neighbours points, not collinear: the smallest neighbourhood that gets a normal."""
    return pts([(0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.0, 0.1, 0.05)], 2), dict(radius=0.5)


def three_collinear():
    return _line(3), dict(radius=0.5)


def four_min5():
    return pts([(0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, 0.0, 0.1)], 4), dict(radius=0.5, min_neighbours=5)


def all_duplicates():
    return pts([(0.3, -0.7, 2.5)] * 40, 5), dict(radius=0.05)


def _axis_grid():
    return np.array([(0.25 * (i - 4), 0.25 * (j - 4), 8.0) for i in range(9) for j in range(9)], np.float64)


def axis_plane_interior():
    """Rows of _axis_grid whose whole disc of radius 0.5 lies inside the grid."""
    return np.array([2 <= i <= 6 and 2 <= j <= 6 for i in range(9) for j in range(9)])


def axis_plane():
    """9 x 9 points at multiples of 0.25 in z = 8, r = 0.5: every coordinate, offset and sum is exact; the neighbours two steps away along an axis
    lie at exactly d2 == r * r."""
    return pts(_axis_grid(), 6), dict(radius=0.5)


def viewpoint_on_plane():
    """The same plane seen from a point in it: dot == 0 exactly for every point, so the canonical sign decides."""
    return pts(_axis_grid(), 6), dict(radius=0.5, viewpoint=(5.0, 5.0, 8.0))


def _tilted(at):
    n = PLANE_NORMAL
    e1 = np.cross(n, [0.0, 0.0, 1.0]); e1 /= np.sqrt((e1 * e1).sum())
    e2 = np.cross(n, e1)
    g = np.array([(0.1 * (i - 15)) * e1 + (0.1 * (j - 15)) * e2 for i in range(31) for j in range(31)])
    return pts(g + np.asarray(at, np.float64), 7)


def tilted_plane():
    """31 x 31 points at 0.1 m on the plane with normal (0.3, -0.5, 0.8) / |.| through the origin."""
    return _tilted((0.0, 0.0, 0.0)), dict(radius=0.25)


def tilted_plane_far():
    """The same plane 1500 m away on each axis: float32 (2^-13 m there) is coarser than the 2^-16 m fixed point."""
    return _tilted((1500.0, 1500.0, 1500.0)), dict(radius=0.25)


def _sphere(n=1500):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return pts(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1) + SPHERE_CENTRE, 8)


def sphere_in():
    """1500 points on the unit sphere about SPHERE_CENTRE, seen from the centre: the normals point inward."""
    return _sphere(), dict(radius=0.2, viewpoint=tuple(SPHERE_CENTRE))


def sphere_out():
    """Seen from outside: the near side's normals point outward, the far side's inward."""
    return _sphere(), dict(radius=0.2, viewpoint=(10.0, 10.0, 10.0))


def dense_cell():
    """600 points inside one cell of the default grid for r = 0.3 (h = 0.1714...: [0, h)^3) and 400 sparse ones around it: more points in a cell than
    a workgroup has threads."""
    rng = np.random.default_rng(9)
    return pts(np.concatenate([rng.uniform(0.01, 0.16, (600, 3)), rng.uniform(-1.5, 1.5, (400, 3))]), 9), dict(radius=0.3)


RING_EDGE_CELL, RING_EDGE_RINGS = 0.2, 2


def ring_edge_radius():
    return (F32(RING_EDGE_RINGS) - F32(0.25)) * F32(RING_EDGE_CELL)          # sor_rho(R, h): the largest radius this grid may serve


def ring_edge():
    """r = sor_rho(2, 0.2) exactly.  Around centres near the low and the high faces of their cells, points just inside r, at r and just outside
    it in 26 directions: the accepted ones reach the far side of the outermost ring."""
    r = float(ring_edge_radius())
    dirs = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
    dirs /= np.sqrt((dirs * dirs).sum(1))[:, None]
    out = []
    for c in [(0.001, 0.001, 0.001), (0.199, 0.199, 0.199), (0.001, 0.199, 0.1), (3.001, -2.001, 0.199), (-5.199, 7.1, -0.001), (10.0, 10.0, 10.0)]:
        c = np.asarray(c)
        out += [c[None, :], c + dirs * (r * (1 - 2e-6)), c + dirs * r, c + dirs * (r * (1 + 2e-6)), c + dirs * (r * 0.5)]
    return pts(np.concatenate(out), 10), dict(radius=r, cell=RING_EDGE_CELL, max_rings=RING_EDGE_RINGS)


def cell_boundary():
    """Points at exact multiples of the cell h = 0.25 on both sides of 0, and points an ulp or so off such multiples."""
    grid = np.array([(0.25 * i, 0.25 * j, 0.25 * k) for i in range(-4, 5) for j in range(-4, 5) for k in range(-1, 2)], np.float32)
    rng = np.random.default_rng(11)
    near = (0.25 * rng.integers(-4, 5, (150, 3))).astype(np.float32)
    near = np.where(rng.integers(0, 2, near.shape) == 1, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf)))
    return pts(np.concatenate([grid, near]), 11), dict(radius=0.4, cell=0.25, max_rings=2)


def invalid_and_span():
    """300 good points within 2 m of 0; NaN and inf points; points no cell accepts; pairs at -5000 / +5000 on x and -2100 / +2100 on z, which put the origin
    at 0 on those axes and are themselves out of span; one at exactly 2048 m on x (out) and one just inside (in, alone)."""
    rng = np.random.default_rng(12)
    good = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1e7, 0, 0], [0, -3e38, 0],
                    [-5000.0, 0, 0], [5000.0, 0, 0], [2048.0, 0.5, 0.5], [np.nextafter(F32(2048.0), F32(0.0)), 0.5, 0.5], [0.5, 0.5, -2100.0], [0.5, 0.5, 2100.0]], np.float32)
    xyz = np.concatenate([good[:100], bad[:6], good[100:200], bad[6:], good[200:]])
    return pts(xyz, 12), dict(radius=0.5)


def tail_257():
    return pts(np.random.default_rng(13).uniform(0.0, 1.0, (257, 3)) + np.array([4.0, -9.0, 1.0]), 13), dict(radius=0.3)


def tail_1000():
    return pts(np.random.default_rng(14).uniform(-0.8, 0.8, (1000, 3)) + np.array([-30.0, 12.0, 2.0]), 14), dict(radius=0.3, viewpoint=(-30.0, 12.0, 50.0))


CASES = {f.__name__: f for f in (one, two, three, three_collinear, four_min5, all_duplicates, axis_plane, viewpoint_on_plane, tilted_plane, tilted_plane_far,
                                 sphere_in, sphere_out, dense_cell, ring_edge, cell_boundary, invalid_and_span, tail_257, tail_1000)}
