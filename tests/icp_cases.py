"""The cases of the aligner tests: name -> (target, source, keyword arguments of icp_ref.run / CloudAligner).  Shared by the CPU
test (restatement against host/icp_test) and the GPU test (device against the restatement)."""
import numpy as np

from tests import voxel_map_ref as VR

F32 = np.float32


def pts(xyz, seed=0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return VR.points(xyz, np.random.default_rng(seed).integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))


def rotation(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.sqrt((a * a).sum())
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def corner():
    """A corner of three planes on a 0.25 m grid with unequal extents: 218 points, fp64, at the origin."""
    g = 0.25
    out = [(i * g, j * g, 0.0) for i in range(10) for j in range(9)]
    out += [(i * g, 0.0, k * g) for i in range(10) for k in range(1, 9)]
    out += [(0.0, j * g, k * g) for j in range(1, 9) for k in range(1, 7)]
    out = np.array(out, np.float64)
    assert len(out) == 218
    return out


AXIS = (0.3, -0.5, 0.8)


def physical(at, deg=1.0, shift=(0.03, -0.02, 0.04), drop=False):
    """-> target, source, truth: the source is the target turned by `deg` about AXIS through `at` and shifted; truth[i] is the target point that
    source point i belongs to (its own row where the point is an added outlier)."""
    c = corner()
    at = np.asarray(at, np.float64)
    tgt = pts(c + at, 1)
    moved = c @ rotation(AXIS, deg).T + np.asarray(shift) + at
    truth = c + at
    if drop:
        keep = np.arange(len(c)) % 3 != 2
        far = np.random.default_rng(7).uniform(-1.0, 1.0, (20, 3)) + np.array([5.0, 5.0, 5.0]) + at + np.array([2.25, 2.0, 2.0])
        moved = np.concatenate([moved[keep], far]); truth = np.concatenate([truth[keep], far])
    return tgt, pts(moved, 2), truth.astype(np.float32)


def blob(n, seed, span=1.0, at=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return rng.uniform(-span, span, (n, 3)) + np.asarray(at)


def moved_blob(n, seed, at=(0.0, 0.0, 0.0), deg=2.0, shift=(0.02, 0.01, -0.03), span=1.5):
    t = blob(n, seed, span)
    return pts(t + np.asarray(at), seed), pts(t @ rotation((0.1, 0.9, -0.3), deg).T + np.asarray(shift) + np.asarray(at), seed + 1)


def d_bound():
    """Dyadic coordinates, so that u and q of the first iteration are exact: pair 0 lies at d2 == D2 exactly, pair 1 at the next float32 above."""
    s = np.array([[1, 1, 1], [3, 1, 1], [1, 3, 1], [3, 3, 2], [2, 2, 3]], np.float32)
    t = s + np.array([[0.5, 0, 0], [0.5, 1.5 * 2.0 ** -13, 0], [0, 0.25, 0], [0, 0, 0.125], [0.25, 0, 0]], np.float32)
    return pts(t, 3), pts(s, 4), dict(max_corr=0.5, max_iter=1)


def ties():
    """Three source points, each with two targets mirrored about it on one axis (x, y, z in turn), and two plain pairs."""
    s = np.array([[2, 2, 2], [6, 2, 2], [2, 6, 2], [6, 6, 3], [4, 4, 4]], np.float32)
    t = np.array([[2.25, 2, 2], [1.75, 2, 2], [6, 2.25, 2], [6, 1.75, 2], [2, 6, 2.25], [2, 6, 1.75], [6, 6.125, 3], [4.125, 4, 4]], np.float32)
    return pts(t, 5), pts(s, 6), dict(max_corr=0.5, max_iter=3)


def stopping(r, at):
    """The sets of the outlier filter's stopping test at k = 1: the candidate in ring r is farther than a point in ring r + 1.  max_corr = 0.7 lies above
    the farthest candidate (3.5 h sqrt(3) = 0.61 on the diagonals at r = 3) and below rho = 7.75 h."""
    from tests.test_sor_gpu import DIRECTIONS, H, _stopping_set
    src, tgt = [], []
    for n, d in enumerate(DIRECTIONS):
        s = _stopping_set(r, d, 1) + 40.0 * float(H) * n * np.array([1.0, 0.0, 0.0])
        src.append(s[:1]); tgt.append(s[1:])
    at = np.asarray(at)
    return pts(np.concatenate(tgt) + at, r), pts(np.concatenate(src) + at, r + 10), dict(max_corr=0.7, max_iter=2, cell=float(H), max_rings=8)


def invalid():
    """NaN, inf, a cell index outside +-2^20 and a point 2048 m or more from the origin, in the source and in the target, among good pairs."""
    tgt, src = moved_blob(60, 11, at=(10.0, 20.0, -5.0), deg=1.0)
    nonfinite = [[np.nan, 1, 1], [1, np.inf, 1], [-np.inf, np.nan, 3], [3.0e7, 0, 0]]
    # the target's two extremes in x lie 4100 m apart about the cloud: the origin stays at the cloud and both are 2050 m from it
    bad_t = np.array(nonfinite + [[-2040.0, 20.0, -5.0], [2060.0, 20.0, -5.0]], np.float32)
    bad_s = np.array(nonfinite + [[10.0, 20.0, 2100.0], [-2040.0, 20.0, -5.0]], np.float32)
    return np.concatenate([tgt[:30], pts(bad_t, 12), tgt[30:]]), np.concatenate([src[:10], pts(bad_s, 13), src[10:]]), dict(max_corr=0.5)


def q_rejected():
    """A usable source point whose q the cell function rejects.  D = 0.01 gives a default cell of about 0.0057 m, so the cell index passes 2^20 at
    about 5991.9 m: the target lies just inside that limit, the last source point 3 m beyond it in x, well within the 2048 m span of the origin."""
    t = blob(40, 21, 0.2, (5990.0, 1.0, 2.0))
    s = np.concatenate([t + np.array([0.002, 0.0, 0.0]), [[5993.0, 1.0, 2.0]]])
    return pts(t, 21), pts(s, 22), dict(max_corr=0.01)


def _three(collinear):
    s = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]] if collinear else [[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float64)
    return pts(s + np.array([10.0, 10.0, 10.0]), 8), pts(s @ rotation((0, 0, 1), 2.0).T + np.array([10.03, 10.02, 9.99]), 9), dict(max_corr=0.5)


CASES = {
    "phys_origin": lambda: physical((0.0, 0.0, 0.0))[:2] + (dict(),),
    "phys_far": lambda: physical((6000.0, -6000.0, 300.0))[:2] + (dict(),),
    "phys3_origin": lambda: physical((0.0, 0.0, 0.0), 3.0, (0.11, -0.06, 0.08), True)[:2] + (dict(),),
    "phys2_far": lambda: physical((6000.0, -6000.0, 300.0), 2.0, (-0.07, 0.11, 0.05), True)[:2] + (dict(),),
    "n_src0": lambda: (moved_blob(50, 1)[0], pts(np.zeros((0, 3))), dict()),
    "n_tgt0": lambda: (pts(np.zeros((0, 3))), moved_blob(50, 1)[1], dict()),
    "all_beyond": lambda: (pts(blob(40, 2)), pts(blob(30, 3, at=(9.0, 0.0, 0.0))), dict()),
    "two_pairs": lambda: (pts([[0, 0, 0], [1, 0, 0], [0, 9, 0]]), pts([[0.1, 0, 0], [1.1, 0, 0], [5, 5, 5]]), dict()),
    "three_pairs": lambda: _three(False),
    "three_collinear": lambda: _three(True),
    "max_iter1": lambda: moved_blob(300, 4) + (dict(max_iter=1),),
    "eps0": lambda: moved_blob(300, 4) + (dict(eps=0.0, max_iter=6),),
    "mse1": lambda: moved_blob(300, 4) + (dict(mse_eps=1.0),),
    "d_bound": d_bound,
    "ties": ties,
    "same_target_40": lambda: (np.concatenate([pts([[3.21, -4.5, 0.77]] * 40, 1), moved_blob(20, 5)[0]]), np.concatenate([pts([[3.3, -4.4, 0.7]], 2), moved_blob(20, 5)[1]]), dict()),
    "dense_cell": lambda: (np.concatenate([pts(blob(700, 6, 0.1, (0.14, 0.14, 0.14)), 6), moved_blob(300, 7)[0]]), np.concatenate([pts(blob(90, 8, 0.12, (0.14, 0.14, 0.14)), 8), moved_blob(300, 7)[1]]),
                           dict()),
    "invalid": invalid,
    "q_rejected": q_rejected,
    "guess": lambda: moved_blob(400, 9, at=(30.0, -8.0, 2.0), deg=20.0, shift=(1.0, -2.0, 0.5)) + (dict(guess=guess_for(9)),),
    "far_2000": lambda: moved_blob(2000, 10, at=(-41.3, -77.7, -3.1), span=4.0) + (dict(),),
}
for _r in (1, 2, 3):
    for _k, _at in enumerate([(0.0, 0.0, 0.0), (6000.0, -6000.0, 300.0), (-41.3, -77.7, -3.1)]):
        CASES["stopping_r%d_at%d" % (_r, _k)] = (lambda r=_r, at=_at: stopping(r, at))


def guess_for(seed):
    """An approximate inverse of the motion of the `guess` case (off by 1 degree and a few centimetres), row-major 3 x 4."""
    at = np.array([30.0, -8.0, 2.0])
    Rm = rotation((0.1, 0.9, -0.3), 19.0)
    t = np.array([0.97, -2.02, 0.52])
    Ri = Rm.T                                                   # x = Ri (y - at - t) + at
    return np.concatenate([Ri, (at - Ri @ (at + t))[:, None]], 1).reshape(12)
