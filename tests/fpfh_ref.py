"""The FPFH descriptors of the map builder restated in numpy from the definition, not from the kernels: brute force over all
pairs, no grid, float32 and float64 operations spelled out one by one, integer sums as Python / numpy integers.  The checker of the FPFH tests."""
import numpy as np

from tests import icp_ref as IR
from tests import voxel_map_ref as VR

F32 = np.float32
F64 = np.float64
U64 = np.uint64
BINS, DIM = 11, 33
MAX_RADIUS = F32(4.0)
MAX_KEYPOINTS = 4096
MIN_D2 = F32(2.0 ** -20)
ONE = F64(2.0 ** 40)
# (cos, sin) of -pi + 2 pi k / 11 for k = 1 .. 5, the literals of fpfh.hpp
EDGES = [(-0.8412535328311811, -0.5406408174555978), (-0.4154150130018863, -0.9096319953545184), (0.14231483827328512, -0.9898214418809327),
         (0.6548607339452851, -0.7557495743542583), (0.9594929736144975, -0.2817325568414295)]

default_cell = IR.default_cell
canon = IR.canon


def params_ok(radius, cell, max_rings):
    r, h = F32(radius), F32(cell)
    with np.errstate(all="ignore"):
        if not (r > 0 and r <= MAX_RADIUS):
            return False
        if not h > 0 or not F32(1.0) / h > 0 or not F32(1.0) / h <= F32(3.0e38) or max_rings < 1 or max_rings > 64:
            return False
        return bool((F32(max_rings) - F32(0.25)) * h >= r)


def value_bin(f):
    """floor((f + 1) * 5.5) clamped to 0 .. 10, on a float64 array."""
    t = (f + F64(1.0)) * F64(5.5)
    return np.where(t >= 10.0, 10, np.where(t >= 1.0, np.floor(np.clip(t, 0.0, 11.0)), 0)).astype(np.int64)


def angle_bin(x, y):
    """The bin of the direction (x, y) (float64 arrays) by comparisons against the edge directions: fpfh_angle_bin."""
    x = np.asarray(x, F64); y = np.asarray(y, F64)
    neg = np.zeros(x.shape, np.int64); pos = np.full(x.shape, 5, np.int64)
    for c, s in EDGES:
        neg += (F64(c) * y - F64(s) * x >= 0.0)
        pos += (F64(c) * y + F64(s) * x >= 0.0)
    return np.where((x == 0.0) & (y == 0.0), 5, np.where(y < 0.0, neg, pos))


def pair_bins(pi, ni, pj, nj):
    """[k][3] float32 arrays of k pairs -> (ok [k] bool, bins [k][3] int64: angle, f2, f3).  fpfh_pair, one operation at a time."""
    pi, ni, pj, nj = (np.asarray(a, np.float32).astype(F64) for a in (pi, ni, pj, nj))
    with np.errstate(all="ignore"):
        d = pj - pi
        f4 = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        a1 = ((ni[:, 0] * d[:, 0] + ni[:, 1] * d[:, 1]) + ni[:, 2] * d[:, 2]) / f4
        a2 = ((nj[:, 0] * d[:, 0] + nj[:, 1] * d[:, 1]) + nj[:, 2] * d[:, 2]) / f4
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[:, None], nj, ni); n2 = np.where(swap[:, None], ni, nj)
        d = np.where(swap[:, None], -d, d)
        f3 = np.where(swap, -a2, a1)
        v0 = d[:, 1] * n1[:, 2] - d[:, 2] * n1[:, 1]; v1 = d[:, 2] * n1[:, 0] - d[:, 0] * n1[:, 2]; v2 = d[:, 0] * n1[:, 1] - d[:, 1] * n1[:, 0]
        vn = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
        ok = vn != 0.0
        u0 = n1[:, 1] * v2 - n1[:, 2] * v1; u1 = n1[:, 2] * v0 - n1[:, 0] * v2; u2 = n1[:, 0] * v1 - n1[:, 1] * v0
        f2 = ((v0 * n2[:, 0] + v1 * n2[:, 1]) + v2 * n2[:, 2]) / vn
        x = (n1[:, 0] * n2[:, 0] + n1[:, 1] * n2[:, 1]) + n1[:, 2] * n2[:, 2]
        y = ((u0 * n2[:, 0] + u1 * n2[:, 1]) + u2 * n2[:, 2]) / vn
        safe = lambda a: np.where(ok, a, 0.0)
        bins = np.stack([angle_bin(safe(x), safe(y)), value_bin(safe(f2)), value_bin(safe(f3))], 1)
    return ok, bins


def weight(d2, nj):
    """(uint64)(2^40 / ((double)max(d2, 2^-20) * (double)nj)): float32 d2 [k], nj [k] > 0."""
    c = np.where(d2 < MIN_D2, MIN_D2, d2).astype(np.float32)
    return (ONE / (c.astype(F64) * nj.astype(F64))).astype(U64)


def _d2(a, b):
    """sor_d2 of every row of a [p][3] to every row of b [q][3], float32: dx = b - a."""
    with np.errstate(all="ignore"):
        dx = b[None, :, 0] - a[:, None, 0]; dy = b[None, :, 1] - a[:, None, 1]; dz = b[None, :, 2] - a[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


class Result:
    pass


def run(points, records, keypoints, radius=0.05, cell=None, max_rings=2):
    """points: POINT_RGB [n]; records: [n][4] float32 (normals_ref's records, NaN: no normal); keypoints: [m][3] float32, finite.  cell and
    max_rings enter through the validity tests alone.  -> Result with desc [m][33] float32, counts [m] uint32, flags [m] uint32, stats [8]
    int64; also spfh [n][34] int64 (rows of points that are not needed are zero), needed [n] bool, has [n] bool, near [m][n] bool."""
    r = F32(radius)
    h = default_cell(r) if cell is None else F32(cell)
    assert params_ok(r, h, max_rings)
    r2 = r * r
    n = len(points)
    kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 3)
    m = len(kp)
    assert m <= MAX_KEYPOINTS and np.isfinite(kp).all()
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 4)
    assert len(rec) == n
    xyz = IR._xyz(points) if n else np.zeros((0, 3), np.float32)
    valid = VR.cell_of(points, h)[0] if n else np.zeros(0, bool)
    o = np.zeros(3, np.float32)
    if valid.any():
        for a in range(3):
            k = IR._ord(xyz[valid, a])
            o[a] = (IR._unord(k.min()) + IR._unord(k.max())) * F32(0.5)
    with np.errstate(all="ignore"):
        ok = valid & IR._in_span(xyz - o[None, :]) if n else valid
    has = ok & ~np.isnan(rec[:, 0])
    usable = VR.cell_of(VR.points(kp, np.zeros(m, np.uint32)), h)[0] if m else np.zeros(0, bool)
    res = Result()
    res.has, res.origin = has, o
    res.near = (_d2(kp, xyz) <= r2) & has[None, :] & usable[:, None] if m and n else np.zeros((m, n), bool)
    res.needed = res.near.any(0)
    res.spfh = np.zeros((n, DIM + 1), np.int64)
    res.skipped = 0                                                     # pairs skipped for |dp x n1| == 0
    idx = np.flatnonzero(res.needed)
    cand = np.flatnonzero(has)
    if len(idx):
        d2 = _d2(xyz[idx], xyz[cand])
        ii, jj = np.nonzero((d2 > 0) & (d2 <= r2))
        i, j = idx[ii], cand[jj]
        good, bins = pair_bins(xyz[i], rec[i, :3], xyz[j], rec[j, :3])
        res.skipped = int((~good).sum())
        i, bins = i[good], bins[good]
        for f in range(3):
            np.add.at(res.spfh, (i, BINS * f + bins[:, f]), 1)
        np.add.at(res.spfh, (i, DIM), 1)
    res.desc = np.zeros((m, DIM), np.float32)
    res.counts = np.zeros(m, np.uint32)
    pairs = res.spfh[:, DIM]
    dk = _d2(kp, xyz) if m and n else np.zeros((m, n), np.float32)
    for k in range(m):
        rows = np.flatnonzero(res.near[k] & (pairs > 0))
        res.counts[k] = len(rows)
        if not len(rows):
            continue
        W = weight(dk[k, rows], pairs[rows])
        P = W[:, None] * res.spfh[rows, :DIM].astype(U64)               # <= 2^60: exact in uint64
        assert (P.astype(object) == W.astype(object)[:, None] * res.spfh[rows, :DIM].astype(object)).all()
        hi = [int(x) for x in (P >> U64(32)).astype(object).sum(0)]
        lo = [int(x) for x in (P & U64(0xFFFFFFFF)).astype(object).sum(0)]
        v = np.array([F64(np.uint64(a)) * F64(4294967296.0) + F64(np.uint64(b)) for a, b in zip(hi, lo)], F64)
        for f in range(3):
            t = v[BINS * f]
            for b in range(1, BINS):
                t = t + v[BINS * f + b]
            res.desc[k, BINS * f:BINS * (f + 1)] = ((v[BINS * f:BINS * (f + 1)] * F64(100.0)) / t).astype(np.float32)
    res.flags = (res.counts > 0).astype(np.uint32)
    c = res.counts.astype(np.int64)
    np_ = pairs[res.needed]
    res.stats = np.array([m, int((c > 0).sum()), int((c == 0).sum()), int(res.needed.sum()), int(np_.sum()), int(np_.max(initial=0)), int(c.sum()), int(c.max(initial=0))], np.int64)
    return res


def text(r):
    """What host/fpfh_test prints for this result."""
    b = np.ascontiguousarray(r.desc, np.float32).view(np.uint32)
    return ["stats " + " ".join(str(int(x)) for x in r.stats)] + [" ".join("%08x" % w for w in b[k]) + " %d %d" % (r.counts[k], r.flags[k]) for k in range(len(b))]
