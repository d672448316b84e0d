"""The statistical outlier removal restated in numpy from the definition, not from the kernels: brute force over all
pairs, no grid, float32 operations spelled out one by one, Python integers for the sums.  The checker of the outlier-filter tests."""
import numpy as np

from tests import voxel_map_ref as VR

POINT_RGB = VR.POINT_RGB
F32 = np.float32
NO_SCORE = 0xFFFFFFFF


def rho_of(cell, max_rings):
    return (F32(max_rings) - F32(0.25)) * F32(cell)                               # float32


def d2_matrix(p, valid):
    """d2[i][j] as the definition computes it, float32; +inf on the diagonal and wherever i or j is not valid."""
    x, y, z = (p[a].astype(np.float32) for a in ("x", "y", "z"))
    with np.errstate(all="ignore"):
        dx = x[None, :] - x[:, None]; dy = y[None, :] - y[:, None]; dz = z[None, :] - z[:, None]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    d2[~valid, :] = np.inf; d2[:, ~valid] = np.inf
    np.fill_diagonal(d2, np.inf)
    return d2


def u_of(d2):
    """(uint64)((double)sqrtf(d2) * 2^32)."""
    return (np.sqrt(d2.astype(np.float32)).astype(np.float64) * 4294967296.0).astype(np.uint64)


def threshold(M, A, Bhi, Blo, mul):
    """mean, sqrt(var), thr in fp64, in the definition's order; M == 0 gives zeros."""
    if M == 0:
        return np.float64(0.0), np.float64(0.0), np.float64(0.0)
    Md = np.float64(M)
    mean = np.float64(A) / Md
    var = np.float64(0.0)
    if M > 1:
        e2 = (np.float64(Bhi) * np.float64(4294967296.0) + np.float64(Blo)) / Md
        var = (e2 - mean * mean) * (Md / np.float64(M - 1))
        if not var > 0.0:
            var = np.float64(0.0)
    sd = np.sqrt(var)
    return mean, sd, mean + np.float64(mul) * sd


class Result:
    pass


def run(p, mean_k=100, stddev_mul=1.0, cell=0.1, max_rings=8):
    """The whole definition over POINT_RGB p.  Result: keep [n] uint8, v [n] uint32, stats [8] int64 (points in, rejected, isolated, M,
    kept, A, Bhi, Blo), mean / sd / thr float64, cloud (the kept points in input order)."""
    n = len(p)
    k = int(mean_k)
    r = Result()
    valid = VR.cell_of(p, cell)[0] if n else np.zeros(0, bool)
    rho = rho_of(cell, max_rings)
    rho2 = rho * rho                                                              # float32
    v = np.full(n, NO_SCORE, np.uint32)
    isolated = 0
    if n:
        d2 = d2_matrix(p, valid)
        inside = (d2 <= rho2).sum(1)
        for i in np.nonzero(valid)[0]:
            if inside[i] < k:
                isolated += 1
                continue
            smallest = np.partition(d2[i], k - 1)[:k]                             # the k smallest values; ties enter by value
            S = sum(int(u) for u in u_of(smallest))
            v[i] = S >> 16
    scored = v != NO_SCORE
    vs = [int(x) for x in v[scored]]
    M = len(vs); A = sum(vs); Bhi = sum(x * x >> 32 for x in vs); Blo = sum(x * x & 0xFFFFFFFF for x in vs)
    r.mean, r.sd, r.thr = threshold(M, A, Bhi, Blo, stddev_mul)
    keep = scored & (v.astype(np.float64) <= r.thr)
    r.keep = keep.astype(np.uint8)
    r.v = v
    r.stats = np.array([n, int((~valid).sum()), isolated, M, int(keep.sum()), A, Bhi, Blo], np.int64)
    r.cloud = p[keep]
    return r


def text(r):
    """What lmono_amd/host/sor_test prints for the same points and parameters."""
    mean, sd, thr = (int(np.array(x, np.float64).view(np.uint64)) for x in (r.mean, r.sd, r.thr))
    lines = ["stats " + " ".join(str(int(s)) for s in r.stats), "threshold %016x %016x %016x" % (mean, sd, thr)]
    lines += ["%d %08x" % (int(kp), int(v)) for kp, v in zip(r.keep, r.v)]
    return "\n".join(lines) + "\n"


def rejected_points(cell=0.1):
    """Points no filter of this cell size accepts: NaN, +-inf, |cell index| >= 2^20."""
    big = np.float32(1048576.0 * cell * 1.01)
    xyz = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0, -big * 2, 0], [0, 0, 3e38], [np.nan, np.nan, np.nan]], np.float32)
    return VR.points(xyz, np.full(len(xyz), 0xFF102030, np.uint32))


def walls(seed,offset=(50.0, -20.0, 0.0)):
    """Two noisy walls at 4 m and 9 m (1400 and 1200 points, sigma 1 cm and 2 cm), 120 uniform "flying" points between them, 30 scattered far
    points; shuffled.  Returns the POINT_RGB cloud and labels [n]: 0 near wall, 1 far wall, 2 flying, 3 far scatter."""
    rng = np.random.default_rng(seed)
    near = np.stack([rng.uniform(-0.8, 0.8, 1400), rng.uniform(-0.5, 0.5, 1400), 4.0 + rng.normal(0.0, 0.01, 1400)], 1)
    far = np.stack([rng.uniform(-1.4, 1.4, 1200), rng.uniform(-0.9, 0.9, 1200), 9.0 + rng.normal(0.0, 0.02, 1200)], 1)
    fly = np.stack([rng.uniform(-0.8, 0.8, 120), rng.uniform(-0.5, 0.5, 120), rng.uniform(4.3, 8.7, 120)], 1)
    scat = rng.uniform(-30.0, 30.0, (30, 3)) + np.array([0.0, 0.0, 60.0])
    xyz = (np.concatenate([near, far, fly, scat]) + np.asarray(offset)).astype(np.float32)
    label = np.concatenate([np.zeros(1400, int), np.ones(1200, int), np.full(120, 2), np.full(30, 3)])
    order = rng.permutation(len(xyz))
    p = VR.points(xyz[order], rng.integers(0, 1 << 32, len(xyz), dtype=np.uint64).astype(np.uint32))
    return p, label[order]
