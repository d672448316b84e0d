"""The surface normals of the map builder restated in numpy from the definition, not from the kernels: brute force over all
pairs, no grid, float32 operations spelled out one by one, integer sums, the solve in fp64 one operation at a time (the Jacobi sweeps are
icp_ref.jacobi, the restatement of rej_jacobi).  The checker of the normals tests."""
import numpy as np

from tests import icp_ref as IR
from tests import voxel_map_ref as VR

POINT_RGB = VR.POINT_RGB
F32 = np.float32
F64 = np.float64
SWEEPS = 8
MAX_RADIUS = F32(4.0)
NAN_BITS = 0x7FC00000
NORMAL = np.dtype([("nx", np.float32), ("ny", np.float32), ("nz", np.float32), ("curvature", np.float32)])

default_cell = IR.default_cell


def params_ok(radius, min_neighbours, cell, max_rings):
    r, h = F32(radius), F32(cell)
    with np.errstate(all="ignore"):
        if not (r > 0 and r <= MAX_RADIUS) or min_neighbours < 3:
            return False
        if not h > 0 or not F32(1.0) / h > 0 or not F32(1.0) / h <= F32(3.0e38) or max_rings < 1 or max_rings > 64:
            return False
        return bool((F32(max_rings) - F32(0.25)) * h >= r)


def solve(N, S, SS, p, vp, info=None):
    """The record [nx, ny, nz, curvature] (np.float32) of the point p (three np.float32) from its exact sums (Python integers; SS: xx, xy, xz,
    yy, yz, zz), N >= min_neighbours; vp: three np.float32 or None."""
    n = F64(N)
    s = [F64(v) for v in S]
    ss = [F64(v) for v in SS]
    c01 = ss[1] - (s[0] * s[1]) / n; c02 = ss[2] - (s[0] * s[2]) / n; c12 = ss[4] - (s[1] * s[2]) / n
    A = [[ss[0] - (s[0] * s[0]) / n, c01, c02],
         [c01, ss[3] - (s[1] * s[1]) / n, c12],
         [c02, c12, ss[5] - (s[2] * s[2]) / n]]
    V = IR.jacobi(A, SWEEPS)
    if info is not None:
        info["offdiag"] = max(info.get("offdiag", 0.0), max(abs(float(A[i][k])) for i in range(3) for k in range(3) if i != k))
    b = 0
    for i in range(1, 3):
        if A[i][i] < A[b][b]:
            b = i
    v = [V[0][b], V[1][b], V[2][b]]
    nrm = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    v = [x / nrm for x in v]
    lam = A[b][b] if A[b][b] > 0.0 else F64(0.0)
    tr = (A[0][0] + A[1][1]) + A[2][2]
    curv = lam / tr if tr > 0.0 else F64(0.0)
    dot = F64(0.0)
    if vp is not None:
        dot = ((F64(vp[0]) - F64(p[0])) * v[0] + (F64(vp[1]) - F64(p[1])) * v[1]) + (F64(vp[2]) - F64(p[2])) * v[2]
    flip = bool(dot < 0.0)
    if dot == 0.0:
        big, ab = v[0], np.abs(v[0])
        for x in v[1:]:
            if np.abs(x) > ab:
                big, ab = x, np.abs(x)
        flip = bool(big < 0.0)
    if flip:
        v = [-x for x in v]
    return np.array([F32(x + F64(0.0)) for x in v] + [F32(curv)], np.float32)


class Result:
    pass


def run(points, radius=0.05, min_neighbours=3, cell=None, max_rings=2, viewpoint=None):
    """cell and max_rings enter through the validity test alone (a point is valid iff its cell index at 1 / cell is within +-2^20).
    -> Result with records [n][4] float32, counts [n] uint32, stats [8] int64; also neighbours [n][n] bool, origin, offdiag."""
    r = F32(radius)
    h = default_cell(r) if cell is None else F32(cell)
    assert params_ok(r, min_neighbours, h, max_rings)
    r2 = r * r
    vp = None if viewpoint is None else np.asarray(viewpoint, np.float32).reshape(3)
    n = len(points)
    xyz = IR._xyz(points) if n else np.zeros((0, 3), np.float32)
    valid = VR.cell_of(points, h)[0] if n else np.zeros(0, bool)
    o = np.zeros(3, np.float32)
    if valid.any():
        for a in range(3):
            k = IR._ord(xyz[valid, a])
            o[a] = (IR._unord(k.min()) + IR._unord(k.max())) * F32(0.5)
    with np.errstate(all="ignore"):
        w = xyz - o[None, :]
    ok = valid & IR._in_span(w) if n else valid
    iw = IR._fix(np.where(ok[:, None], w, F32(0.0)))
    res = Result()
    res.records = np.full((n, 4), np.array([NAN_BITS], np.uint32).view(np.float32)[0], np.float32)
    res.counts = np.zeros(n, np.uint32)
    res.neighbours = np.zeros((n, n), bool)
    info = {}
    idx = np.flatnonzero(ok)
    if len(idx):
        q = xyz[idx]
        with np.errstate(all="ignore"):
            dx = q[None, :, 0] - q[:, None, 0]; dy = q[None, :, 1] - q[:, None, 1]; dz = q[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        near = d2 <= r2
        res.neighbours[np.ix_(idx, idx)] = near
        iq = iw[idx]
        for t, i in enumerate(idx):
            d = iq[near[t]] - iq[t][None, :]                      # int64; |d| < 2^19 and fewer than 2^25 rows: no int64 sum below can overflow
            N = len(d)
            assert N >= 1 and np.abs(d).max(initial=0) < (1 << 19) and N < (1 << 25)
            res.counts[i] = N
            if N < min_neighbours:
                continue
            S = [int(d[:, a].sum()) for a in range(3)]
            SS = [int((d[:, a] * d[:, b]).sum()) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            res.records[i] = solve(N, S, SS, xyz[i], vp, info)
    c = res.counts.astype(np.int64)
    res.stats = np.array([n, int((~ok).sum()), int((c >= min_neighbours).sum()), int((ok & (c < min_neighbours)).sum()), int(c.sum()), int(c.max(initial=0)), 0, 0], np.int64)
    res.origin, res.ok, res.offdiag = o, ok, info.get("offdiag", 0.0)
    return res


def canon(a):
    """The bytes of a float32 array with every NaN replaced by one pattern: a NaN's sign and payload are not part of the definition."""
    return IR.canon(a)


def records_of(rec):
    """A NORMAL record array (what SurfaceNormals.read gives) as [n][4] float32."""
    rec = np.ascontiguousarray(rec, NORMAL)
    return rec.view(np.float32).reshape(-1, 4)


def text(r):
    """What host/normals_test prints for this result, without its offdiag line; NaNs as 7fc00000."""
    v = np.array(r.records, np.float32)
    v[np.isnan(v)] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    b = v.view(np.uint32)
    return ["stats " + " ".join(str(int(x)) for x in r.stats)] + ["%08x %08x %08x %08x %d" % (b[i, 0], b[i, 1], b[i, 2], b[i, 3], r.counts[i]) for i in range(len(b))]
