"""The point-to-point ICP of the map builder restated in numpy from the definition, not from the kernels: brute force over
all pairs, no grid, float32 operations spelled out one by one, Python integers for the sums, the solve in fp64 one operation at a time.
The checker of the aligner tests."""
import numpy as np

from tests import voxel_map_ref as VR

POINT_RGB = VR.POINT_RGB
F32 = np.float32
F64 = np.float64
SWEEPS = 8
SPAN = F32(2048.0)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def default_cell(max_corr):
    """The smallest float32 h >= D / 1.75 with (2 - 0.25) h >= D in float32: D / 1.75 alone misses by an ulp for about one D in twenty."""
    D = F32(max_corr)
    h = D / F32(1.75)
    for _ in range(4):
        if (F32(2) - F32(0.25)) * h >= D:
            break
        h = np.nextafter(h, F32(np.inf))
    return h


def params_ok(max_corr, max_iter, eps, mse_eps, cell, max_rings):
    D, h = F32(max_corr), F32(cell)
    with np.errstate(all="ignore"):
        if not (D > 0 and D <= F32(16.0)) or max_iter < 1 or max_iter > 65536 or not eps >= 0.0 or not mse_eps >= 0.0:
            return False
        if not h > 0 or not F32(1.0) / h > 0 or max_rings < 1 or max_rings > 64:
            return False
        return bool((F32(max_rings) - F32(0.25)) * h >= D)


def _ord(x):
    """The order of min / max for the origin: the float order with -0 below +0, as unsigned integers."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> np.uint64(31) != 0, b ^ np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def _unord(k):
    k = int(k)
    b = (k & 0x7FFFFFFF) if k & 0x80000000 else (k ^ 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def _xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def _in_span(c):
    with np.errstate(all="ignore"):
        return ((c > -SPAN) & (c < SPAN)).all(1)


def _fix(c):
    """(int64)((double)c * 65536.0), truncated."""
    return (c.astype(np.float64) * 65536.0).astype(np.int64)


def jacobi(A, sweeps):
    """Cyclic Jacobi on a symmetric matrix given as a list of lists of np.float64 (modified in place) -> V (columns = eigenvectors).  Fixed sweep
    count, fixed (p, q) order, a rotation is skipped iff a_pq == 0; theta may overflow to inf, t is then 0, as on the device."""
    n = len(A)
    V = [[F64(1.0) if i == j else F64(0.0) for j in range(n)] for i in range(n)]
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[p][q]
                    if apq == 0.0:
                        continue
                    app, aqq = A[p][p], A[q][q]
                    theta = (aqq - app) / (F64(2.0) * apq)
                    t = F64(1.0) / (np.abs(theta) + np.sqrt(theta * theta + F64(1.0)))
                    if theta < 0.0:
                        t = -t
                    c = F64(1.0) / np.sqrt(t * t + F64(1.0))
                    s = t * c
                    for k in range(n):
                        if k == p or k == q:
                            continue
                        akp, akq = A[k][p], A[k][q]
                        n1 = c * akp - s * akq; n2 = s * akp + c * akq
                        A[k][p] = n1; A[p][k] = n1; A[k][q] = n2; A[q][k] = n2
                    A[p][p] = app - t * apq; A[q][q] = aqq + t * apq
                    A[p][q] = F64(0.0); A[q][p] = F64(0.0)
                    for k in range(n):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq
    return V


def solve(N, Su, Sw, hi, lo, info=None):
    """R' [9] and tau' [3] (np.float64) from the exact sums, N >= 3."""
    n = F64(N)
    ub = [F64(v) / n for v in Su]
    wb = [F64(v) / n for v in Sw]
    S = [[(F64(hi[3 * a + b]) * F64(67108864.0) + F64(lo[3 * a + b])) - F64(Su[a]) * wb[b] for b in range(3)] for a in range(3)]
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    A = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (-Sxx + Syy) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (-Sxx - Syy) + Szz]]
    V = jacobi(A, SWEEPS)
    if info is not None:
        info["offdiag"] = max(info.get("offdiag", 0.0), max(abs(float(A[i][k])) for i in range(4) for k in range(4) if i != k))
    b = 0
    for i in range(1, 4):
        if A[i][i] > A[b][b]:
            b = i
    w, x, y, z = V[0][b], V[1][b], V[2][b], V[3][b]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    two, one = F64(2.0), F64(1.0)
    R = [one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
         two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
         two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]
    tau = [(wb[a] - ((R[3 * a] * ub[0] + R[3 * a + 1] * ub[1]) + R[3 * a + 2] * ub[2])) / F64(65536.0) for a in range(3)]
    return np.array(R, np.float64), np.array(tau, np.float64)


def _guess(G, xyz):
    """p0 = (float)(G p): fp64 products and sums in a fixed order, one cast."""
    x, y, z = (xyz[:, a].astype(np.float64) for a in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(((G[4 * a] * x + G[4 * a + 1] * y) + G[4 * a + 2] * z) + G[4 * a + 3]).astype(np.float32) for a in range(3)], 1)


def _q(R, tau, o, u):
    """q = (float)((double)o + (R (double)u + tau))."""
    ux, uy, uz = (u[:, a].astype(np.float64) for a in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(F64(o[a]) + (((R[3 * a] * ux + R[3 * a + 1] * uy) + R[3 * a + 2] * uz) + tau[a])).astype(np.float32) for a in range(3)], 1)


class Result:
    pass


def run(target, source, max_corr=0.5, max_iter=50, eps=1e-8, mse_eps=0.0, cell=None, max_rings=2, guess=None):
    """cell and max_rings enter through the validity test alone (a point is valid iff its cell index at 1 / cell is within +-2^20)."""
    D = F32(max_corr)
    h = default_cell(D) if cell is None else F32(cell)
    assert params_ok(D, max_iter, eps, mse_eps, h, max_rings)
    D2 = D * D
    G = IDENTITY.copy() if guess is None else np.asarray(guess, np.float64).reshape(12)
    r = Result()
    info = {}
    # target
    m = _xyz(target)
    valid = VR.cell_of(target, h)[0]
    o = np.zeros(3, np.float32)
    if valid.any():
        for a in range(3):
            k = _ord(m[valid, a])
            o[a] = (_unord(k.min()) + _unord(k.max())) * F32(0.5)
    with np.errstate(all="ignore"):
        w = m - o[None, :]
    t_ok = valid & _in_span(w)
    mt, wt = m[t_ok], w[t_ok]
    order = np.lexsort((mt[:, 2], mt[:, 1], mt[:, 0]))          # by x, then y, then z: the first minimum below is the definition's tie-break
    mt, wt = mt[order], wt[order]
    iw = _fix(wt)
    # source
    p0 = _guess(G, _xyz(source))
    with np.errstate(all="ignore"):
        u = p0 - o[None, :]
    usable = _in_span(u)
    iu = _fix(np.where(usable[:, None], u, F32(0.0)))
    ns = len(source)
    R = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], np.float64)
    tau = np.zeros(3, np.float64)
    k, status, done, mse_prev, N, E = 0, 3, ns == 0, F64(0.0), 0, 0
    hist = []
    d2_last = np.full(ns, np.inf, np.float32)
    while not done:
        k += 1
        q = _q(R, tau, o, u)
        qp = np.zeros(ns, POINT_RGB); qp["x"] = q[:, 0]; qp["y"] = q[:, 1]; qp["z"] = q[:, 2]
        cand = usable & VR.cell_of(qp, h)[0]
        d2_last = np.full(ns, np.inf, np.float32)
        best = np.zeros(ns, np.int64)
        if len(mt) and cand.any():
            with np.errstate(all="ignore"):
                dx = mt[None, :, 0] - q[cand, None, 0]; dy = mt[None, :, 1] - q[cand, None, 1]; dz = mt[None, :, 2] - q[cand, None, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            j = d2.argmin(1)                                     # the first of equal minima: the smallest (x, y, z)
            dmin = d2[np.arange(len(j)), j]
            ok = dmin <= D2
            idx = np.flatnonzero(cand)
            d2_last[idx[ok]] = dmin[ok]
            best[idx[ok]] = j[ok]
        acc = np.isfinite(d2_last)
        a_iu = iu[acc].astype(object); a_iw = iw[best[acc]].astype(object)
        N = int(acc.sum())
        Su = [int(sum(a_iu[:, a])) for a in range(3)]
        Sw = [int(sum(a_iw[:, a])) for a in range(3)]
        hi, lo = [], []
        for a in range(3):
            for b in range(3):
                P = a_iu[:, a] * a_iw[:, b]
                ph = [int(v) >> 26 for v in P]
                hi.append(sum(ph)); lo.append(sum(int(v) - (h_ << 26) for v, h_ in zip(P, ph)))
        E = sum(int(v) for v in (d2_last[acc].astype(np.float64) * 16777216.0).astype(np.uint64))
        hist.append((N, E))
        if N < 3:
            status, done = 3, True
            break
        R1, tau1 = solve(N, Su, Sw, hi, lo, info)
        dt = F64(0.0)
        for a in range(3):
            d = tau1[a] - tau[a]; dt = dt + d * d
        dR = F64(0.0)
        for e in range(9):
            d = R1[e] - R[e]; dR = dR + d * d
        R, tau = R1, tau1
        mse = F64(E) / F64(N) / F64(16777216.0)
        if dt < eps and dR < eps:
            status, done = 0, True
        elif mse_eps > 0 and k >= 2 and abs(mse - mse_prev) < mse_eps:
            status, done = 2, True
        elif k == max_iter:
            status, done = 1, True
        mse_prev = mse
    # results
    T = np.zeros(12, np.float64)
    od = o.astype(np.float64)
    for a in range(3):
        ra = R[3 * a:3 * a + 3]
        t = (od[a] + tau[a]) - ((ra[0] * od[0] + ra[1] * od[1]) + ra[2] * od[2])
        for b in range(3):
            T[4 * a + b] = (ra[0] * G[b] + ra[1] * G[4 + b]) + ra[2] * G[8 + b]
        T[4 * a + 3] = ((ra[0] * G[3] + ra[1] * G[7]) + ra[2] * G[11]) + t
    q = _q(R, tau, o, u)
    cloud = np.array(source, POINT_RGB)
    cloud["x"] = q[:, 0]; cloud["y"] = q[:, 1]; cloud["z"] = q[:, 2]
    r.transform = T
    r.cloud = cloud
    r.d2 = d2_last
    r.history = np.array(hist, np.int64).reshape(-1, 2)
    r.stats = np.array([ns, int((~usable).sum()), len(target), int((~t_ok).sum()), k, status, N if k else 0, E if k else 0], np.int64)
    r.iterations, r.status, r.N, r.origin, r.R, r.tau = k, status, (N if k else 0), o, R, tau
    r.offdiag = info.get("offdiag", 0.0)
    return r


def canon(a):
    """The bytes of a float32 array with every NaN replaced by one pattern: a NaN's sign and payload are not part of the definition."""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def cloud_bytes(c):
    return canon(_xyz(c)) + np.ascontiguousarray(c["bgra"]).tobytes()


def text(r):
    """What host/icp_test prints for this result, without its offdiag line; NaNs as 7fc00000."""
    def f32(v):
        v = np.array(v, np.float32); v[np.isnan(v)] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
        return v.view(np.uint32)
    out = ["transform " + " ".join("%016x" % v for v in r.transform.view(np.uint64)), "stats " + " ".join(str(int(v)) for v in r.stats),
           "history %d" % len(r.history)] + ["%d %d" % (n, e) for n, e in r.history.tolist()]
    xyz = f32(_xyz(r.cloud)); d2 = f32(r.d2)
    out += ["%08x %08x %08x %08x" % (d2[i], xyz[i, 0], xyz[i, 1], xyz[i, 2]) for i in range(len(d2))]
    return out
