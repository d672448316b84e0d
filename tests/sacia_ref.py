"""numpy restatement of lmono_amd/csrc/sacia.hpp, the sample-consensus initial alignment on FPFH descriptors: every operation
a single IEEE operation in the header's order, so the device, the host program and this file agree to the byte.  The fit is tests/icp_ref.solve,
the generator tests/pnp_ref.mix."""
import numpy as np

from tests import icp_ref as IR
from tests import pnp_ref as PR

F32, F64, U64 = np.float32, np.float64, np.uint64
MAX_DRAWS = 64
KEY = 0x5ac1a
VOID = np.uint64(0xFFFFFFFFFFFFFFFF)
M32 = np.uint64(0xFFFFFFFF)


def params_ok(min_sample_dist, max_corr, k_corr, n_hyp):
    return 0.0 <= min_sample_dist <= 4096.0 and 0.0 < max_corr <= 16.0 and 1 <= k_corr <= 32 and 1 <= n_hyp <= 65536


def keys(seed, n_hyp):
    h = np.arange(n_hyp, dtype=U64)
    base = PR.mix(PR.mix(U64(seed ^ 0x9e3779b9) & M32) ^ U64(KEY))
    return PR.mix(base ^ h)


def below(r, n):
    return ((r * U64(n)) >> U64(32)).astype(np.int64)


def d2(a, b):
    """sor_d2(a, b) in float32: ((dx dx + dy dy) + dz dz) with d = b - a; broadcasts over the leading axes."""
    with np.errstate(all="ignore"):
        d = (b - a).astype(F32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def desc_d2(a, b):
    """[ns][nt] float32: the 33 terms added in index order from 0."""
    s = np.zeros((len(a), len(b)), F32)
    for k in range(a.shape[1]):
        d = a[:, None, k] - b[None, :, k]
        s = s + d * d
    return s


def candidates(sdesc, tdesc, K):
    """[ns][K] target entries by (distance, index)."""
    D = desc_d2(sdesc, tdesc)
    return np.argsort(D, axis=1, kind="stable")[:, :K].astype(np.int64), D


def sample(seed, n_hyp, u, msd2):
    """-> (idx [n_hyp][3], ok [n_hyp])"""
    ky = keys(seed, n_hyp)
    ns = len(u)
    idx = np.zeros((n_hyp, 3), np.int64)
    have = np.zeros(n_hyp, np.int64)
    for d in range(MAX_DRAWS):
        todo = have < 3
        if not todo.any():
            break
        c = below(PR.mix(ky ^ U64(d)), ns)
        ok = todo.copy()
        for q in range(3):
            e = idx[:, q]
            ok &= ~(q < have) | ((e != c) & (d2(u[e], u[c]) >= msd2))
        rows = np.flatnonzero(ok)
        idx[rows, have[rows]] = c[rows]
        have[rows] += 1
    return idx, have == 3, ky


def fit(u3, w3):
    """icp_terms of three pairs added, icp_solve."""
    iu, iw = IR._fix(u3), IR._fix(w3)
    Su = [int(v) for v in iu.sum(0)]; Sw = [int(v) for v in iw.sum(0)]
    hi, lo = [], []
    for a in range(3):
        for b in range(3):
            P = iu[:, a] * iw[:, b]
            h = P >> 26
            hi.append(int(h.sum())); lo.append(int((P - h * 67108864).sum()))
    return IR.solve(3, Su, Sw, hi, lo)


def transform(R, tau, cs, ct):
    T = np.zeros(12, F64)
    for a in range(3):
        r = R[3 * a:3 * a + 3]
        T[4 * a:4 * a + 3] = r
        T[4 * a + 3] = (F64(ct[a]) + tau[a]) - ((r[0] * F64(cs[0]) + r[1] * F64(cs[1])) + r[2] * F64(cs[2]))
    return T


class Result:
    pass


def run(skp, sdesc, sflag, tkp, tdesc, tflag, min_sample_dist=0.5, max_corr=1.0, k_corr=10, n_hyp=1024, seed=1):
    """None when a side has fewer than 3 usable keypoints or one out of span (LMONO_EINVAL)."""
    assert params_ok(min_sample_dist, max_corr, k_corr, n_hyp)
    sl, tl = np.flatnonzero(np.asarray(sflag) == 1), np.flatnonzero(np.asarray(tflag) == 1)
    if len(sl) < 3 or len(tl) < 3:
        return None
    sp, tp = np.asarray(skp, F32)[sl], np.asarray(tkp, F32)[tl]
    cs, ct = sp[0], tp[0]
    u, w = sp - cs, tp - ct
    if not (IR._in_span(u).all() and IR._in_span(w).all()):
        return None
    ns, nt = len(sl), len(tl)
    K = min(k_corr, nt)
    cand, D = candidates(np.asarray(sdesc, F32)[sl], np.asarray(tdesc, F32)[tl], K)
    msd2, mc2 = F32(min_sample_dist) * F32(min_sample_dist), F32(max_corr) * F32(max_corr)
    idx, ok, ky = sample(seed, n_hyp, u, msd2)
    part = np.stack([below(PR.mix(ky ^ U64(MAX_DRAWS + e)), K) for e in range(3)], 1)
    tj = cand[idx, part]                                                    # [n_hyp][3] target entries
    r = Result()
    r.sl, r.tl, r.cand, r.D, r.idx, r.tj, r.valid = sl, tl, cand, D, idx, tj, ok
    r.err = np.full(n_hyp, VOID, U64); r.inl = np.zeros(n_hyp, np.uint32)
    r.fits = {}
    cache = {}
    for h in np.flatnonzero(ok):
        k = (tuple(idx[h]), tuple(tj[h]))
        if k not in cache:
            R, tau = fit(u[idx[h]], w[tj[h]])
            q = IR._q(R, tau, ct, u)
            best = d2(q[:, None, :], tp[None, :, :]).min(1)
            cache[k] = (R, tau, U64(((np.where(best <= mc2, best, mc2).astype(F64) * 16777216.0).astype(U64)).sum()), np.uint32((best <= mc2).sum()))
        R, tau, r.err[h], r.inl[h] = cache[k]
        r.fits[int(h)] = (R, tau)
    r.voids = int((~ok).sum())
    r.ok = int(ok.any())
    r.h = int(np.flatnonzero(ok)[np.argmin(r.err[ok])]) if r.ok else -1        # argmin: the first of the least
    r.T = transform(*r.fits[r.h], cs, ct) if r.ok else None
    r.cs, r.ct = cs, ct
    r.stats = np.array([r.ok, r.h, int(r.err[r.h]) if r.ok else 0, int(r.inl[r.h]) if r.ok else 0, r.voids, ns, nt, n_hyp], np.int64)
    return r


def transform_of(r, h):
    return transform(*r.fits[h], r.cs, r.ct)


def text(r):
    """The lines lmono_amd/host/sacia_test prints."""
    out = ["stats " + " ".join(str(int(v)) for v in r.stats)]
    out.append("T " + (" ".join("%016x" % v for v in r.T.view(np.uint64)) if r.ok else "none"))
    out += ["%d %d" % (int(e), int(i)) for e, i in zip(r.err, r.inl)]
    return out


def pose_error(T, R_true, t_true):
    """(rotation error in degrees, translation error in m) of a 3 x 4 transform."""
    T = np.asarray(T, F64).reshape(3, 4)
    dR = T[:, :3] @ np.asarray(R_true).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.sqrt(((T[:, 3] - np.asarray(t_true)) ** 2).sum()))
