"""Plain 50-digit references of the marginalisation numerics (lmono_amd/csrc/marg.hip), written from the formulas in that file's header and from
nothing in this project's device code:
    prior_dx           the parameterisation of Marginalization::Evaluate: translation difference, then 2 vec(q0^-1 (x) q), negated when the scalar
                       part is negative, q0^-1 = conj(q0) / |q0|^2 (quaternions are x, y, z, w)
    evaluate           r + J dx
    second_new         MARGIN_SECOND_NEW: r = r0 + J0 dx, H = J0^T J0, b = J0^T r, dropped block first, H_mm symmetrised, its 6x6 pseudo-inverse with
                       the 1e-8 cut (mp.eigsy), Schur complement -> H', b'
    cut_products       sum over eigenvalues > 1e-8 of lambda v v^T and of v v^T b': what lin_J^T lin_J and lin_J^T lin_r must equal (n <= 30: mp.eigsy
                       takes ~1 s there and ~10 s at n = 60)
    marginalize_dense  MARGIN_OLD: H, b over [pose0, depths, ex, pose1..10] assembled in numpy from the factor functions of oracle/ba_numpy.py (their
                       accuracy on the device has its own tests), then the dense pseudo-inverse of H_mm with the cut and the Schur complement in mp
Inputs are fp64 arrays and enter exactly; everything after that is 50 digits."""
import mpmath
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
EPS = mpf(1e-8)        # the cut, the very double the kernels compare with


def M(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mpf(float(v)) for v in row] for row in a]) if a.ndim == 2 else mp.matrix([mpf(float(v)) for v in a])


def to_np(m):
    a = np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    return a[:, 0] if m.cols == 1 else a


def maxabs(m):
    return max([abs(v) for v in m] + [mpf(0)])


def prior_dx(x0, x):
    x0 = np.asarray(x0, np.float64).reshape(-1, 7); x = np.asarray(x, np.float64).reshape(-1, 7)
    out = mp.matrix(6 * len(x), 1)
    for k in range(len(x)):
        a0 = [mpf(float(v)) for v in x0[k]]; a = [mpf(float(v)) for v in x[k]]
        for c in range(3):
            out[6 * k + c] = a[c] - a0[c]
        n2 = a0[3] ** 2 + a0[4] ** 2 + a0[5] ** 2 + a0[6] ** 2
        ix, iy, iz, iw = -a0[3] / n2, -a0[4] / n2, -a0[5] / n2, a0[6] / n2
        qx, qy, qz, qw = a[3:]
        rw = iw * qw - ix * qx - iy * qy - iz * qz
        rv = [iw * qx + ix * qw + iy * qz - iz * qy, iw * qy + iy * qw + iz * qx - ix * qz, iw * qz + iz * qw + ix * qy - iy * qx]
        s = 1 if rw >= 0 else -1
        for c in range(3):
            out[6 * k + 3 + c] = 2 * s * rv[c]
    return out


def evaluate(J, r, x0, x):
    return M(r) + M(J) * prior_dx(x0, x)


def pinv_cut(A):
    """Pseudo-inverse of the symmetric mp matrix A keeping eigenvalues > 1e-8; also the eigenvalues."""
    E, Q = mp.eigsy(A)
    n = A.rows
    out = mp.matrix(n, n)
    for k in range(n):
        if E[k] > EPS:
            v = Q[:, k]
            out += v * v.T / E[k]
    return out, [E[k] for k in range(n)]


def schur(H, b, m):
    """H' = H_rr - H_rm H_mm^+ H_mr, b' = b_r - H_rm H_mm^+ b_m with the first m rows / columns eliminated (H_mm symmetrised); + H_mm's eigenvalues."""
    Hmm = (H[:m, :m] + H[:m, :m].T) / 2
    Hinv, E = pinv_cut(Hmm)
    T = H[m:, :m] * Hinv
    return H[m:, m:] - T * H[:m, m:], b[m:] - T * b[:m], E


def second_new(J0, r0, x0, x, drop):
    J0 = np.asarray(J0, np.float64); nb = J0.shape[0] // 6
    Jm = M(J0)
    r = M(r0) + Jm * prior_dx(x0, x)
    perm = [6 * drop + c for c in range(6)] + [6 * k + c for k in range(nb) if k != drop for c in range(6)]
    Jp = mp.matrix(6 * nb, 6 * nb)
    for i in range(6 * nb):
        for j in range(6 * nb):
            Jp[i, j] = Jm[i, perm[j]]
    Hp, bp, _ = schur(Jp.T * Jp, Jp.T * r, 6)
    return Hp, bp


def cut_products(Hp, bp):
    assert Hp.rows <= 30, "mp.eigsy is too slow for a test above n = 30"
    E, Q = mp.eigsy((Hp + Hp.T) / 2)
    n = Hp.rows
    Hc = mp.matrix(n, n); bc = mp.matrix(n, 1)
    for k in range(n):
        if E[k] > EPS:
            v = Q[:, k]
            Hc += E[k] * (v * v.T)
            bc += v * (v.T * bp)[0]
    return Hc, bc, [E[k] for k in range(n)]


def assemble_dense(win):
    """(H, b, m) of MARGIN_OLD in fp64 numpy over [pose0, depths, ex, pose1..10] from a window dict as Context.marginalize takes it."""
    from oracle import ba_numpy as B
    F0 = len(win["invd"]); m = 6 + F0; pos = m + 66
    H = np.zeros((pos, pos)); b = np.zeros(pos)
    idx_pose = lambda i: 0 if i == 0 else m + 6 + 6 * (i - 1)

    def add(blocks, res):
        for (ia, Ja) in blocks:
            for (ib, Jb) in blocks:
                H[ia:ia + Ja.shape[1], ib:ib + Jb.shape[1]] += Ja.T @ Jb
            b[ia:ia + Ja.shape[1]] += Ja.T @ res
    c = np.asarray(win["laser01"], np.float64); poses = np.asarray(win["poses"], np.float64); ex = np.asarray(win["ex"], np.float64)
    rr, Ji, Jj = B.laser_factor(poses[0], poses[1], c[:9].reshape(3, 3), c[9:18].reshape(3, 3), c[18:21], c[21:24], np.asarray(win["laser_info"], np.float64))
    add([(idx_pose(0), Ji[:, :6]), (idx_pose(1), Jj[:, :6])], rr)
    pts = np.asarray(win["pts"], np.float64).reshape(-1, 4)
    for o in range(len(win["obs_j"])):
        f, j = int(win["obs_feat"][o]), int(win["obs_j"][o])
        rr, Jx, Ja, Jb_, Jd = B.mono_projection_factor(ex, poses[0], poses[j], win["invd"][f], pts[o, :2], pts[o, 2:], np.asarray(win["mono_info"], np.float64))
        rc, Js = B.corrector(rr, [Jx, Ja, Jb_, Jd.reshape(2, 1)], B.cauchy(rr @ rr))
        add([(m, Js[0][:, :6]), (idx_pose(0), Js[1][:, :6]), (idx_pose(j), Js[2][:, :6]), (6 + f, Js[3])], rc)
    return H, b, m


def marginalize_dense(win):
    """(H', b', eigenvalues of H_mm) in mp; 6 + F0 <= 30 keeps the mp eigen step of H_mm affordable."""
    H, b, m = assemble_dense(win)
    assert m <= 30
    return schur(M(H), M(b), m)


def marginalize_dense_np(win, cut=True):
    """The same in fp64 numpy for any F0 (numpy.linalg.eigh): (H', b') with the eps cut applied to H' when `cut`; + H_mm's smallest eigenvalue."""
    H, b, m = assemble_dense(win)
    Hmm = 0.5 * (H[:m, :m] + H[:m, :m].T)
    wv, V = np.linalg.eigh(Hmm)
    Hinv = V @ np.diag(np.where(wv > 1e-8, 1.0 / np.where(wv > 1e-8, wv, 1), 0)) @ V.T
    Hp = H[m:, m:] - H[m:, :m] @ Hinv @ H[:m, m:]
    bp = b[m:] - H[m:, :m] @ Hinv @ b[:m]
    if cut:
        wv2, V2 = np.linalg.eigh(0.5 * (Hp + Hp.T))
        keep = wv2 > 1e-8
        Hp, bp = (V2[:, keep] * wv2[keep]) @ V2[:, keep].T, V2[:, keep] @ (V2[:, keep].T @ bp)
    return Hp, bp, wv.min()
