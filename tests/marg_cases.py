"""Generators of the marginalisation test cases (tests/test_marg_ref_cpu.py validates them on the CPU, tests/test_marg_gpu.py runs them on the device).

Group A  constructed spectra for lmono_marg_second_new.  x = x0 (dx = 0); J0 holds a well-conditioned 6x6 block D_m in rows 0..5 x the dropped block's
         columns and S in rows 6.. x the kept columns, nothing else: H_mm = D_m^T D_m, H_mr = 0, so H' = S^T S and b' = S^T r_S EXACTLY.  S = Lambda^1/2 Q^T
         with Q a product of Householder reflectors rounded to fp64; the reference is formed at 50 digits from the rounded S, so Q's rounding is immaterial.
         `keep` lists the rows of S whose eigenvalue survives the 1e-8 cut; the expected products are S[keep]^T S[keep] and S[keep]^T r_S[keep] (rows of a
         rounded S are orthogonal to ~1e-16 sqrt(l_i l_j), so the cut eigenspace is the span of the other rows to ~1e-21; the CPU test proves that with
         mp.eigsy at n = 30).  Cases marked ref = "mp" use marg_ref.second_new + cut_products in full.
Group B  dx branches on a real prior (oracle.marginalize(make_window(seed))): flipped quaternions, x0 quaternions of norm 2 and 0.5, ~170 / 190 degree turns.
Group C  window shapes for lmono_marginalize derived from make_window selections.

Branch of marg.hip -> case that reaches it
  marg_eig_ql scale == 0 / h == 0 rows      A diag_n60, A diag_n6 (every row), A blockdiag (rows 30..59 mid-reduction), A singular_drop has none
  l == 0 (last Householder step)            every case (i = 1)
  m == l on first look                      A diag_*, A repeat_identity, A repeat_clusters, A tiny_all (after the fix below)
  zero_r underflow recovery + list shift    A tiny_tridiag: ql_trace() shows x == 0 at step i = 0 of the block l = 0, m = 2 with one rotation listed
  n < 66 with leading dimension n           A size_nb{2..11}_drop* (n = 6 .. 60), A diag_n6
  the 64 + lane halves (n > 64)             every C case (n = 66), B evaluate
  two rotation lists in flight              every case with a dense spectrum (A graded, A size_*, C *): consecutive sweeps alternate the two lists
  eps cut: D                                C noobs (D = 0 for the empty track, status bit 0)
  eps cut: S_A via pinv6                    A singular_drop (H_mm = 0, status bit 0)
  eps cut: eigenvalues of H', lin_J, lin_r  A rank_k{1,6,n-1}, A gap_n30 / gap_n60, A blockdiag, A tiny_all
  factor pass, 3 waves of 64 tracks         C f0_63 / 64 / 65 / 128 / 129 / 160
  while (todo) with several frames          C stagger (three frames in round 0 of wave 0), C gaps, C len1
  nmax versus no, F0 = 0, empty mid-batch   C len1 (1 and 10 observations in a wave), C f0_0, C batch5 = (40, 0, 65, 1, 129)
  W_d assigned, one observation per frame   refused by lmono_marginalize (test_marg_argument_checks: the same frame twice in a track)
  dx: !(rw >= 0), / n2, several windows     B flip, B turn190; B scale2, B scale05; B evaluate (5 windows, 5 different x)
  k_marg_second_new permutation             A size_nb*_drop{0, nb // 2, nb - 1}

Errors against the 50-digit reference, max over a group's cases of err / (n 2^-52 scale)   [scale: max|H'|, max|b'| + 1, max|r| + 1]; device = MI355X
  group                                   oracle H'   device H'   oracle b'   device b'   oracle r   device r
  A second_new, constructed (n 6..60)       2.74        1.15        60.7        6.0
  B second_new on a real prior (n 24)       1.46        0.133       10.8        18.6
  B marg_evaluate, 5 windows                                                                1.22       1.22
  C marginalize, F0 1..13 (50 digits)       5.01        4.69        151         26
  C f0_0 (exact H' = 0: all rounding)       6.6e-9 abs  2.0e-8 abs  1.4e4       2.0e4
  C F0 >= 40 against fp64 numpy (relative)              7.3e-14                 1.1e-12    (bound 1e-7, the existing tests' bound)
(worst single cases: A b' gap_n60 for the oracle, A b' graded for the device; B b' scale2; C b' gaps.)  With F0 = 0 the LASERFactor alone leaves
H' = H_rr - G^T S_A^+ G = 0 exactly; max|H'| of the reference is 3.5e-9, so the unit is meaningless there and the absolute errors are listed.
The bound of every comparison is 8 max(err_oracle, n 2^-52 scale) with err_oracle measured on the same case (bound()); the products J^T J and J^T r are
formed in fp64 numpy for both sides, which adds at most n 2^-53 scale to either error and sits inside the floor term.

Kernel fix found by A tiny_all: with H' ~ 1e-170 the first step of a QL sweep squared a sub-diagonal element of ~1e-170, x = f^2 + g^2 underflowed to 0,
the underflow branch left everything as it was, and after 60 such sweeps status bit 1 was set.  marg_eig_ql now treats |e| < 1e-150 as negligible."""
import numpy as np

from tests import ba_cases as K
from tests import marg_ref as R

EPS = 1e-8


def bound(err_oracle, n, scale):
    return 8.0 * max(err_oracle, n * 2.0 ** -52 * scale)


# ---- group A ----------------------------------------------------------------------------------------------------------------------------------------
def _Q(n, rng, k=4):
    Q = np.eye(n)
    for _ in range(k):
        v = rng.normal(size=n)
        Q = Q - 2.0 * np.outer(v, v @ Q) / (v @ v)
    return Q


def _poses(nb, rng):
    return np.stack([K.rand_pose(rng) for _ in range(nb)])


def _case(name, S, rng, nb, drop, keep=None, ref="rows", Dm=None, status=0):
    n = 6 * nb - 6
    assert S.shape == (n, n)
    if Dm is None:
        Dm = _Q(6, rng, 3) * rng.uniform(1.0, 2.0, 6)[:, None]
    J0 = np.zeros((6 * nb, 6 * nb))
    kp = np.array([6 * k + c for k in range(nb) if k != drop for c in range(6)], int)
    J0[:6, 6 * drop:6 * drop + 6] = Dm
    J0[6:, kp] = S
    r0 = rng.normal(size=6 * nb)
    x0 = _poses(nb, rng)
    return dict(name=name, nb=nb, drop=drop, n=n, J0=J0, r0=r0, x0=x0, x=x0.copy(), S=S, rs=r0[6:].copy(),
                keep=np.arange(n) if keep is None else np.asarray(keep, int), ref=ref, status=status)


def _spectrum(lam, rng):
    lam = np.asarray(lam, np.float64)
    return np.sqrt(lam)[:, None] * _Q(len(lam), rng).T


def tiny_tridiag_block():
    """3x3 lower-bidiagonal block whose S^T S has d = (1e-140, 1e-140, 1e-134), e = (2e-150, 4e-150): the sweep of l = 0, m = 2 gets s ~ 4e-16 in its
    first step and f = s e_0 ~ 8e-166, g ~ e_1 e_0 / d_2 ~ 8e-166 in the second, whose squares underflow."""
    a = c = 1e-70; e = 1e-67
    return np.array([[a, 0, 0], [2e-150 / c, c, 0], [0, 4e-150 / e, e]])


def ql_trace(d, e, tiny=1e-150):
    """The scalar recurrence of an implicit QL sweep (Numerical Recipes' tqli with r^2 = f^2 + g^2 formed directly, as marg_eig_ql does) on the tridiagonal
    (d, e[i] = T[i][i + 1]): the list of (l, m, i) at which f^2 + g^2 == 0 was met.  Host-side check of a generator's condition only."""
    d = np.array(d, np.float64); n = len(d); e = np.concatenate([np.array(e, np.float64), [0.0]])
    hits = []
    for l in range(n):
        for it in range(61):
            m = l
            while m < n - 1 and not (abs(e[m]) <= 2.220446049250313e-16 * (abs(d[m]) + abs(d[m + 1])) or abs(e[m]) < tiny):
                m += 1
            if m == l:
                break
            g = (d[l + 1] - d[l]) / (2.0 * e[l]); r = np.sqrt(g * g + 1.0)
            g = d[m] - d[l] + e[l] / (g + (r if g >= 0 else -r))
            s = c = 1.0; p = 0.0; zero = False
            for i in range(m - 1, l - 1, -1):
                f = s * e[i]; b = c * e[i]
                x = f * f + g * g
                if x == 0.0:
                    d[i + 1] -= p; e[m] = 0.0; e[i + 1] = 0.0; hits.append((l, m, i)); zero = True
                    break
                r = np.sqrt(x); e[i + 1] = r; s = f / r; c = g / r
                g = d[i + 1] - p; r = (d[i] - g) * s + 2.0 * c * b; p = s * r; d[i + 1] = g + p; g = c * r - b
            if not zero:
                d[l] -= p; e[l] = g; e[m] = 0.0
        else:
            hits.append((l, -1, -1))      # the 60-sweep cap
    return hits


def group_a():
    rng = np.random.default_rng(4101)
    out = []
    n = 60
    out.append(_case("diag_n60", np.diag(rng.uniform(0.5, 3.0, n)), rng, 11, 10))
    out.append(_case("diag_n6", np.diag(rng.uniform(0.5, 3.0, 6)), rng, 2, 1))
    out.append(_case("tridiag", np.diag(rng.uniform(1.0, 2.0, n)) + np.diag(rng.uniform(-0.5, 0.5, n - 1), 1), rng, 11, 10))
    S = np.zeros((n, n)); S[:30, :30] = _spectrum(rng.uniform(0.5, 4.0, 30), rng)
    out.append(_case("blockdiag", S, rng, 11, 10, keep=np.arange(30)))
    out.append(_case("repeat_identity", _spectrum(np.ones(n), rng), rng, 11, 10))
    out.append(_case("repeat_clusters", _spectrum(np.repeat([1.0, 2.0, 3.0], 20), rng), rng, 11, 10))
    out.append(_case("graded", _spectrum(10.0 ** (-4 + 10 * np.arange(n) / (n - 1)), rng), rng, 11, 10))
    for k in (1, 6, n - 1):
        lam = rng.uniform(0.2, 1.0, n); lam[rng.permutation(n)[:k]] = 0.0
        out.append(_case("rank_k%d" % k, _spectrum(lam, rng), rng, 11, 5, keep=np.nonzero(lam)[0]))
    for nn, nb in ((30, 6), (60, 11)):
        lam = rng.uniform(0.1, 1.0, nn); lam[0] = 1.0; pm = rng.permutation(nn)
        lam[pm[:3]] = 1e-11; lam[pm[3:6]] = 1e-5
        out.append(_case("gap_n%d" % nn, _spectrum(lam, rng), rng, nb, nb // 2, keep=np.nonzero(lam > 1e-8)[0]))
    out.append(_case("tiny_all", rng.uniform(-1, 1, (n, n)) * 1e-85, rng, 11, 10, keep=[]))
    S = np.eye(12); S[:3, :3] = tiny_tridiag_block()
    out.append(_case("tiny_tridiag", S, rng, 3, 2, keep=np.arange(3, 12)))
    for nb in range(2, 12):
        nn = 6 * nb - 6
        for drop in sorted({0, nb // 2, nb - 1}):
            S = _Q(nn, rng) @ _spectrum(rng.uniform(0.5, 3.0, nn), rng)      # dense, rows not orthogonal; eigenvalues of S^T S in [0.5, 3]
            out.append(_case("size_nb%d_drop%d" % (nb, drop), S, rng, nb, drop, ref="mp" if nb <= 6 else "rows"))
    out.append(_case("singular_drop", _spectrum(rng.uniform(0.5, 2.0, n), rng), rng, 11, 4, Dm=np.zeros((6, 6)), status=1))
    return out


def _gram(S, rs):
    """S^T S and S^T rs at 50 digits from the fp64 entries, rounded to fp64 once at the end."""
    rows = [i for i in range(S.shape[0]) if np.any(S[i] != 0.0)]
    n = S.shape[1]
    cols = [[R.mpf(float(S[i, j])) for i in rows] for j in range(n)]
    rv = [R.mpf(float(rs[i])) for i in rows]
    H = np.zeros((n, n)); b = np.zeros(n)
    nzc = [j for j in range(n) if any(v != 0 for v in cols[j])]
    for a in nzc:
        b[a] = float(R.mp.fdot(cols[a], rv))
        for c in nzc:
            if c >= a:
                H[a, c] = H[c, a] = float(R.mp.fdot(cols[a], cols[c]))
    return H, b


def expected_a(case):
    """(H_exp, b_exp) as fp64 roundings of the 50-digit products, + the mp eigenvalues where the full mp path ran (else None)."""
    if case["ref"] == "mp":
        Hp, bp = R.second_new(case["J0"], case["r0"], case["x0"], case["x"], case["drop"])
        Hc, bc, E = R.cut_products(Hp, bp)
        return R.to_np(Hc), R.to_np(bc), np.array([float(v) for v in E])
    k = case["keep"]
    H, b = _gram(case["S"][k], case["rs"][k])
    return H, b, None


def products(J, r):
    return J.T @ J, J.T @ r


def err_products(J, r, H_exp, b_exp):
    H, b = products(np.asarray(J), np.asarray(r))
    return np.abs(H - H_exp).max(), np.abs(b - b_exp).max()


# ---- group B ----------------------------------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


B_VARIANTS = ("flip", "scale2", "scale05", "turn170", "turn190")


def dx_variants(x0, seed):
    """{name: (x0', x)}: the prior's linearisation point (its quaternions possibly rescaled) and a current state for each dx branch."""
    from oracle import ba_numpy as B
    rng = np.random.default_rng(seed)
    near = np.stack([B.pose_plus(x0[k], rng.normal(0, 2e-3, 6)) for k in range(len(x0))])
    out = {}
    x = near.copy(); x[::2, 3:] *= -1.0                     # the same rotations, every other quaternion negated
    out["flip"] = (x0.copy(), x)
    for name, s in (("scale2", 2.0), ("scale05", 0.5)):
        y0 = x0.copy(); y0[:, 3:] *= s
        out[name] = (y0, near.copy())
    for name, deg in (("turn170", 170.0), ("turn190", 190.0)):
        x = near.copy()
        for k in range(len(x)):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            h = np.deg2rad(deg + rng.uniform(-2, 2)) / 2
            x[k, 3:] = _qmul(near[k, 3:], np.concatenate([ax * np.sin(h), [np.cos(h)]]))
        out[name] = (x0.copy(), x)
    return out


def real_prior(oracle, seed=7):
    w = K.make_window(seed)
    J0, r0, m, x0, _ = oracle.marginalize(w)
    return J0, r0, x0


def shrink_prior(oracle, J, r, x0, nb_target):
    """Drop trailing blocks with the oracle at x = x0 until nb_target blocks are left."""
    while len(x0) > nb_target:
        J, r = oracle.marg_second_new(J, r, x0, x0, len(x0) - 1)
        x0 = x0[:-1]
    return J, r, x0


# ---- group C ----------------------------------------------------------------------------------------------------------------------------------------
def base_window(oracle, seed=5):
    w = K.make_window(seed)
    _, _, _, _, sel = oracle.marginalize(w)
    tracks = []
    for f in range(len(sel["invd"])):
        o = np.nonzero(sel["obs_feat"] == f)[0]
        tracks.append(dict(invd=float(sel["invd"][f]), j=sel["obs_j"][o].astype(int), pts=sel["pts"][o].copy()))
    return w, tracks


def window_from(w, tracks, laser_info=None):
    of, oj, pts = [], [], []
    for g, t in enumerate(tracks):
        for k in range(len(t["j"])):
            of.append(g); oj.append(int(t["j"][k])); pts.append(t["pts"][k])
    return dict(poses=np.ascontiguousarray(w["poses"], np.float64), ex=np.ascontiguousarray(w["ex"], np.float64),
                invd=np.array([t["invd"] for t in tracks], np.float64), obs_feat=np.array(of, np.int32), obs_j=np.array(oj, np.int32),
                pts=np.array(pts, np.float64).reshape(-1, 4), laser01=np.ascontiguousarray(w["laser_consts"][0], np.float64),
                laser_info=np.ascontiguousarray(w["laser_info"] if laser_info is None else laser_info, np.float64),
                mono_info=np.ascontiguousarray(w["mono_info"], np.float64))


def replicate(tracks, F0, rng):
    """F0 tracks: the given ones over and over with slightly different depths and points (as test_marginalize_150_tracks_anchored_at_frame_0 does)."""
    out = []
    rep = 0
    while len(out) < F0:
        for t in tracks:
            if len(out) == F0:
                break
            out.append(dict(invd=t["invd"] * (1 + 0.01 * rep), j=t["j"].copy(), pts=t["pts"] + rng.normal(0, 1e-4 * rep, t["pts"].shape)))
        rep += 1
    return out


def round_frames(win, wave=0):
    """[set of frames of the it-th observations of the tracks 64 wave .. 64 wave + 63] for it = 0, 1, ..: what one `while (todo)` loop walks through."""
    rounds = []
    F0 = len(win["invd"])
    per = [win["obs_j"][win["obs_feat"] == f] for f in range(64 * wave, min(F0, 64 * wave + 64))]
    for it in range(max([len(p) for p in per] + [0])):
        rounds.append(set(int(p[it]) for p in per if len(p) > it))
    return rounds


F0_SIZES = (0, 1, 63, 64, 65, 128, 129, 160)
BATCH5 = (40, 0, 65, 1, 129)


def group_c(oracle):
    """{name: window}.  Windows with 6 + F0 <= 30 are compared with the 50-digit Schur complement, the others with the oracle / numpy."""
    w, tracks = base_window(oracle)
    rng = np.random.default_rng(4103)
    out = {}
    for F0 in F0_SIZES:
        out["f0_%d" % F0] = window_from(w, replicate(tracks, F0, rng))
    long = [t for t in tracks if len(t["j"]) == 10]
    assert len(long) >= 3, "the base window needs tracks seen in all of the frames 1..10"
    sub = lambda t, fr: dict(invd=t["invd"], j=t["j"][np.isin(t["j"], fr)], pts=t["pts"][np.isin(t["j"], fr)])
    out["gaps"] = window_from(w, [sub(t, [1, 3, 7]) for t in replicate(long, 9, rng)])
    out["len1"] = window_from(w, [t if k % 2 == 0 else sub(t, [10]) for k, t in enumerate(replicate(long, 10, rng))])
    out["stagger"] = window_from(w, [sub(t, list(range(1 + k % 3, 11))) for k, t in enumerate(replicate(long, 9, rng))])
    full = replicate(tracks, 12, rng)
    empty = dict(invd=0.1, j=np.zeros(0, int), pts=np.zeros((0, 4)))
    out["noobs"] = window_from(w, full[:5] + [empty] + full[5:])
    out["noobs_without"] = window_from(w, full)
    return out


def batch5(oracle):
    w, tracks = base_window(oracle)
    rng = np.random.default_rng(4104)
    return [window_from(w, replicate(tracks, F0, rng)) for F0 in BATCH5]


def laser0(oracle):
    w, tracks = base_window(oracle)
    return window_from(w, replicate(tracks, 20, np.random.default_rng(4105)), laser_info=np.zeros((6, 6)))


def oracle_marginalize(oracle, win):
    import ctypes as C
    J = np.zeros((66, 66)); r = np.zeros(66); m = C.c_int(0)
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    F0 = len(win["invd"])
    pad = lambda a, dt: a if a.size else np.zeros(4, dt)        # (never read when the counts are 0)
    oracle.lib().lo_marginalize(fp(win["poses"]), fp(win["ex"]), C.c_int(F0), fp(pad(win["invd"], np.float64)), C.c_int(len(win["obs_j"])),
                                fp(pad(win["obs_feat"], np.int32)), fp(pad(win["obs_j"], np.int32)), fp(pad(win["pts"], np.float64)), fp(win["laser01"]),
                                fp(win["laser_info"]), fp(win["mono_info"]), fp(J), fp(r), C.byref(m))
    assert m.value == 6 + F0
    return J, r


def expected_c(win):
    """(H_exp, b_exp, kind): kind "mp" = the 50-digit Schur complement, uncut (6 + F0 <= 30); "np" = fp64 numpy with the cut."""
    if 6 + len(win["invd"]) <= 30:
        Hp, bp, _ = R.marginalize_dense(win)
        return R.to_np(Hp), R.to_np(bp), "mp"
    Hp, bp, _ = R.marginalize_dense_np(win)
    return Hp, bp, "np"
