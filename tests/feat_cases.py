"""Case builders for the per-track kernels (tests/test_feat_ref_cpu.py, tests/test_feat_gpu.py).  A window is the dict Context._pack_windows takes
(Rs [11,3,3], Ps [11,3], tlc 4x4, trk_start, trk_off, trk_pts) plus 'depth0' (the estimated_depth a call starts from: -1 or a given depth) and 'true'
(the landmark's depth in its anchor camera).  Everything is seeded and small; the builders are cached, so a session builds each case once."""
import functools

import numpy as np

N_FRAMES = 11
BASELINES = (0.8, 0.1, 1e-2, 1e-3, 1e-4)
PIX_NOISE = 5e-4
Z_EDGE_DELTAS = (1e-12, 1e-9, 1e-6, 1e-3)

# camera (x right, y down, z forward) in the LiDAR frame (x forward, y left, z up), with a lever arm
TLC = np.array([[0.0, 0.0, 1.0, 0.27], [-1.0, 0.0, 0.0, -0.06], [0.0, -1.0, 0.0, -0.08], [0.0, 0.0, 0.0, 1.0]])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def camera(w, k):
    R = w["Rs"][k] @ w["tlc"][:3, :3]
    return R, w["Ps"][k] + w["Rs"][k] @ w["tlc"][:3, 3]


def traj_x(baseline):
    """11 frames, the camera translating along its own x axis by `baseline` per frame, no rotation."""
    Rs = np.tile(np.eye(3), (N_FRAMES, 1, 1))
    Ps = np.array([TLC[:3, :3] @ np.array([k * baseline, 0.0, 0.0]) for k in range(N_FRAMES)])
    return Rs, Ps


def traj_rotation():
    """pure rotation: the CAMERA centre stays put while the body yaws 0.02 rad per frame (Ps moves so that Ps + Rs Tlc is constant)."""
    Rs = np.array([rot_z(0.02 * k) for k in range(N_FRAMES)])
    Ps = np.array([TLC[:3, 3] - Rs[k] @ TLC[:3, 3] for k in range(N_FRAMES)])
    return Rs, Ps


def traj_general(seed):
    """a driving camera: ~0.5 m per frame sideways and forward, a few degrees of yaw, small pitch / roll."""
    rng = np.random.default_rng(seed)
    Rs, Ps = [], []
    for k in range(N_FRAMES):
        a = 0.03 * k + 0.004 * rng.standard_normal()
        c, s = np.cos(0.01 * k), np.sin(0.01 * k)
        Rs.append(rot_z(a) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]))
        Ps.append(np.array([0.35 * k, -0.45 * k, 0.02 * k]) + 0.02 * rng.standard_normal(3))
    return np.array(Rs), np.array(Ps)


def build(Rs, Ps, tracks, noise, rng, tlc=TLC):
    """tracks: (start, nobs, depth in the anchor camera, (u, v) in the anchor camera, depth0, noisy) -> window.  The landmark may be behind the camera
    (depth < 0): its observations are the same central projection, which is what a mismatched track hands the triangulation."""
    w = dict(Rs=np.asarray(Rs, float), Ps=np.asarray(Ps, float), tlc=np.asarray(tlc, float))
    start, off, pts, depth0, true = [], [0], [], [], []
    for s, n, d, uv, d0, noisy in tracks:
        assert 0 <= s and n >= 0 and (n == 0 or s + n <= N_FRAMES)
        R0, t0 = camera(w, s)
        X = R0 @ (np.array([uv[0], uv[1], 1.0]) * d) + t0
        for o in range(n):
            R, t = camera(w, s + o)
            q = R.T @ (X - t)
            p = q[:2] / q[2]
            if noisy:
                p = p + noise * rng.standard_normal(2)
            pts.append(p)
        start.append(s); off.append(off[-1] + n); depth0.append(d0); true.append(d)
    w.update(trk_start=np.array(start, np.int32), trk_off=np.array(off, np.int32), trk_pts=np.array(pts, float).reshape(-1, 2),
             depth0=np.array(depth0, float), true=np.array(true, float))
    return w


def _uv(rng):
    return tuple(rng.uniform(-0.4, 0.4, 2))


@functools.lru_cache(maxsize=None)
def parallax_window(baseline):
    """Two tracks of every length 3..11 at depths 2..250 m (log-uniform) with 5e-4 noise; eight exact landmarks at z = 0.1 -+ delta; three behind the camera."""
    rng = np.random.default_rng(int(round(-np.log10(baseline) * 1000)) + 7)
    Rs, Ps = traj_x(baseline)
    tr = []
    for n in range(3, N_FRAMES + 1):
        for _ in range(2):
            tr.append((int(rng.integers(0, N_FRAMES - n + 1)), n, float(np.exp(rng.uniform(np.log(2.0), np.log(250.0)))), _uv(rng), -1.0, True))
    for dl in Z_EDGE_DELTAS:
        for sgn in (-1.0, 1.0):
            tr.append((0, 4, 0.1 + sgn * dl, (0.1, -0.05), -1.0, False))
    tr += [(1, 5, -5.0, (0.2, 0.1), -1.0, False), (0, 8, -30.0, (-0.1, 0.2), -1.0, True), (3, 3, -0.5, (0.0, 0.0), -1.0, True)]
    return build(Rs, Ps, tr, PIX_NOISE, rng)


@functools.lru_cache(maxsize=None)
def rotation_window():
    rng = np.random.default_rng(99)
    Rs, Ps = traj_rotation()
    tr = [(int(rng.integers(0, 4)), int(rng.integers(3, 8)), float(rng.uniform(2, 250)), _uv(rng), -1.0, True) for _ in range(8)]
    return build(Rs, Ps, tr, PIX_NOISE, rng)


def sweep_windows():
    return [parallax_window(b) for b in BASELINES] + [rotation_window()]


@functools.lru_cache(maxsize=None)
def mixed_window(seed=3):
    """Given depths and -1, lengths 1 and 2, anchors at every frame 0..10, tracks ending in frame 10, tracks that are only {9, 10}."""
    rng = np.random.default_rng(seed)
    Rs, Ps = traj_general(seed)
    tr = []
    for s in range(N_FRAMES):
        lens = sorted({1, 2, 3, 4, N_FRAMES - s, N_FRAMES - s - 1} & set(range(1, N_FRAMES - s + 1)))
        for n in lens:
            for given in (False, True):
                d = float(np.exp(rng.uniform(np.log(3.0), np.log(80.0))))
                tr.append((s, n, d, _uv(rng), d * rng.uniform(0.7, 1.4) if given else -1.0, True))
    order = rng.permutation(len(tr))
    return build(Rs, Ps, [tr[k] for k in order], PIX_NOISE, rng)


@functools.lru_cache(maxsize=None)
def plain_window(seed, n_tracks, nobs=None, n_long=0):
    """n_tracks ordinary tracks (depth -1, 5e-4 noise) on the driving trajectory; nobs fixes their length (default: 3..8); the last n_long are one longer."""
    rng = np.random.default_rng(seed)
    Rs, Ps = traj_general(seed)
    tr = []
    for k in range(n_tracks):
        n = int(rng.integers(3, 9)) if nobs is None else nobs + (1 if k >= n_tracks - n_long else 0)
        tr.append((int(rng.integers(0, N_FRAMES - n + 1)), n, float(np.exp(rng.uniform(np.log(3.0), np.log(120.0)))), _uv(rng), -1.0, True))
    return build(Rs, Ps, tr, PIX_NOISE, rng)


def empty_window(seed=0):
    Rs, Ps = traj_general(seed)
    return build(Rs, Ps, [], 0.0, np.random.default_rng(0))


def roundtrip_depth(target):
    """a depth d with 1 / (1 / d) == target in binary64 (the refinement returns 1 / x with x = 1 / depth), searched around target."""
    up = down = float(target)
    for _ in range(64):
        for d in (up, down):
            if 1.0 / (1.0 / d) == target:
                return d
        up, down = float(np.nextafter(up, np.inf)), float(np.nextafter(down, -np.inf))
    raise AssertionError("no binary64 depth round-trips to %r" % target)


def roundtrip_beyond(target, towards):
    """the binary64 depth nearest to target whose 1 / (1 / d) lies strictly on the `towards` side of target."""
    d = float(target)
    for _ in range(64):
        d = float(np.nextafter(d, towards))
        if (1.0 / (1.0 / d) < target) == (towards < target) and 1.0 / (1.0 / d) != target:
            return d
    raise AssertionError("no binary64 depth round-trips beyond %r" % target)


# Why no case reaches the loop's `radius <= 1e-32` exit.  The radius only shrinks through rejected steps (1e4 / 2 / 4 / 8 ...: fifteen in a row), and a
# rejected step is a VALID one: finite, with model > 0.  Per track it is s = -g scale / (h scale^2 + diag / radius) with diag >= 1e-6 (min_diag) and
# scale <= 1, so the move of x is at most 1e6 |g| radius, and the step norm over the window falls in proportion to the radius.  Before the next
# rejection the loop tests the parameter tolerance, |step| <= 1e-8 (|x| + 1e-8), whose right side is at least 1e-16: it ends the loop as soon as
# 1e6 |g| radius sqrt(F) < 1e-16, i.e. long before 1e-32 unless some |g| exceeds ~1e9.  g = sum w^2 J.r / (1 + w^2 |r|^2) is at most w |J| / 2 per
# observation and |J| is about the baseline between the two frames, so that needs weight x baseline ~ 1e9 m with every depth of the window beyond 1e8 m
# -- not a window, and with weight = 1500 out of reach by six orders.  A NaN or inf that would defeat the tolerance test (a NaN step norm, an inf
# cost) makes the step invalid instead, which is the `invalid >= 5` exit hostile_window(True) takes.  So the exit is dead code for finite input; it
# stays in kernel and oracle because the reference's solver has it.
@functools.lru_cache(maxsize=None)
def hostile_window(with_infinity=True):
    """Good tracks plus: a given depth of +inf (a point at infinity: every step of the window's shared trust region is invalid, so `invalid` reaches 5 and
    nothing moves); a runaway start 1 / d = 1e7; exact landmarks whose refined depth falls on either side of 0.1 and of 300; and {9, 10}-only tracks
    (no residual under window_size = 10: their depth only passes through 1 / (1 / d)) whose depth round-trips to exactly 0.1, just below it, exactly 300
    and just above it."""
    rng = np.random.default_rng(17)
    Rs, Ps = traj_x(0.8)
    tr = [(int(rng.integers(0, 5)), int(rng.integers(3, 7)), float(rng.uniform(3, 60)), _uv(rng), -1.0, True) for _ in range(12)]
    tr.append((0, 6, 20.0, (0.1, 0.1), 1e-7, True))                                  # runaway
    for d in (0.09, 0.11, 290.0, 310.0):
        tr.append((0, 10, d, (0.05, -0.02), d, False))                                # exact data, start at the truth
    for d in (roundtrip_depth(0.1), roundtrip_beyond(0.1, 0.0), roundtrip_depth(300.0), roundtrip_beyond(300.0, np.inf)):
        tr.append((9, 2, d, (0.0, 0.1), d, False))
    if with_infinity:
        tr.insert(5, (2, 5, 10.0, (0.2, 0.0), np.inf, True))
    return build(Rs, Ps, tr, PIX_NOISE, rng)


def oracle_triangulate(oracle, w, depth=None, **kw):
    return oracle.triangulate(w["Rs"], w["Ps"], w["tlc"], w["trk_start"], w["trk_off"], w["trk_pts"], w["depth0"] if depth is None else depth, **kw)


def oracle_scores(oracle, w, depth, **kw):
    return oracle.outlier_scores(w["Rs"], w["Ps"], w["tlc"], w["trk_start"], w["trk_off"], w["trk_pts"], depth, **kw)


def shift_case(seed=5, n=24):
    """(back_R0, back_P0, R1, P1, tlc, pt_i [n,2], depth [n]) with shifted z on both sides of 0 and two tracks placed so that it is 0 up to rounding."""
    rng = np.random.default_rng(seed)
    Rs, Ps = traj_general(seed)
    w = dict(Rs=Rs, Ps=Ps, tlc=TLC)
    (Ra, ta), (Rb, tb) = camera(w, 0), camera(w, 1)
    pt = rng.uniform(-0.4, 0.4, (n, 2)); dep = np.exp(rng.uniform(np.log(0.05), np.log(100.0), n))
    dep[:4] = -dep[:4]                                                                 # negative input depths
    for k in (4, 5):                                                                   # z in the new camera: row 2 of Rb^T (Ra p d + ta - tb) = 0 -> d
        p = np.array([pt[k, 0], pt[k, 1], 1.0]); a = (Rb.T @ Ra @ p)[2]; b = (Rb.T @ (ta - tb))[2]
        dep[k] = -b / a
    return Rs[0], Ps[0], Rs[1], Ps[1], TLC, pt, dep


# ---- the linear step against the 50-digit SVD (shared by the CPU run of the oracle and the GPU run of the kernel) -------------------------------------
LINEAR_FACTOR = 64 * 2.0 ** -52          # the issue's bound: 64 eps sigma1^2 / (sigma3^2 - sigma4^2)
LINEAR_EXCLUDE = 1e-6


@functools.lru_cache(maxsize=None)
def sweep_reference():
    """per sweep window: (z_ref [F] as mpf, bound [F] float) from tests/feat_ref.linear_triangulation -- computed once per session."""
    from tests import feat_ref as R
    out = []
    for w in sweep_windows():
        cams = R.cameras(w)
        zs, bs = [], []
        for f in range(len(w["trk_start"])):
            z, s, _ = R.linear_triangulation(w, f, cams)
            gap = s[2] ** 2 - s[3] ** 2
            zs.append(z); bs.append(float(LINEAR_FACTOR * s[0] ** 2 / gap) if gap > 0 else np.inf)
        out.append((zs, np.array(bs)))
    return out


def linear_step_report(d0_per_window):
    """Compares linear-step depths (one array per sweep window, -1 = rejected) with the reference.  Returns dict(n, excluded, worst_ratio, below, above,
    failures): failures lists every track that breaks the value bound or the z < 0.1 decision; below / above count the tracks whose decision is checked."""
    from mpmath import mpf
    rep = dict(n=0, excluded=0, worst_ratio=0.0, below=0, above=0, failures=[])
    for k, ((zs, bs), d0) in enumerate(zip(sweep_reference(), d0_per_window)):
        for f, (z, b) in enumerate(zip(zs, bs)):
            rep["n"] += 1
            got = float(d0[f])
            decidable = abs(z - mpf("0.1")) > b * abs(z)             # b bounds the relative error of z
            if decidable:
                rep["below" if z < 0.1 else "above"] += 1
                if (got == -1.0) != bool(z < 0.1):
                    rep["failures"].append("window %d track %d: z_ref = %s but the linear step gave %r" % (k, f, mpf(z), got))
                    continue
            if not (b <= LINEAR_EXCLUDE):
                rep["excluded"] += 1
                continue
            if got == -1.0 or z < 0.1:
                continue                                              # rejected on both sides (or undecidable at the threshold): no value to compare
            ratio = float(abs((mpf(got) - z) / z)) / b
            rep["worst_ratio"] = max(rep["worst_ratio"], ratio)
            if not ratio <= 1.0:
                rep["failures"].append("window %d track %d: relative error / bound = %.3g (z_ref = %.17g, bound %.3g)" % (k, f, ratio, float(z), b))
    return rep


# ---- raw C-ABI calls (liblmono_hip.so and the CPU shim share the signatures) and malformed descriptors --------------------------------------------------
def pack(windows):
    """what Context._pack_windows builds, as a dict of arrays (restated here: the malformed cases edit these arrays)."""
    W = len(windows)
    Rs = np.zeros((W, 11, 9)); Ps = np.zeros((W, 11, 3))
    for k, w in enumerate(windows):
        Rs[k] = np.asarray(w["Rs"]).reshape(11, 9); Ps[k] = w["Ps"]
    tlc = np.ascontiguousarray([np.asarray(w["tlc"]).ravel() for w in windows], np.float64)
    feat_off = np.concatenate([[0], np.cumsum([len(w["trk_start"]) for w in windows])]).astype(np.int32)
    start = np.ascontiguousarray(np.concatenate([w["trk_start"] for w in windows]), np.int32)
    offs, base = [0], 0
    for w in windows:
        offs.extend((np.asarray(w["trk_off"][1:]) + base).tolist()); base += int(w["trk_off"][-1])
    pts = np.ascontiguousarray(np.concatenate([np.asarray(w["trk_pts"]).reshape(-1, 2) for w in windows]), np.float64)
    return dict(W=W, feat_off=feat_off, Rs=Rs, Ps=Ps, tlc=tlc, start=start, obs_off=np.array(offs, np.int32), pts=pts)


def malformed(p):
    """(label, packed descriptor, extra arguments) of every structural error the per-track entry points must refuse; p: pack() of >= 2 windows."""
    def edit(**kw):
        q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        for k, fn in kw.items():
            fn(q[k])
        return q
    F = int(p["feat_off"][-1])
    long_f = int(np.argmax(np.diff(p["obs_off"])))
    nobs = int(np.diff(p["obs_off"])[long_f])

    def set_(i, v):
        return lambda a: a.__setitem__(i, v)
    return [
        ("feat_off[0] != 0", edit(feat_off=set_(0, 1)), {}),
        ("feat_off descending", edit(feat_off=set_(1, int(p["feat_off"][2]) + 1)), {}),
        ("obs_off descending", edit(obs_off=set_(F // 2, int(p["obs_off"][F // 2 + 1]) + 1)), {}),
        ("obs_off[0] negative", edit(obs_off=set_(0, -1)), {}),
        ("start_frame negative", edit(start=set_(3, -1)), {}),
        ("start_frame + nobs > 11", edit(start=set_(long_f, 12 - nobs)), {}),
        ("start_frame + nobs > 11 in the last track", edit(start=set_(F - 1, 11)), {}),
        ("track_cnt 0", p, dict(track_cnt=0)),
        ("track_cnt negative", p, dict(track_cnt=-3)),
        ("window_size 11", p, dict(window_size=11)),
        ("window_size -1", p, dict(window_size=-1)),
        ("refine_max_iter above the cap", p, dict(refine_iters=1001)),
    ]


def raw_triangulate(L, h, q, depth, flag, track_cnt=3, window_size=10, weight=1500.0, refine_iters=50):
    import ctypes as C
    L.lmono_triangulate.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_int, C.c_double, C.c_int]
    return L.lmono_triangulate(h, q["W"], q["feat_off"].ctypes.data, q["Rs"].ctypes.data, q["Ps"].ctypes.data, q["tlc"].ctypes.data, q["start"].ctypes.data,
                               q["obs_off"].ctypes.data, q["pts"].ctypes.data, depth.ctypes.data, flag.ctypes.data, track_cnt, window_size, weight, refine_iters)


def raw_scores(L, h, q, depth, score, track_cnt=3, weight=1500.0):
    import ctypes as C
    L.lmono_outlier_scores.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_double, C.c_void_p]
    return L.lmono_outlier_scores(h, q["W"], q["feat_off"].ctypes.data, q["Rs"].ctypes.data, q["Ps"].ctypes.data, q["tlc"].ctypes.data, q["start"].ctypes.data,
                                  q["obs_off"].ctypes.data, q["pts"].ctypes.data, depth.ctypes.data, track_cnt, weight, score.ctypes.data)


def raw_shift_batch(L, h, frames, off, pt, dep, out):
    import ctypes as C
    L.lmono_shift_depth_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return L.lmono_shift_depth_batch(h, len(off) - 1, frames.ctypes.data, off.ctypes.data, pt.ctypes.data, dep.ctypes.data, out.ctypes.data)


EINVAL = -1


def check_malformed_refused(L, h, windows):
    """Every malformed descriptor answers LMONO_EINVAL from lmono_triangulate and lmono_outlier_scores and leaves depth / flag / score as they were; the
    batched shift refuses bad offsets likewise.  Host-side only: a refused call uploads and launches nothing."""
    p = pack(windows)
    F = int(p["feat_off"][-1])
    for label, q, extra in malformed(p):
        depth = np.full(F, -1.0); flag = np.full(F, 77, np.int32); score = np.full(F, 123.0)
        rc = raw_triangulate(L, h, q, depth, flag, **extra)
        assert rc == EINVAL, (label, rc)
        assert (depth == -1.0).all() and (flag == 77).all(), label
        if "track_cnt" in extra or not extra:
            rc = raw_scores(L, h, q, np.full(F, 5.0), score, **{k: v for k, v in extra.items() if k == "track_cnt"})
            assert rc == EINVAL, (label, rc)
            assert (score == 123.0).all(), label
    frames = np.zeros((3, 40)); pt = np.zeros((6, 2)); dep = np.ones(6)
    for off in ([1, 2, 4, 6], [0, 4, 2, 6], [0, 2, 4, -1]):
        out = np.full(6, 9.0)
        assert raw_shift_batch(L, h, frames, np.array(off, np.int32), pt, dep, out) == EINVAL, off
        assert (out == 9.0).all(), off


# ---- the refinement as an optimiser: every window of the case families, on the kernel the dispatch gives it ----------------------------------------------
def optimiser_cases():
    """name -> (batch, index of the window under test).  The windows above 256 tracks run on the kernel named: w600 alone would take the items kernel, so it
    is batched with the 1025-track window, which sends the whole batch to the 256-thread kernel."""
    c = {"parallax %g" % b: ([parallax_window(b)], 0) for b in BASELINES}
    c.update({
        "rotation": ([rotation_window()], 0), "mixed": ([mixed_window()], 0),
        "hostile with infinity": ([hostile_window(True)], 0), "hostile": ([hostile_window(False)], 0),
        "plain 40": ([plain_window(31, 40)], 0), "plain 200": ([plain_window(31, 200)], 0),
        "1024 tracks (items kernel)": ([plain_window(21, 1024, nobs=3)], 0), "1025 tracks (256-thread kernel)": ([plain_window(22, 1025, nobs=3)], 0),
        "3072 observations (items kernel)": ([plain_window(23, 384, nobs=8)], 0), "3073 observations (256-thread kernel)": ([plain_window(23, 384, nobs=8, n_long=1)], 0),
        "600 tracks (items kernel)": ([plain_window(24, 600, nobs=4)], 0),
        "600 tracks (256-thread kernel)": ([plain_window(24, 600, nobs=4), plain_window(22, 1025, nobs=3)], 0),
    })
    return c


NEWTON_MAX_TRACKS = 130      # the Newton-step bound differentiates every track at 50 digits: windows up to this size
