"""k_marginalize / k_marg_evaluate (through the C ABI) against the CPU restatement (gauge-invariant products)."""
import numpy as np
import pytest

from tests import ba_cases as K

pytestmark = pytest.mark.gpu


def test_marginalize_matches_oracle(oracle, gpu_ctx):
    wins, refs = [], []
    for seed in (5, 6, 8):
        w = K.make_window(seed)
        J, r, m, x0, sel = oracle.marginalize(w)
        refs.append((J, r, x0))
        wins.append(dict(poses=w["poses"], ex=w["ex"], invd=sel["invd"], obs_feat=sel["obs_feat"], obs_j=sel["obs_j"], pts=sel["pts"],
                         laser01=w["laser_consts"][0], laser_info=w["laser_info"], mono_info=w["mono_info"]))
    Jg, rg, st = gpu_ctx.marginalize(wins)
    assert (st == 0).all()
    for k, (J, r, x0) in enumerate(refs):
        H_ref, b_ref = J.T @ J, J.T @ r
        H_gpu, b_gpu = Jg[k].T @ Jg[k], Jg[k].T @ rg[k]
        # structured pseudo-inverse + parallel Jacobi vs dense eigen pseudo-inverse: same prior to ~1e-8 relative
        assert np.abs(H_gpu - H_ref).max() < 1e-7 * np.abs(H_ref).max()
        assert np.abs(b_gpu - b_ref).max() < 1e-7 * (np.abs(b_ref).max() + 1)
        # the prior's cost at a perturbed state: 0.5 |r0 + J dx|^2 is what a solver would see
        from oracle import ba_numpy as B
        rng = np.random.default_rng(k)
        x = np.stack([B.pose_plus(x0[i], rng.normal(0, 1e-3, 6)) for i in range(11)])
        res_gpu = gpu_ctx.marg_evaluate(Jg[k:k + 1], rg[k:k + 1], x0[None], x[None])[0]
        res_self, _ = oracle.marg_evaluate(Jg[k], rg[k], x0, x, want_jac=False)
        assert np.abs(res_gpu - res_self).max() < 1e-9 * (np.abs(res_self).max() + 1)
        res_ref, _ = oracle.marg_evaluate(J, r, x0, x, want_jac=False)
        c_gpu, c_ref = 0.5 * res_gpu @ res_gpu, 0.5 * res_ref @ res_ref
        assert abs(c_gpu - c_ref) < 1e-6 * c_ref


def _prior_products(J, r):
    return J.T @ J, J.T @ r


def test_margin_chain_old_second_new_old(oracle, gpu_ctx):
    """MARGIN_OLD -> MARGIN_SECOND_NEW -> MARGIN_OLD as Estimator::margin() runs them (Estimator.cc:1307-1470),
    GPU against the oracle at every link.  Kept blocks after MARGIN_OLD: [ex, pose1..pose10] = after the address shift
    [ex, pose0..pose9]; MARGIN_SECOND_NEW drops the block aliasing para_pose[WINDOW_SIZE - 1] (index 10)."""
    from oracle import ba_numpy as B
    w = K.make_window(9)
    J0, r0, m, x0, sel = oracle.marginalize(w)
    win = dict(poses=w["poses"], ex=w["ex"], invd=sel["invd"], obs_feat=sel["obs_feat"], obs_j=sel["obs_j"], pts=sel["pts"],
               laser01=w["laser_consts"][0], laser_info=w["laser_info"], mono_info=w["mono_info"])
    Jg0, rg0, st = gpu_ctx.marginalize([win])
    assert st[0] == 0
    rng = np.random.default_rng(11)
    x = np.stack([B.pose_plus(x0[k], rng.normal(0, 2e-3, 6)) for k in range(11)])     # the next frame's state
    # link 2 on both sides from their OWN link-1 priors, and on the GPU from the oracle's prior (isolates the new kernel)
    J1, r1 = oracle.marg_second_new(J0, r0, x0, x, 10)
    Jg1, rg1, st1 = gpu_ctx.marg_second_new(Jg0, rg0, x0[None], x[None], 10)
    Jx1, rx1, _ = gpu_ctx.marg_second_new(J0[None], r0[None], x0[None], x[None], 10)
    assert st1[0] == 0 and Jg1.shape == (1, 60, 60)
    H_ref, b_ref = _prior_products(J1, r1)
    for Jt, rt, tol in ((Jx1[0], rx1[0], 1e-9), (Jg1[0], rg1[0], 1e-6)):
        H, b = _prior_products(Jt, rt)
        assert np.abs(H - H_ref).max() < tol * np.abs(H_ref).max()
        assert np.abs(b - b_ref).max() < tol * (np.abs(b_ref).max() + 1)
    # the new prior's cost at a further perturbed state (what a solver would see), new linearisation point = x without pose9
    xk = np.delete(x, 10, 0)
    xq = np.stack([B.pose_plus(xk[k], rng.normal(0, 1e-3, 6)) for k in range(10)])
    dx = oracle.prior_dx(xk, xq)
    c_ref = 0.5 * np.sum((r1 + J1 @ dx) ** 2); c_gpu = 0.5 * np.sum((rg1[0] + Jg1[0] @ dx) ** 2)
    assert abs(c_gpu - c_ref) < 1e-6 * c_ref
    # link 3: a keyframe again -- MARGIN_OLD builds a fresh prior (the previous one is never chained: `valid` stays false)
    w3 = K.make_window(10)
    J3, r3, m3, x03, sel3 = oracle.marginalize(w3)
    Jg3, rg3, st3 = gpu_ctx.marginalize([dict(poses=w3["poses"], ex=w3["ex"], invd=sel3["invd"], obs_feat=sel3["obs_feat"], obs_j=sel3["obs_j"],
                                              pts=sel3["pts"], laser01=w3["laser_consts"][0], laser_info=w3["laser_info"], mono_info=w3["mono_info"])])
    H_ref, b_ref = _prior_products(J3, r3); H, b = _prior_products(Jg3[0], rg3[0])
    assert st3[0] == 0 and np.abs(H - H_ref).max() < 1e-7 * np.abs(H_ref).max() and np.abs(b - b_ref).max() < 1e-7 * (np.abs(b_ref).max() + 1)


def test_marginalize_150_tracks_anchored_at_frame_0(oracle, gpu_ctx):
    """the tracker keeps up to MAX_CNT = 150 features per frame (FeatureTracker.cc:21) and all of them can be anchored at
    frame 0; lmono_marginalize takes them (capacity 160) and still matches the oracle."""
    w = K.make_window(5)
    J, r, m, x0, sel = oracle.marginalize(w)
    F0 = len(sel["invd"])
    # replicate the frame-0 tracks (slightly different depths / points) up to exactly 150
    rng = np.random.default_rng(2)
    reps = int(np.ceil(150 / F0))
    invd, of, oj, pts = [], [], [], []
    for rep in range(reps):
        for f in range(F0):
            if len(invd) == 150:
                break
            sel_o = np.nonzero(sel["obs_feat"] == f)[0]
            g = len(invd)
            invd.append(sel["invd"][f] * (1 + 0.01 * rep))
            for o in sel_o:
                of.append(g); oj.append(sel["obs_j"][o]); pts.append(sel["pts"][o] + rng.normal(0, 1e-4 * rep, 4))
    assert len(invd) == 150
    w2 = dict(w)
    poses, ex = w["poses"], w["ex"]
    lc = np.ascontiguousarray(w["laser_consts"][0], np.float64)
    invd = np.array(invd); of = np.array(of, np.int32); oj = np.array(oj, np.int32); pts = np.array(pts)
    import ctypes as C
    Jr = np.zeros((66, 66)); rr = np.zeros(66); mm = C.c_int(0)
    li = np.ascontiguousarray(w["laser_info"], np.float64); mi = np.ascontiguousarray(w["mono_info"], np.float64)
    fp = lambda a: a.ctypes.data_as(C.c_void_p)
    oracle.lib().lo_marginalize(fp(np.ascontiguousarray(poses)), fp(np.ascontiguousarray(ex)), C.c_int(150), fp(invd), C.c_int(len(of)), fp(of), fp(oj), fp(pts),
                                fp(lc), fp(li), fp(mi), fp(Jr), fp(rr), C.byref(mm))
    assert mm.value == 156
    Jg, rg, st = gpu_ctx.marginalize([dict(poses=poses, ex=ex, invd=invd, obs_feat=of, obs_j=oj, pts=pts, laser01=lc, laser_info=li, mono_info=mi)])
    H_ref, b_ref = Jr.T @ Jr, Jr.T @ rr
    H, b = Jg[0].T @ Jg[0], Jg[0].T @ rg[0]
    assert np.abs(H - H_ref).max() < 1e-7 * np.abs(H_ref).max() and np.abs(b - b_ref).max() < 1e-7 * (np.abs(b_ref).max() + 1)
    # one more than the capacity is a clean error, not a fault
    import lmono_amd
    big = dict(poses=poses, ex=ex, invd=np.full(161, 0.1), obs_feat=np.arange(161, dtype=np.int32), obs_j=np.full(161, 1, np.int32), pts=np.zeros((161, 4)),
               laser01=lc, laser_info=li, mono_info=mi)
    with pytest.raises(lmono_amd.LmonoError):
        gpu_ctx.marginalize([big])


# ---- constructed spectra, dx branches, window shapes: against the 50-digit reference (tests/marg_ref.py, cases of tests/marg_cases.py) ---------------
# Every comparison: err_gpu <= 8 max(err_oracle, n 2^-52 scale), err_oracle = oracle/lo_marg.c on the same case against the same reference.
def _check(tag, name, err, err_oracle, n, scale):
    from tests import marg_cases as MC
    unit = n * 2.0 ** -52 * scale
    print("%s %-22s err_gpu %9.3g  err_oracle %9.3g  [n 2^-52 scale]" % (tag, name, err / unit, err_oracle / unit))
    assert err <= MC.bound(err_oracle, n, scale), (tag, name, err, err_oracle, unit)


def test_second_new_constructed_spectra(oracle, gpu_ctx):
    """Group A.  tiny_all is the case that found the stalled QL sweeps (status bit 1 set on a 1e-170 matrix) fixed in marg_eig_ql."""
    from tests import marg_cases as MC
    cases = MC.group_a()
    calls = {}
    for c in cases:
        calls.setdefault((c["nb"], c["drop"]), []).append(c)
    for (nb, drop), cs in calls.items():
        Jg, rg, st = gpu_ctx.marg_second_new(np.stack([c["J0"] for c in cs]), np.stack([c["r0"] for c in cs]), np.stack([c["x0"] for c in cs]),
                                             np.stack([c["x"] for c in cs]), drop)
        for k, c in enumerate(cs):
            n = c["n"]
            assert np.isfinite(Jg[k]).all() and np.isfinite(rg[k]).all(), c["name"]
            assert st[k] == c["status"], (c["name"], st[k])
            H_exp, b_exp, E = MC.expected_a(c)
            Jo, ro = oracle.marg_second_new(c["J0"], c["r0"], c["x0"], c["x"], drop)
            eHo, ebo = MC.err_products(Jo, ro, H_exp, b_exp)
            eH, eb = MC.err_products(Jg[k], rg[k], H_exp, b_exp)
            _check("A H'", c["name"], eH, eHo, n, max(np.abs(H_exp).max(), 1e-300))
            _check("A b'", c["name"], eb, ebo, n, np.abs(b_exp).max() + 1)
            # the rows of the cut eigenvalues are exact zeros, and there are exactly n - rank of them
            zero = ~Jg[k].any(1)
            assert zero.sum() == n - len(c["keep"]) and not rg[k][zero].any(), (c["name"], zero.sum())
            if E is not None:
                lam = np.sort(np.sum(Jg[k] * Jg[k], 1)); lam_o = np.sort(np.sum(Jo * Jo, 1)); Ec = np.sort(np.where(E > MC.EPS, E, 0))
                _check("A eig", c["name"], np.abs(lam - Ec).max(), np.abs(lam_o - Ec).max(), n, Ec.max())
            if c["name"] == "tiny_all":
                assert not Jg[k].any() and not rg[k].any()


def test_marg_dx_branches(oracle, gpu_ctx):
    """Group B: flipped quaternions, x0 quaternions of norm 2 and 0.5, ~170 / 190 degree turns; five windows in one launch of each kernel."""
    from tests import marg_cases as MC
    from tests import marg_ref as R
    J0, r0, x0 = MC.real_prior(oracle)
    var = MC.dx_variants(x0, 21)
    names = list(MC.B_VARIANTS)
    res = gpu_ctx.marg_evaluate(np.stack([J0] * 5), np.stack([r0] * 5), np.stack([var[v][0] for v in names]), np.stack([var[v][1] for v in names]))
    for k, v in enumerate(names):
        ref = R.to_np(R.evaluate(J0, r0, *var[v]))
        ro, _ = oracle.marg_evaluate(J0, r0, var[v][0], var[v][1], want_jac=False)
        _check("B res", v, np.abs(res[k] - ref).max(), np.abs(ro - ref).max(), 66, np.abs(ref).max() + 1)
    J5, r5, x05 = MC.shrink_prior(oracle, J0, r0, x0, 5)
    var = MC.dx_variants(x05, 22)
    Jg, rg, st = gpu_ctx.marg_second_new(np.stack([J5] * 5), np.stack([r5] * 5), np.stack([var[v][0] for v in names]), np.stack([var[v][1] for v in names]), 2)
    assert not (st & 2).any()
    for k, v in enumerate(names):
        Hc, bc, _ = R.cut_products(*R.second_new(J5, r5, var[v][0], var[v][1], 2))
        H_exp, b_exp = R.to_np(Hc), R.to_np(bc)
        Jo, ro = oracle.marg_second_new(J5, r5, var[v][0], var[v][1], 2)
        eHo, ebo = MC.err_products(Jo, ro, H_exp, b_exp)
        eH, eb = MC.err_products(Jg[k], rg[k], H_exp, b_exp)
        _check("B H'", v, eH, eHo, 24, np.abs(H_exp).max())
        _check("B b'", v, eb, ebo, 24, np.abs(b_exp).max() + 1)
    # the full-size prior (n = 60) against the oracle alone, every variant in one launch
    var = MC.dx_variants(x0, 23)
    Jg, rg, st = gpu_ctx.marg_second_new(np.stack([J0] * 5), np.stack([r0] * 5), np.stack([var[v][0] for v in names]), np.stack([var[v][1] for v in names]), 5)
    for k, v in enumerate(names):
        Jo, ro = oracle.marg_second_new(J0, r0, var[v][0], var[v][1], 5)
        H_ref, b_ref = Jo.T @ Jo, Jo.T @ ro
        H, b = Jg[k].T @ Jg[k], Jg[k].T @ rg[k]
        assert np.abs(H - H_ref).max() < 1e-9 * np.abs(H_ref).max() and np.abs(b - b_ref).max() < 1e-9 * (np.abs(b_ref).max() + 1), v


def test_marginalize_window_shapes(oracle, gpu_ctx):
    """Group C: F0 across the wave boundaries, gaps, mixed track lengths, several frames in one round, an empty track, offsets inside a batch."""
    from tests import marg_cases as MC
    wins = MC.group_c(oracle)
    names = list(wins)
    Jg, rg, st = gpu_ctx.marginalize([wins[k] for k in names])
    b5 = MC.batch5(oracle)
    J5, r5, st5 = gpu_ctx.marginalize(b5)
    todo = [(k, wins[k], Jg[i], rg[i], st[i]) for i, k in enumerate(names)] + [("batch5_%d" % i, b5[i], J5[i], r5[i], st5[i]) for i in range(5)]
    for name, win, J, r, s in todo:
        assert s == (1 if name == "noobs" else 0), (name, s)
        H_exp, b_exp, kind = MC.expected_c(win)
        sH, sb = np.abs(H_exp).max(), np.abs(b_exp).max() + 1
        eH, eb = MC.err_products(J, r, H_exp, b_exp)
        if kind == "mp":
            Jo, ro = MC.oracle_marginalize(oracle, win)
            eHo, ebo = MC.err_products(Jo, ro, H_exp, b_exp)
            _check("C H'", name, eH, eHo, 66, sH)
            _check("C b'", name, eb, ebo, 66, sb)
        else:
            print("C np   %-22s err_gpu H' %9.3g  b' %9.3g  [relative]" % (name, eH / sH, eb / sb))
            assert eH < 1e-7 * sH and eb < 1e-7 * sb, (name, eH / sH, eb / sb)
    # the empty track changes nothing but the status
    i, j = names.index("noobs"), names.index("noobs_without")
    Ha, ba = MC.products(Jg[i], rg[i]); Hb, bb = MC.products(Jg[j], rg[j])
    assert np.abs(Ha - Hb).max() <= MC.bound(0.0, 66, np.abs(Hb).max()) and np.abs(ba - bb).max() <= MC.bound(0.0, 66, np.abs(bb).max() + 1)
    # laser_info = 0: pose0 is held by the tracks alone; only the status and finiteness are promised
    from tests import marg_ref as R
    win = MC.laser0(oracle)
    J, r, s = gpu_ctx.marginalize([win])
    _, _, wmin = R.marginalize_dense_np(win)
    assert np.isfinite(J).all() and np.isfinite(r).all() and not (s[0] & 2) and (s[0] & 1) == (0 if wmin > MC.EPS else 1), (s, wmin)


def test_marg_deterministic_alone_in_batch_and_again(oracle, gpu_ctx):
    """No atomics across waves, fixed association: a window alone, as the 4th of 5 and once more gives the same bytes."""
    from tests import marg_cases as MC
    b5 = MC.batch5(oracle)
    win = b5[4]
    assert len(win["invd"]) == 129
    alone = gpu_ctx.marginalize([win])
    batch = gpu_ctx.marginalize([b5[0], b5[1], b5[2], win, b5[3]])
    again = gpu_ctx.marginalize([win])
    for a, b, c in zip(alone, batch, again):
        assert a[0].tobytes() == b[3].tobytes() == c[0].tobytes()
    J0, r0, x0 = MC.real_prior(oracle)
    var = MC.dx_variants(x0, 31)
    names = list(MC.B_VARIANTS)
    X0 = np.stack([var[v][0] for v in names]); X = np.stack([var[v][1] for v in names])
    alone = gpu_ctx.marg_second_new(J0[None], r0[None], X0[3:4], X[3:4], 10)
    batch = gpu_ctx.marg_second_new(np.stack([J0] * 5), np.stack([r0] * 5), X0, X, 10)
    again = gpu_ctx.marg_second_new(J0[None], r0[None], X0[3:4], X[3:4], 10)
    for a, b, c in zip(alone, batch, again):
        assert a[0].tobytes() == b[3].tobytes() == c[0].tobytes()


def test_marg_argument_checks(oracle, gpu_ctx):
    """Malformed input is refused on the host before any launch."""
    import ctypes as C
    import lmono_amd
    from tests import marg_cases as MC
    J0 = np.zeros((1, 66, 66)); r0 = np.zeros((1, 66)); x0 = np.zeros((1, 11, 7)); x0[..., 6] = 1
    out = (np.zeros((1, 66, 66)), np.zeros((1, 66)), np.zeros(1, np.int32))
    p = lambda a: a.ctypes.data
    for nb, drop in ((1, 0), (12, 0), (11, -1), (11, 11), (5, 5)):
        rc = gpu_ctx.L.lmono_marg_second_new(gpu_ctx.h, 1, nb, drop, p(J0), p(r0), p(x0), p(x0), p(out[0]), p(out[1]), p(out[2]))
        assert rc == lmono_amd.capi.LMONO_EINVAL if hasattr(lmono_amd.capi, "LMONO_EINVAL") else rc != 0, (nb, drop, rc)
    win = MC.group_c(oracle)["f0_1"]
    win = dict(win, invd=np.concatenate([win["invd"]] * 2), obs_feat=np.concatenate([win["obs_feat"], win["obs_feat"] + 1]),
               obs_j=np.concatenate([win["obs_j"]] * 2), pts=np.concatenate([win["pts"]] * 2))
    gpu_ctx.marginalize([win])                                   # two tracks, well-formed
    n = len(win["obs_j"]) // 2
    assert n >= 2
    for what, mod in (("obs_j 0", dict(obs_j=np.where(np.arange(2 * n) == 1, 0, win["obs_j"]).astype(np.int32))),
                      ("obs_j 11", dict(obs_j=np.where(np.arange(2 * n) == 1, 11, win["obs_j"]).astype(np.int32))),
                      ("not grouped", dict(obs_feat=np.where(np.arange(2 * n) == 0, 1, win["obs_feat"]).astype(np.int32))),
                      ("same frame twice", dict(obs_j=np.where(np.arange(2 * n) == 1, win["obs_j"][0], win["obs_j"]).astype(np.int32)))):
        with pytest.raises(lmono_amd.LmonoError):
            gpu_ctx.marginalize([dict(win, **mod)])
    # the same frame twice and null arrays with nonzero counts: LMONO_EINVAL (-1 would be any error: compare with the header's value)
    einval = gpu_ctx.L.lmono_marg_second_new(gpu_ctx.h, 1, 1, 0, p(J0), p(r0), p(x0), p(x0), p(out[0]), p(out[1]), p(out[2]))
    feat_off = np.array([0, 2], np.int32); obs_off = np.array([0, 2 * n], np.int32)
    dup = np.where(np.arange(2 * n) == 1, win["obs_j"][0], win["obs_j"]).astype(np.int32)
    arrs = dict(invd=win["invd"], obs_feat=win["obs_feat"].astype(np.int32), obs_j=win["obs_j"].astype(np.int32), pts=np.ascontiguousarray(win["pts"]))

    def call(**null):
        a = {k: (None if k in null else p(v)) for k, v in arrs.items()}
        if "dup" in null:
            a["obs_j"] = p(dup)
        return gpu_ctx.L.lmono_marginalize(gpu_ctx.h, 1, p(feat_off), p(obs_off), p(win["poses"]), p(win["ex"]), a["invd"], a["obs_feat"], a["obs_j"], a["pts"],
                                           p(win["laser01"]), p(win["laser_info"]), p(win["mono_info"]), p(out[0]), p(out[1]), p(out[2]))
    assert call() == 0
    assert call(dup=1) == einval != 0
    for k in arrs:
        assert call(**{k: 1}) == einval, k
