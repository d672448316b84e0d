"""The 50-digit marginalisation reference (tests/marg_ref.py) and the case generators (tests/marg_cases.py) against oracle/lo_marg.c and a dense numpy
computation, on every case the GPU tests run; the generators' stated conditions are proved here, without a GPU.  Run with -s for the oracle's error table."""
import numpy as np

from tests import marg_cases as MC
from tests import marg_ref as R
from tests.test_marg_cpu import _second_new_numpy

_table = {}


def _note(group, what, err, n, scale):
    key = (group, what)
    _table[key] = max(_table.get(key, 0.0), err / (n * 2.0 ** -52 * scale))


def test_prior_dx_matches_numpy(oracle):
    rng = np.random.default_rng(1)
    x0 = np.stack([MC.K.rand_pose(rng) for _ in range(11)])
    for name, (y0, x) in MC.dx_variants(x0, 3).items():
        ref = R.to_np(R.prior_dx(y0, x))
        assert np.abs(oracle.prior_dx(y0, x) - ref).max() < 1e-14 * (np.abs(ref).max() + 1), name


def test_group_a_reference_oracle_numpy(oracle):
    names = set()
    for c in MC.group_a():
        names.add(c["name"])
        n = c["n"]
        H_exp, b_exp, E = MC.expected_a(c)
        Jo, ro = oracle.marg_second_new(c["J0"], c["r0"], c["x0"], c["x"], c["drop"])
        eH, eb = MC.err_products(Jo, ro, H_exp, b_exp)
        sH, sb = np.abs(H_exp).max(), np.abs(b_exp).max() + 1
        _note("A", "H'", eH, n, max(sH, 1e-300)); _note("A", "b'", eb, n, sb)
        Hn, bn = _second_new_numpy(c["J0"], c["r0"], c["x0"], c["x"], c["drop"], oracle)
        # three independent routes to the same products; 1e-10 relative leaves room for the dense Jacobi / eigh of the graded spectrum (1e10 spread)
        for tag, (dH, db) in (("oracle", (eH, eb)), ("numpy", (np.abs(Hn - H_exp).max(), np.abs(bn - b_exp).max()))):
            assert dH <= 1e-10 * sH and db <= 1e-10 * sb, (c["name"], tag, dH, db)
        # generator conditions
        lam = np.sum(c["S"] ** 2, 1)                                       # eigenvalues by construction (squared row norms of S)
        if c["name"] in ("tiny_all", "tiny_tridiag"):
            assert np.sum(c["S"][np.setdiff1d(np.arange(n), c["keep"])] ** 2) < MC.EPS / 100       # (the trace bounds every cut eigenvalue)
        elif c["ref"] == "rows" and c["name"] != "tridiag" and not c["name"].startswith("size_"):
            kept = np.zeros(n, bool); kept[c["keep"]] = True
            assert (lam[kept] > 100 * MC.EPS).all() and (lam[~kept] < MC.EPS / 100).all(), c["name"]
            G = c["S"] @ c["S"].T                                          # rows orthogonal to rounding: the spectrum is lam
            assert np.abs(G - np.diag(np.diag(G))).max() <= 1e-14 * max(lam.max(), 1e-300), c["name"]
        if c["name"] == "tridiag" or c["name"].startswith("size_"):
            assert np.linalg.svd(c["S"], compute_uv=False).min() ** 2 > 100 * MC.EPS
        if c["name"] == "tridiag":
            H = c["S"].T @ c["S"]
            assert np.abs(np.triu(H, 2)).max() == 0.0 and np.abs(np.diag(H, 1)).min() > 0.0
        if c["name"] == "blockdiag":
            assert not c["S"][30:].any() and not c["S"][:, 30:].any()
        if c["name"].startswith("diag"):
            assert np.count_nonzero(c["S"] - np.diag(np.diag(c["S"]))) == 0
        if c["name"].startswith("rank_k"):
            assert np.count_nonzero(~c["S"].any(1)) == int(c["name"][6:]) and np.count_nonzero(np.abs(Jo).sum(1)) == len(c["keep"])
        if c["name"] == "tiny_all":
            assert 1e-87 < np.abs(c["S"]).max() < 1e-85 and not Jo.any() and not ro.any()
        if c["name"] == "tiny_tridiag":
            T = c["S"].T @ c["S"]
            hits = MC.ql_trace(np.diag(T), np.diag(T, 1))
            assert (0, 2, 0) in hits and all(h[1] >= 0 for h in hits), hits      # underflow met at step i = 0 < m - 1 with one rotation listed; no cap
            assert all(h[1] < 0 or h[2] < h[1] - 1 for h in hits), hits           # never in a sweep's first step (which would list nothing and stall)
        if c["name"] == "singular_drop":
            assert not c["J0"][:6].any()
            kp = [6 * k + q for k in range(c["nb"]) if k != c["drop"] for q in range(6)]
            Hk = (c["J0"].T @ c["J0"])[np.ix_(kp, kp)]
            assert np.abs(Hk - H_exp).max() <= n * 2.0 ** -52 * sH
        if E is not None:
            assert (np.abs(np.log10(E / MC.EPS)) > 2).all(), c["name"]           # nothing within a factor 100 of the cut
            assert np.abs(np.sort(np.sum(Jo * Jo, 1)) - np.sort(np.where(E > MC.EPS, E, 0))).max() <= 1e-10 * E.max()
        if c["name"] == "gap_n30":
            # the by-construction expectation against the full 50-digit route
            Hp, bp = R.second_new(c["J0"], c["r0"], c["x0"], c["x"], c["drop"])
            Hc, bc, Em = R.cut_products(Hp, bp)
            Em = np.array([float(v) for v in Em])
            assert (np.abs(np.log10(Em / MC.EPS)) > 2).all() and (Em > MC.EPS).sum() == 27 and abs(Em.max() - 1.0) < 1e-12
            assert np.abs(R.to_np(Hc) - H_exp).max() < 1e-15 and np.abs(R.to_np(bc) - b_exp).max() < 1e-15
            k = c["keep"]; Sk = R.M(c["S"][k])
            assert R.maxabs(Sk.T * Sk - Hc) < 1e-18 and R.maxabs(Sk.T * R.M(c["rs"][k]) - bc) < 1e-18
    want = {"diag_n60", "diag_n6", "tridiag", "blockdiag", "repeat_identity", "repeat_clusters", "graded", "rank_k1", "rank_k6", "rank_k59", "gap_n30", "gap_n60",
            "tiny_all", "tiny_tridiag", "singular_drop"} | {"size_nb%d_drop%d" % (nb, d) for nb in range(2, 12) for d in (0, nb // 2, nb - 1)}
    assert names == want


def test_tiny_first_step_underflow_is_what_the_floor_removes():
    """Without the |e| < 1e-150 rule a 1e-170 tridiagonal meets f^2 + g^2 == 0 in the first step of every sweep and runs into the cap."""
    d = np.full(6, 2e-170); e = np.full(5, 1e-170)
    assert (0, -1, -1) in MC.ql_trace(d, e, tiny=0.0)
    assert MC.ql_trace(d, e) == []


def test_group_b_reference_oracle(oracle):
    J0, r0, x0 = MC.real_prior(oracle)
    flips = 0
    for name, (y0, x) in MC.dx_variants(x0, 21).items():
        ref = R.to_np(R.evaluate(J0, r0, y0, x))
        res, _ = oracle.marg_evaluate(J0, r0, y0, x, want_jac=False)
        sc = np.abs(ref).max() + 1
        err = np.abs(res - ref).max()
        _note("B", "residual", err, 66, sc)
        assert err <= 1e-10 * sc, (name, err)
        q0, q = y0[:, 3:], x[:, 3:]
        rw = q0[:, 3] * q[:, 3] + (q0[:, :3] * q[:, :3]).sum(1)
        flips += (rw < 0).sum()
        if name in ("flip", "turn190"):
            assert (rw < 0).any(), name
        if name == "turn170":
            assert (rw > 0).all() and (rw < 0.12).all()
    assert flips > 0
    J5, r5, x05 = MC.shrink_prior(oracle, J0, r0, x0, 5)
    for name, (y0, x) in MC.dx_variants(x05, 22).items():
        Hp, bp = R.second_new(J5, r5, y0, x, 2)
        Hc, bc, E = R.cut_products(Hp, bp)
        H_exp, b_exp = R.to_np(Hc), R.to_np(bc)
        Jo, ro = oracle.marg_second_new(J5, r5, y0, x, 2)
        eH, eb = MC.err_products(Jo, ro, H_exp, b_exp)
        sH, sb = np.abs(H_exp).max(), np.abs(b_exp).max() + 1
        _note("B", "H'", eH, 24, sH); _note("B", "b'", eb, 24, sb)
        assert eH <= 1e-9 * sH and eb <= 1e-9 * sb, (name, eH / sH, eb / sb)


def test_group_c_reference_oracle_numpy(oracle):
    wins = MC.group_c(oracle)
    assert set(wins) == {"f0_%d" % f for f in MC.F0_SIZES} | {"gaps", "len1", "stagger", "noobs", "noobs_without"}
    for name, win in list(wins.items()) + [("batch5_%d" % k, w) for k, w in enumerate(MC.batch5(oracle))]:
        H_exp, b_exp, kind = MC.expected_c(win)
        Jo, ro = MC.oracle_marginalize(oracle, win)
        eH, eb = MC.err_products(Jo, ro, H_exp, b_exp)
        sH, sb = np.abs(H_exp).max(), np.abs(b_exp).max() + 1
        if kind == "mp":
            _note("C", "H'", eH, 66, sH); _note("C", "b'", eb, 66, sb)
            # the uncut 50-digit H' / b' are the expectation: every eigenvalue is either far above the cut or so small that cutting it or not moves
            # H' by no more than the rounding of the Schur complement itself, n 2^-52 max|H| (with F0 = 0 the exact H' is 0 and what anyone computes
            # is rounding of H_rr; the oracle's error, which enters the bound, is of that size), and b' has no more than n 2^-52 (max|b| + 1) along them
            Hn, bn, _ = R.marginalize_dense_np(win, cut=False)
            ev, V = np.linalg.eigh(0.5 * (Hn + Hn.T))
            sR = np.abs(R.assemble_dense(win)[0]).max()              # errors of a Schur complement are relative to what was subtracted
            small = np.abs(ev) <= 66 * 2.0 ** -52 * sR
            assert (small | (ev > 100 * MC.EPS)).all(), (name, ev[:8])
            assert np.abs(V[:, small] @ (V[:, small].T @ bn)).max() <= 66 * 2.0 ** -52 * (np.abs(R.assemble_dense(win)[1]).max() + 1), name
            print("C %-14s oracle err H' %9.3g b' %9.3g  max|H'| %9.3g max|H| %9.3g  ev[:7] %s" % (name, eH, eb, sH, sR, ev[:7]))
            assert np.abs(Hn - H_exp).max() <= 1e-9 * sR and np.abs(bn - b_exp).max() <= 1e-9 * sb, name
            assert eH <= 1e-8 * sR and eb <= 1e-8 * sb, (name, kind, eH / sR, eb / sb)
        else:
            assert eH <= 1e-8 * sH and eb <= 1e-8 * sb, (name, kind, eH / sH, eb / sb)       # the bound of test_marg_cpu.py for this comparison
    assert len(wins["f0_0"]["invd"]) == 0 and [len(w["invd"]) for w in MC.batch5(oracle)] == list(MC.BATCH5)
    assert any(len(s) >= 3 for s in MC.round_frames(wins["stagger"])), MC.round_frames(wins["stagger"])
    assert set(wins["gaps"]["obs_j"]) == {1, 3, 7} and all(s <= {1, 3, 7} for s in MC.round_frames(wins["gaps"]))
    per = [int((wins["len1"]["obs_feat"] == f).sum()) for f in range(len(wins["len1"]["invd"]))]
    assert set(per) == {1, 10} and set(wins["len1"]["obs_j"][[o for o in range(len(wins["len1"]["obs_j"])) if per[wins["len1"]["obs_feat"][o]] == 1]]) == {10}
    assert 5 not in set(wins["noobs"]["obs_feat"]) and len(wins["noobs"]["invd"]) == 13
    # the empty track only adds a zero row / column to H_mm: the same products as the window without it
    Ha, ba, _ = MC.expected_c(wins["noobs"]); Hb, bb, _ = MC.expected_c(wins["noobs_without"])
    assert np.abs(Ha - Hb).max() <= 1e-12 * np.abs(Hb).max() and np.abs(ba - bb).max() <= 1e-12 * (np.abs(bb).max() + 1)
    # laser_info = 0: the dense H_mm's smallest eigenvalue is clear of the cut, so status bit 0 has a definite expectation
    _, _, wmin = R.marginalize_dense_np(MC.laser0(oracle))
    assert wmin > 100 * MC.EPS or wmin < MC.EPS / 100


def test_error_table():
    """The oracle's error against the 50-digit reference in units of n 2^-52 scale, per group (filled by the tests above; -s prints it)."""
    for (g, what), v in sorted(_table.items()):
        print("oracle error  group %s  %-9s %10.3g  x n 2^-52 scale" % (g, what, v))
    assert all(np.isfinite(v) for v in _table.values())
