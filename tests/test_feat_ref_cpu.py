"""The 50-digit references (tests/feat_ref.py) and the case builders (tests/feat_cases.py) of the per-track kernels, checked on the CPU against the
oracle's C code -- and the oracle's linear step (the eigenvector of A^T A, the kernel's own algorithm) checked against the SVD of A the reference takes.
tests/test_feat_gpu.py asks the same of the HIP kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import feat_cases as K
from tests import feat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_linear_step_within_the_svd_bound(oracle):
    """Per track, |z - z_ref| / |z_ref| <= 64 * 2^-52 * sigma1^2 / (sigma3^2 - sigma4^2) with sigma from the 50-digit SVD of A: forming A^T A squares
    the singular values, its smallest eigenvector moves by eps |A^T A| / gap = eps sigma1^2 / (sigma3^2 - sigma4^2) (Davis-Kahan), and 64 covers the
    22-row accumulation and the Jacobi sweeps.  Measured for the oracle's C code on the sweep (baselines 0.8 .. 1e-4 m per frame, depths 2 .. 250 m,
    5e-4 noise, plus a pure rotation; 153 tracks): largest error / bound = 0.075 (at 0.1 m per frame), 0.07 at 0.8 m, 0.011 at 1e-2, 0.0025 at 1e-3,
    0.0012 at 1e-4; one track of 153 (0.7 %) has a bound above 1e-6 and is left out of the value comparison; the z < 0.1 decision equals the
    reference's on every track whose distance from 0.1 exceeds its bound.  So the bound is neither too tight nor absurdly loose (a factor 13), and
    the squared conditioning stays far below what would move a depth the Estimator uses."""
    d0 = [K.oracle_triangulate(oracle, w, refine_iters=-1)[0] for w in K.sweep_windows()]
    rep = K.linear_step_report(d0)
    print("linear step, oracle vs 50-digit SVD: %d tracks, %d excluded (%.1f %%), largest error / bound = %.3g, decisions checked: %d below 0.1, %d above"
          % (rep["n"], rep["excluded"], 100.0 * rep["excluded"] / rep["n"], rep["worst_ratio"], rep["below"], rep["above"]))
    assert not rep["failures"], "\n".join(rep["failures"])
    assert rep["excluded"] * 4 <= rep["n"]
    assert rep["below"] >= 5 and rep["above"] >= 5


def test_sweep_holds_what_it_claims():
    for b, w in zip(K.BASELINES, K.sweep_windows()):
        n = np.diff(w["trk_off"])
        assert set(n[:18]) == set(range(3, 12)) and w["true"][:18].min() >= 2 and w["true"][:18].max() <= 250
        assert (w["true"] < 0).sum() == 3
        for dl in K.Z_EDGE_DELTAS:
            assert (np.abs(w["true"] - (0.1 + dl)) < 1e-15).sum() == 1 and (np.abs(w["true"] - (0.1 - dl)) < 1e-15).sum() == 1
        c = [K.camera(w, k)[1] for k in range(11)]
        assert np.allclose(np.linalg.norm(np.diff(c, axis=0), axis=1), b, rtol=1e-9)
    w = K.rotation_window()
    c = np.array([K.camera(w, k)[1] for k in range(11)])
    assert np.abs(c - c[0]).max() < 1e-15 and np.abs(w["Rs"][10] - w["Rs"][0]).max() > 0.1


def test_reference_matches_oracle_on_the_mixed_window(oracle):
    """residual / cost / score / linear step of the plain reference against the oracle where both are well conditioned (the driving trajectory)."""
    w = K.mixed_window()
    n = np.diff(w["trk_off"])
    assert set(w["trk_start"]) == set(range(11)) and {1, 2} <= set(n)
    assert ((w["trk_start"] == 9) & (n == 2)).any() and ((w["trk_start"] + n == 11) & (n >= 3)).any()
    assert (w["depth0"] > 0).sum() > 10 and (w["depth0"] == -1).sum() > 10
    d0, d1, flag = K.oracle_triangulate(oracle, w)
    assert (flag[n < 3] == 0).all() and (d1[n < 3] == w["depth0"][n < 3]).all()                 # short tracks: untouched
    assert (d0[w["depth0"] > 0] == w["depth0"][w["depth0"] > 0]).all()                           # a given depth skips the linear step
    cams = R.cameras(w)
    sc = K.oracle_scores(oracle, w, d1)
    for f in range(0, len(n), 3):
        if n[f] < 3:
            assert sc[f] == -1.0
            continue
        ref = R.outlier_score(w, f, d1[f], cams=cams)
        assert abs(sc[f] - float(ref)) <= 1e-9 * max(1.0, float(ref))
        if w["depth0"][f] < 0:
            z, s, _ = R.linear_triangulation(w, f, cams)
            assert abs(d0[f] - float(z)) <= 1e-9 * float(z)
    # the cost the oracle minimises is the reference's: its refinement does not raise it
    c0 = sum(R.cauchy_cost(w, f, 1.0 / d0[f], cams=cams) for f in range(len(n)))
    c1 = sum(R.cauchy_cost(w, f, 1.0 / d1[f], cams=cams) for f in range(len(n)))
    assert c1 <= c0 and c1 < 0.9 * c0
    # Gauss-Newton terms against a difference quotient of the cost (rho' J.r is the cost's derivative)
    f = int(np.nonzero((n >= 4) & (w["trk_start"] < 5))[0][0])
    x = R.mpf(1.0 / d0[f])
    g, h = R.gauss_newton_terms(w, f, x, cams=cams)
    assert abs(R.mp.diff(lambda t: R.cauchy_cost(w, f, t, cams=cams), x) - g) <= 1e-30 * abs(g) and h > 0


def test_reference_shifted_depth_matches_oracle(oracle):
    a = K.shift_case()
    out = oracle.shift_depth(*a)
    pt, dep = a[5], a[6]
    assert (out == -1.0).sum() >= 4 and (out > 0).sum() >= 10
    for k in range(len(dep)):
        ref = float(R.shifted_depth(*a[:5], pt[k], dep[k]))
        if k in (4, 5):                      # placed at z = 0 up to rounding: either sign is right, and then the answer is -1 or that tiny z
            assert out[k] == -1.0 or 0 < out[k] < 1e-12
        else:
            assert abs(out[k] - ref) <= 1e-12 * max(1.0, abs(ref))


def test_limit_and_hostile_cases_are_what_they_claim(oracle):
    assert len(K.plain_window(21, 1024, nobs=3)["trk_start"]) == 1024 and K.plain_window(21, 1024, nobs=3)["trk_off"][-1] == 3072
    assert len(K.plain_window(22, 1025, nobs=3)["trk_start"]) == 1025
    assert K.plain_window(23, 384, nobs=8)["trk_off"][-1] == 3072 and K.plain_window(23, 384, nobs=8, n_long=1)["trk_off"][-1] == 3073
    # hostile: the point at infinity makes every step invalid -- five of them end the loop and no depth moves
    w = K.hostile_window()
    info = np.zeros(3)
    d0, d1, flag = K.oracle_triangulate(oracle, w, info=info)
    assert info[0] == 2 and info[1] == 5, info
    n = np.diff(w["trk_off"])
    with np.errstate(divide="ignore"):
        assert np.array_equal(1.0 / (1.0 / d0[n >= 3]), d1[n >= 3])
    # without it the window is refined: final depths on both sides of 0.1 and of 300, the runaway track flagged 2
    w = K.hostile_window(False)
    d0, d1, flag = K.oracle_triangulate(oracle, w, info=info)
    assert info[0] in (1, 3, 4), info
    ex = slice(13, 17)
    assert list(flag[ex]) == [2, 1, 1, 2] and d1[13] < 0.1 < d1[14] and d1[15] < 300 < d1[16]
    assert flag[12] == 2 or abs(d1[12] - 20.0) < 2.0          # the runaway start either stays lost (flag 2) or is pulled back
    # the {9, 10}-only tracks under track_cnt = 2: no residual, the depth passes through 1 / (1 / d) and lands exactly on the limits
    d0, d1, flag = K.oracle_triangulate(oracle, w, track_cnt=2)
    assert d1[17] == 0.1 and d1[18] < 0.1 and 0.1 - d1[18] < 1e-15 and d1[19] == 300.0 and d1[20] > 300.0 and d1[20] - 300.0 < 1e-12, d1[17:21]
    assert list(flag[17:21]) == [1, 2, 1, 2]


@pytest.fixture(scope="module")
def shim(oracle, tmp_path_factory):
    """oracle/cpu_shim.cpp (the CPU twin of the per-track entry points) as a shared library."""
    so = str(tmp_path_factory.mktemp("shim") / "liblmono_cpu_shim.so")
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", os.path.join(odir, "cpu_shim.cpp"), "-o", so,
                           "-L" + odir, "-llmono_oracle", "-Wl,-rpath," + odir, "-lm"])
    L = C.CDLL(so)
    L.lmono_create.restype = C.c_void_p
    L.lmono_create.argtypes = [C.c_int]
    L.lmono_destroy.argtypes = [C.c_void_p]
    L.lmono_last_error.restype = C.c_char_p
    L.lmono_last_error.argtypes = [C.c_void_p]
    h = L.lmono_create(0)
    yield L, h
    L.lmono_destroy(h)


def test_cpu_shim_refuses_malformed_descriptors(shim, oracle):
    L, h = shim
    wins = [K.mixed_window(), K.hostile_window(False)]
    K.check_malformed_refused(L, h, wins)
    assert b"window_size" in L.lmono_last_error(h) or b"offsets" in L.lmono_last_error(h)
    # and the well-formed call goes through, empty windows first, in the middle and last, with the oracle's bytes
    batch = [K.empty_window(), wins[0], K.empty_window(), wins[1], K.empty_window()]
    p = K.pack(batch)
    depth = np.concatenate([w["depth0"] for w in batch]); flag = np.zeros(len(depth), np.int32)
    assert K.raw_triangulate(L, h, p, depth, flag) == 0
    want = np.concatenate([K.oracle_triangulate(oracle, w)[1] for w in wins])
    assert depth.tobytes() == want.tobytes()


def test_pack_equals_the_context_packing():
    """tests/feat_cases.pack restates Context._pack_windows so that the malformed cases can edit its arrays: the two must stay the same arrays"""
    import lmono_amd
    batch = [K.empty_window(), K.mixed_window(), K.empty_window(), K.hostile_window(False), K.plain_window(41, 40), K.empty_window()]
    W, feat_off, Rs, Ps, tlc, start, obs_off, pts = lmono_amd.Context._pack_windows(batch)
    p = K.pack(batch)
    assert p["W"] == W
    for name, a in (("feat_off", feat_off), ("Rs", Rs), ("Ps", Ps), ("tlc", tlc), ("start", start), ("obs_off", obs_off), ("pts", pts)):
        assert p[name].dtype == a.dtype and p[name].shape == a.shape and p[name].tobytes() == a.tobytes(), name
