"""The sample-consensus initial alignment without a GPU: (a) the host program lmono_amd/host/sacia_test -- the header the
kernels include, by brute force -- prints the numpy restatement's words on every case of tests/sacia_cases.py, (b) each case is what it claims
to be, (c) the candidates are the exact k nearest with ties to the lowest index, (d) on the rigid copy every hypothesis that is not void recovers
the transform at k_corr = 1 and the best of 16384 is an exact one at k_corr = 10, (e) on the differently sampled source the ICP restatement
started from the coarse transform ends where it ends when started from the known transform, and started from the identity it does not.

Measured on the restatement (the figures of DESIGN.md 6c-8):
  rigid copy, k_corr = 1, 256 hypotheses, none void: largest error 0.0518 degrees, 0.00155 m; asserted at 4 x that.
  resampled source (114 target keypoints, 85 % crop, other jitter), max_corr = 1.0: coarse error 8.67 degrees, 0.418 m at n_hyp = 1024 and
  2.58 degrees, 0.224 m at 16384.  The ICP (max_corr 0.25, 50 iterations) from the known transform settles 0.1256 degrees, 0.00790 m from it (its
  converged residual: the crop and the jitter); from the 16384-hypothesis coarse transform it ends 0.1256 degrees, 0.00790 m away, from the
  identity 41.6 degrees, 0.93 m.  Asserted: within 2 x the converged residual from the coarse start, outside it from the identity.
  From the 1024-hypothesis coarse transform the same ICP ends 1.47 degrees, 0.118 m away: recorded, not asserted."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import fpfh_cases as FC
from tests import icp_ref as IR
from tests import sacia_cases as SC
from tests import sacia_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")

MEASURED_K1_MAX = (0.0518, 0.00155)         # degrees, m: the largest error of a hypothesis at k_corr = 1 on the rigid copy
ICP_KW = dict(max_corr=0.25, max_iter=50)   # the fine stage of the resampled test: twice the scene's 0.125 m spacing, above the coarse error of 0.22 m


@functools.lru_cache(maxsize=None)
def ref(name, **more):
    return R.run(*SC.sides(name), **dict(SC.CASES[name][4], **more))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_program_prints_the_restatements_words(tmp_path, name):
    subprocess.check_call(["make", "-s", "-C", HOST, "sacia_test"])
    paths = []
    for i, a in enumerate(SC.sides(name)):
        paths.append(str(tmp_path / ("%d.bin" % i)))
        np.ascontiguousarray(a).tofile(paths[-1])
    kw = SC.CASES[name][4]
    pr = subprocess.run([os.path.join(HOST, "sacia_test")] + paths + [repr(kw["min_sample_dist"]), repr(kw["max_corr"]), str(kw["k_corr"]), str(kw["n_hyp"]), str(kw["seed"])],
                        text=True, capture_output=True)
    r = ref(name)
    if r is None:
        assert pr.returncode == 3
    else:
        assert pr.returncode == 0 and [ln for ln in pr.stdout.split("\n") if ln] == R.text(r)


def test_the_cases_are_what_they_claim():
    sk, sd, sf, tk, td, tf = SC.sides("rigid_k1")
    assert sf.all() and tf.all() and len(sk) == len(tk) == 108
    assert np.abs(sk.astype(np.float64) @ FC.SCENE_R.T + FC.SCENE_T - tk).max() < 1e-6        # the target keypoints are the moved source keypoints
    for name, k in (("rigid_k1", 1), ("rigid_k3", 3), ("rigid_k10", 10)):
        r = ref(name)
        assert r.cand.shape == (108, k) and r.ok and r.voids == 0 and (r.err != R.VOID).all()
    assert ref("rigid_k10").err.tobytes() != ref("rigid_seed2").err.tobytes()                  # two seeds differ
    one = ref("one_hypothesis")
    assert len(one.err) == 1 and one.h == 0 and one.err[0] == ref("rigid_k10").err[0]
    void = ref("all_void")
    assert void.ok == 0 and void.h == -1 and void.T is None and void.voids == 64 and (void.err == R.VOID).all() and not void.inl.any()
    tied = ref("tied")
    assert tied.stats[5] == 3 and tied.stats[6] == 5 and tied.valid.any()
    assert len(set(tied.err[tied.valid].tolist())) == 1 and tied.h == int(np.flatnonzero(tied.valid)[0])     # every valid hypothesis ties: the lowest h wins
    assert len({tuple(sorted(i)) for i in tied.idx[tied.valid].tolist()}) == 1 and len({tuple(i) for i in tied.idx[tied.valid].tolist()}) > 1
    three = ref("three_usable")
    assert three.stats[5] == 3 and three.stats[6] == 3 and three.ok and three.cand.shape == (3, 3)         # k_corr above nt: K = nt
    assert ref("two_usable") is None
    res = SC.sides("resampled")
    assert len(res[3]) == 114 and res[5].all()


def test_the_candidates_are_the_exact_nearest_with_ties_to_the_lowest_index():
    r = ref("rigid_k10")
    D = r.D.astype(np.float64)
    for i in range(len(D)):
        want = sorted(range(D.shape[1]), key=lambda j: (D[i, j], j))[:10]
        assert r.cand[i].tolist() == want
    # tied distances: a target whose descriptors repeat
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 100, (5, 33)).astype(np.float32)
    b = np.repeat(rng.uniform(0, 100, (4, 33)).astype(np.float32), 3, 0)[rng.permutation(12)]
    cand, D = R.candidates(a, b, 7)
    for i in range(5):
        assert cand[i].tolist() == sorted(range(12), key=lambda j: (float(D[i, j]), j))[:7]
        assert (np.diff(D[i, cand[i]]) == 0).sum() >= 4
    # the distance: 33 float32 terms in index order
    s = np.float32(0)
    for k in range(33):
        d = np.float32(a[0, k] - b[0, k]); s = np.float32(s + np.float32(d * d))
    assert D[0, 0] == s


def test_the_samples_are_distinct_and_apart():
    r = ref("rigid_k10")
    u = SC.sides("rigid_k10")[0]
    for i in r.idx[r.valid]:
        assert len(set(i.tolist())) == 3
        for a in range(3):
            for b in range(a):
                assert ((u[i[a]] - u[i[b]]).astype(np.float64) ** 2).sum() >= 0.25 - 1e-6
    assert (ref("all_void").valid == 0).all()


def test_recovery_on_the_rigid_copy():
    # every source keypoint's nearest descriptor is its true partner
    r = ref("rigid_k1", n_hyp=256)
    assert (r.cand[:, 0] == np.arange(108)).all()
    pe = np.array([R.pose_error(R.transform_of(r, h), FC.SCENE_R, FC.SCENE_T) for h in sorted(r.fits)])
    print("k_corr = 1: %d hypotheses, largest error %.6f degrees, %.6f m" % (len(pe), pe[:, 0].max(), pe[:, 1].max()))
    assert len(pe) == 256 and r.voids == 0
    assert pe[:, 0].max() <= 4.0 * MEASURED_K1_MAX[0] and pe[:, 1].max() <= 4.0 * MEASURED_K1_MAX[1]
    # k_corr = 10, 16384 hypotheses at min_sample_dist 0.5: the best one drew three true partners
    r = ref("rigid_k10", n_hyp=16384)
    e = R.pose_error(r.T, FC.SCENE_R, FC.SCENE_T)
    print("k_corr = 10: winner %d, error %.6f degrees, %.6f m" % (r.h, *e))
    assert r.ok and (r.tj[r.h] == r.idx[r.h]).all()
    assert e[0] <= 4.0 * MEASURED_K1_MAX[0] and e[1] <= 4.0 * MEASURED_K1_MAX[1]


def test_the_differently_sampled_source_then_the_icp():
    ps, pt = SC.fpfh_of("scene")[0], SC.fpfh_of("scene_resampled")[0]
    true = np.concatenate([FC.SCENE_R, FC.SCENE_T[:, None]], 1).reshape(-1)
    settled = R.pose_error(IR.run(pt, ps, guess=true, **ICP_KW).transform, FC.SCENE_R, FC.SCENE_T)        # the ICP's own converged residual
    print("icp from the known transform: %.4f degrees, %.5f m" % settled)
    for n in (1024, 16384):
        c = ref("resampled", max_corr=1.0, n_hyp=n)
        e = R.pose_error(c.T, FC.SCENE_R, FC.SCENE_T)
        f = R.pose_error(IR.run(pt, ps, guess=c.T, **ICP_KW).transform, FC.SCENE_R, FC.SCENE_T)
        print("n_hyp %d: coarse %.3f degrees, %.4f m; icp from it %.4f degrees, %.5f m" % (n, *e, *f))
    assert f[0] <= 2.0 * settled[0] and f[1] <= 2.0 * settled[1]                                          # from the 16384-hypothesis coarse transform
    i = R.pose_error(IR.run(pt, ps, **ICP_KW).transform, FC.SCENE_R, FC.SCENE_T)
    print("icp from the identity: %.3f degrees, %.4f m" % i)
    assert i[0] > 2.0 * settled[0] and i[1] > 2.0 * settled[1]
