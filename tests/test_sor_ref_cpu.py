"""The statistical outlier removal without a GPU: (a) the host program lmono_amd/host/sor_test -- the header the kernels
include, by brute force -- equals the numpy restatement byte for byte, (b) the restatement against PCL's formulas in float64 (k-d tree,
mean of the k nearest distances, sample standard deviation), (c) the filter does its job on two walls with flying points between them,
(d) the result does not depend on the order of the input."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import sor_ref as R
from tests import voxel_map_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")
CELL, RINGS = 0.2, 4                                                              # rho = 3.75 * 0.2 = 0.75 m


@functools.lru_cache(maxsize=None)
def _walls(seed):
    return R.walls(seed)


@functools.lru_cache(maxsize=None)
def _run(seed, k, mul=1.0):
    return R.run(_walls(seed)[0], k, mul, CELL, RINGS)


def _host_text(tmp_path, p, k, mul, cell, rings):
    subprocess.check_call(["make", "-s", "-C", HOST, "sor_test"])
    path = str(tmp_path / "points.bin")
    p.tofile(path)
    return subprocess.check_output([os.path.join(HOST, "sor_test"), path, str(k), repr(float(mul)), repr(float(cell)), str(rings)], text=True)


def _mixed():
    """Walls with rejected points, duplicates and a far pair mixed in."""
    p = _walls(3)[0][:900].copy()
    p = np.concatenate([p[:300], R.rejected_points(CELL), p[300:], p[10:40], VR.points([[500.0, 500.0, 500.0], [500.05, 500.0, 500.0]], [1, 2])])
    return p


@pytest.mark.parametrize("k,mul", [(1, 1.0), (8, 0.0), (16, -0.5), (128, 2.0)])
def test_host_program_equals_the_restatement(tmp_path, k, mul):
    p = _mixed()
    r = R.run(p, k, mul, CELL, RINGS)
    assert r.stats[1] == len(R.rejected_points(CELL)) and r.stats[2] >= 2           # the far pair is isolated for every k here but 1
    assert _host_text(tmp_path, p, k, mul, CELL, RINGS) == R.text(r)


def test_host_program_on_the_smallest_inputs(tmp_path):
    one = VR.points([[1.0, 2.0, 3.0]], [7])
    for p, k in ((one[:0], 1), (one, 1), (np.concatenate([one] * 5), 4), (np.concatenate([one] * 4), 4)):
        r = R.run(p, k, 1.0, 0.1, 8)
        assert _host_text(tmp_path, p, k, 1.0, 0.1, 8) == R.text(r)
    r = R.run(np.concatenate([one] * 5), 4, 1.0, 0.1, 8)
    assert r.stats.tolist() == [5, 0, 0, 5, 5, 0, 0, 0] and r.thr == 0.0          # identical points: v = 0, var = 0, all kept
    assert R.run(np.concatenate([one] * 4), 4, 1.0, 0.1, 8).stats.tolist() == [4, 0, 4, 0, 0, 0, 0, 0]


def _pcl_float64(p, k, mul, rho):
    """PCL's formulas in float64 over a k-d tree: mean distance to the k nearest, isolated iff the k-th lies beyond rho."""
    from scipy.spatial import cKDTree
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
    d, _ = cKDTree(xyz).query(xyz, k + 1)
    assert (d[:, 0] == 0.0).all()
    d = d[:, 1:]
    isolated = d[:, -1] > rho
    m = d.mean(1)
    ms = m[~isolated]
    thr = ms.mean() + mul * ms.std(ddof=1)
    return m, isolated, thr, d[:, -1]


@pytest.mark.parametrize("k", [8, 16, 50])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_restatement_against_pcl_formulas_in_float64(seed, k):
    p, _ = _walls(seed)
    r = _run(seed, k)
    rho = float(R.rho_of(CELL, RINGS))
    assert rho == 0.75 and len(p) == 2750 and r.stats[1] == 0
    m_ref, iso_ref, thr_ref, kth = _pcl_float64(p, k, 1.0, rho)
    # conditions on the input, from the reference alone
    assert (np.abs(kth - rho) > 2.0 ** -20 * rho).all()
    delta = 2.0 ** -15 / k + 2.0 ** -20 * thr_ref
    borderline = ~iso_ref & (np.abs(m_ref - thr_ref) <= delta)
    assert borderline.sum() <= 0.005 * len(p)
    # the restatement
    iso = (r.v == R.NO_SCORE)
    assert (iso == iso_ref).all()
    m = r.v[~iso].astype(np.float64) / 65536.0 / k
    assert np.abs(m - m_ref[~iso]).max() <= 2.0 ** -16 / k + 2.0 ** -20 * m_ref[~iso].max()
    keep_ref = ~iso_ref & ~(m_ref > thr_ref)
    assert (r.keep.astype(bool) == keep_ref)[~borderline].all()
    assert abs(r.thr / 65536.0 / k - thr_ref) <= delta


def test_the_filter_removes_flying_points_and_keeps_the_walls():
    """k = 16, multiplier 1.0, seed 0.  The restatement's own run printed: flying removed 120 of 120, wall points removed 12 of 2600
    (0.5 %), far points removed 30 of 30."""
    p, label = _walls(0)
    r = _run(0, 16)
    removed = r.keep == 0
    fly, wall = removed[label == 2].mean(), removed[label < 2].mean()
    print("flying removed %d of %d, wall removed %d of %d, far removed %d of %d" % (removed[label == 2].sum(), (label == 2).sum(), removed[label < 2].sum(),
                                                                                      (label < 2).sum(), removed[label == 3].sum(), (label == 3).sum()))
    assert fly > 0.5 and wall < 0.15
    assert removed[label == 3].all()


def test_order_free():
    p, _ = _walls(1)
    p = np.concatenate([p[:700], R.rejected_points(CELL)])
    perm = np.random.default_rng(9).permutation(len(p))
    a, b = R.run(p, 16, 1.0, CELL, RINGS), R.run(p[perm], 16, 1.0, CELL, RINGS)
    assert a.stats.tobytes() == b.stats.tobytes()
    assert np.array([a.mean, a.sd, a.thr]).tobytes() == np.array([b.mean, b.sd, b.thr]).tobytes()
    assert (a.keep[perm] == b.keep).all() and (a.v[perm] == b.v).all()
    assert b.cloud.tobytes() == p[perm][b.keep.astype(bool)].tobytes()
