"""The cases of the sample-consensus alignment tests: name -> (source FPFH case, target FPFH case, keypoints kept on the source (None:
all), keypoints kept on the target, keyword arguments of sacia_ref.run / CoarseAligner).  The descriptors are those of the FPFH restatement on the
scenes of tests/fpfh_cases.py, which the device gives as bytes (tests/test_fpfh_gpu.py).  Source `scene`, target `scene_rigid`: the known transform
is (fpfh_cases.SCENE_R, SCENE_T), 40 degrees and 1 m.  Shared by the CPU test and the GPU test."""
import functools

import numpy as np

from tests import fpfh_cases as FC
from tests import fpfh_ref as FR
from tests import normals_ref as NR

KW = dict(min_sample_dist=0.5, max_corr=1.0, k_corr=10, n_hyp=64, seed=1)

CASES = {
    "rigid_k1": ("scene", "scene_rigid", None, None, dict(KW, k_corr=1)),
    "rigid_k3": ("scene", "scene_rigid", None, None, dict(KW, k_corr=3)),
    "rigid_k10": ("scene", "scene_rigid", None, None, KW),
    "rigid_seed2": ("scene", "scene_rigid", None, None, dict(KW, seed=2)),
    "one_hypothesis": ("scene", "scene_rigid", None, None, dict(KW, n_hyp=1)),
    "all_void": ("scene", "scene_rigid", None, None, dict(KW, min_sample_dist=100.0)),
    "tied": ("scene", "scene_rigid", (5, 50, 90), (5, 20, 50, 70, 90), dict(KW, k_corr=1, min_sample_dist=0.25)),
    "three_usable": ("scene", "scene_rigid", (5, 50, 90), (5, 50, 90), dict(KW, k_corr=10, min_sample_dist=0.25)),
    "two_usable": ("scene", "scene_rigid", (5, 50), None, KW),
    "resampled": ("scene", "scene_resampled", None, None, dict(KW, max_corr=0.3, n_hyp=256)),
}


def keypoints_of(name, keep):
    """The keypoints of a case of tests/fpfh_cases.py; with `keep`, every other one is moved 500 m away, where it has no neighbour and so no
    descriptor (flag 0): it takes no part.  The kept ones' descriptors do not change."""
    k = FC.CASES[name]()[2].copy()
    if keep is not None:
        away = np.ones(len(k), bool)
        away[list(keep)] = False
        k[away] += np.float32(500.0)
    return k


@functools.lru_cache(maxsize=None)
def normals_of(name):
    p, nkw, _, _ = FC.CASES[name]()
    return p, nkw, NR.run(p, **nkw)


@functools.lru_cache(maxsize=None)
def fpfh_of(name, keep=None):
    """(points, normals keywords, keypoints, FPFH keywords, the restatement's result)."""
    p, nkw, nr = normals_of(name)
    fkw = FC.CASES[name]()[3]
    k = keypoints_of(name, keep)
    return p, nkw, k, fkw, FR.run(p, nr.records, k, **fkw)


@functools.lru_cache(maxsize=None)
def sides(name):
    """(source keypoints, descriptors, flags, target keypoints, descriptors, flags) of a case."""
    s, t, ks, kt, _ = CASES[name]
    a, b = fpfh_of(s, ks), fpfh_of(t, kt)
    return a[2], a[4].desc, a[4].flags, b[2], b[4].desc, b[4].flags
