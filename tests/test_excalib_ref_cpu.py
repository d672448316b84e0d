"""The restatement of the camera-LiDAR rotation calibration (tests/excalib_ref.py) against numpy.linalg and the truth,
and the host build of the kernel's arithmetic (lmono_amd/host/excalib_test) against the restatement, byte for byte.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import excalib_cases as C
from tests import excalib_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lmono_amd", "host")
TEST_BIN = os.path.join(HOST, "excalib_test")


def run_sequence(frames, count=10, check=True):
    """frames of C.scene -> per frame dict of the restatement's outputs; asserts the scene's preconditions on the way."""
    cal = X.Calibrator(count)
    out = []
    for P, Rc, ql in frames:
        info = {}
        R, stats, rlc, sv, huber, ok = cal.step(P, ql, info)
        if check:
            assert abs(cal.info["deg"] - 5.0) > 1e-6, "an angular distance within 1e-6 degrees of 5: choose another seed"
            if cal.frame_count >= count:
                assert abs(sv[2] - 0.25) > 1e-3, "sv[2] within 1e-3 of 0.25 on a deciding frame: choose another seed"
        out.append(dict(R=R, stats=stats, rlc=rlc, sv=sv, huber=huber, ok=ok, state=cal.state(), eig=cal.info["eig"], deg=cal.info["deg"], Rc=Rc))
    return out


@pytest.mark.parametrize("m", [9, 64, 150])
def test_noise_free_scene_against_truth(m):
    res = run_sequence(C.scene(1, m, 12, 8.0, 12.0))
    for k, r in enumerate(res):
        assert r["stats"][0] == m and r["stats"][5] in (0, 1)
        assert max(r["stats"][1:5]) == m                      # every point in front of both cameras for the winner
        assert C.angle_between(r["R"].reshape(3, 3), r["Rc"]) < 1e-8, (k, C.angle_between(r["R"].reshape(3, 3), r["Rc"]))
        if k >= 2:                                            # from the third frame on the null space is a line
            assert r["eig"][1] - r["eig"][0] >= 1e-3
            assert C.angle_between(r["rlc"].reshape(3, 3), C.RLC_TRUE) < 1e-7, (k, C.angle_between(r["rlc"].reshape(3, 3), C.RLC_TRUE))
    # 8-12 degrees per frame about changing axes: success on frame 10 exactly
    assert [r["ok"] for r in res] == [False] * 9 + [True] * 3


def test_against_numpy_linalg():
    """The Jacobi answers against LAPACK on the same matrices: the essential matrix's null vector, and the stage-4 eigenpairs."""
    frames = C.scene(2, 64, 6, 8.0, 12.0)
    cal = X.Calibrator(10)
    for P, Rc, ql in frames:
        E = X.essential(P).reshape(3, 3)
        s = np.linalg.svd(E, compute_uv=False)
        assert s[2] / s[0] < 1e-14                         # rank 2 after the deflation
        assert abs(s[0] - s[1]) / s[0] < 1e-9              # noise-free: an essential matrix
        resid = np.abs(np.einsum("ki,ij,kj->k", np.column_stack([P[:, 2:], np.ones(len(P))]), E, np.column_stack([P[:, :2], np.ones(len(P))])))
        assert resid.max() / s[0] < 1e-12                  # cur^T E prev = 0
        cal.step(P, ql)
        w, v = np.linalg.eigh(cal.M)
        assert np.abs(cal.info["eig"] - w).max() < 1e-12
        if w[1] - w[0] >= 1e-3:
            assert 1.0 - abs(float(cal.info["x"] @ v[:, 0])) < 1e-12


def test_yaw_only_never_succeeds():
    res = run_sequence(C.scene(3, 64, 30, 8.0, 12.0, yaw_only=True))
    assert not any(r["ok"] for r in res)
    assert max(r["sv"][2] for r in res) < 1e-6             # one rotation axis: the null space keeps two dimensions


FIRST_SLOW = 38         # of this seed (a LAPACK prototype of the pipeline on another seed: 36)


def test_slow_rotation_succeeds_late():
    """2-4.5 degrees per frame: the third singular value grows slowly, success comes long after frame 10."""
    pairs = C.rotation_pairs(4, 60, 2.0, 4.5)
    cal = X.Calibrator(10)
    oks = [cal.push(qc, ql)[3] for qc, ql in pairs]
    first = oks.index(True) + 1
    assert first == FIRST_SLOW and all(oks[first - 1:])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pixel_noise_within_one_degree(seed):
    res = run_sequence(C.scene(10 + seed, 150, 14, 8.0, 12.0, noise_px=0.5))
    first = [r["ok"] for r in res].index(True)
    assert first == 9
    err = np.rad2deg(C.angle_between(res[first]["rlc"].reshape(3, 3), C.RLC_TRUE))
    assert err < 1.0, err


def test_running_sum_equals_rebuilt_matrix():
    """Observation A: the 4 x 4 running sum against the reference's rebuilt 4k x 4 matrix, Huber weights below 1 included."""
    pairs = C.rotation_pairs(5, 14, outlier_at=3)
    cal = X.Calibrator(10)
    hubers = []
    for qc, ql in pairs:
        rlc, sv, huber, ok = cal.push(qc, ql)
        hubers.append(huber)
        A = np.vstack(cal.blocks)
        _, s, vt = np.linalg.svd(A)
        assert np.abs(np.sort(s * s) - cal.info["eig"]).max() < 1e-12
        if cal.info["eig"][1] - cal.info["eig"][0] >= 1e-3:
            assert np.abs(np.abs(cal.info["x"]) - np.abs(vt[3])).max() < 1e-12
    assert min(hubers) < 1.0


def _host_sequences():
    """The cases of tests/test_excalib_gpu.py as excalib_test sequences: (count, frames), whether stage 4 is comparable by bytes."""
    seqs = []
    for m in (8, 9, 10, 64, 65, 150, 512):
        P = C.scene(20 + m, m, 1, 3.0, 6.0)[0][0]
        seqs.append((10, [(0, P, None, None)], True))
    for P in C.degenerate_cases().values():
        seqs.append((10, [(0, P, None, None)], True))
    seqs.append((10, [(1, P, None, ql) for P, _, ql in C.scene(30, (40, 64, 150), 14, 0.5, 2.4)], True))
    seqs.append((10, [(1, P, None, ql) for P, _, ql in C.scene(1, 64, 12, 8.0, 12.0)], False))
    seqs.append((10, [(2, np.zeros((0, 4)), qc, ql) for qc, ql in C.rotation_pairs(5, 14, outlier_at=3)], False))
    seqs.append((10, [(2, np.zeros((0, 4)), qc, ql) for qc, ql in C.rotation_pairs(14, 14, outlier_at=3, small_first=3)], False))
    for n in (1, 3, 70):        # the batches of the GPU test
        for frames in C.batch_scenes(n):
            seqs.append((2, [(1, P, None, ql) for P, _, ql in frames], False))
    seqs.append((10, [(1, P, None, ql) for P, _, ql in C.scene(40, 30, 3, 4.0, 9.0)], False))       # its error-return test
    from workloads import s7    # the estimator test's stream, as the mirror feeds it
    st = s7.make_stream(25, seed=0, angle_deg=(8.0, 12.0))
    seqs.append((10, [(1, s7.frame_pairs(st, k), None, np.array(X.m2q(X.mul33(st["L0"][k - 1][:3, :3].T, st["L0"][k][:3, :3])))) for k in range(1, 11)], False))
    return seqs


def test_host_arithmetic_equals_restatement(tmp_path):
    if not os.path.exists(TEST_BIN):
        subprocess.check_call(["make", "-s", "-C", HOST, "excalib_test"])
    seqs = _host_sequences()
    path = tmp_path / "cases.bin"
    C.write_cases(path, [(c, f) for c, f, _ in seqs])
    got = C.parse_results(subprocess.run([TEST_BIN, str(path)], check=True, capture_output=True, text=True).stdout)
    at = 0
    n_cal_bytes = 0
    for count, frames, by_bytes in seqs:
        cal = X.Calibrator(count)
        all_one = True
        for kind, P, qc, ql in frames:
            if kind != 2:
                R, stats = X.relative_rotation(P)
                g = got[at]; at += 1
                assert g[0] == "REL" and g[1].tobytes() == R.tobytes() and (g[2] == stats).all(), (kind, len(P), g, R, stats)
                qc = X.m2q(R.reshape(3, 3))
            if kind != 0:
                rlc, sv, huber, ok = cal.push(qc, ql)
                g = got[at]; at += 1
                all_one = all_one and huber == 1.0
                assert g[0] == "CAL" and g[4] == ok and g[5] == cal.frame_count
                # bytes also where a weight is below 1: the host program's atan2 and math.atan2 are the same libm function, so no
                # tolerance (and with it no eigen-gap precondition) is needed on this side; the device's atan2 is the GPU test's matter
                assert g[1].tobytes() == rlc.tobytes() and g[2].tobytes() == sv.tobytes() and g[3] == huber and g[6].tobytes() == cal.M.tobytes()
                n_cal_bytes += 1 if all_one else 0
        if by_bytes:
            assert all_one, "a sequence meant to have every Huber weight 1 has one below"
    assert at == len(got) and n_cal_bytes >= 14
