"""ESTIMATE_LASER == 2 in the host mirror's frame loop (lmono_amd/host: Estimator::processImage -> getCorresponding -> AXXBSolver over
lmono_excalib_step; Estimator.cc:403-430): a hand-held S7 stream calibrates on frame 10, initialises on that frame from the
calibrated extrinsic and goes on exactly as a run that was given that extrinsic from the start; a yaw-only stream never calibrates."""
import os
import subprocess

import numpy as np
import pytest

from tests import excalib_cases as C
from tests import excalib_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmono_amd", "host", "estimator_seq")
pytestmark = pytest.mark.gpu


def _run(st, tmp_path, name, *args):
    from workloads import s2
    fx = tmp_path / (name + ".bin")
    s2.write_stream(fx, st)
    out = subprocess.run([EXE, str(fx), "-"] + list(args), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    return ([ln for ln in lines if ln.startswith("FRM")], [ln for ln in lines if ln.startswith("ODO")], [ln for ln in lines if ln.startswith("CAL")])


@pytest.fixture(scope="module")
def handheld():
    from workloads import s7
    return s7.make_stream(25, seed=0, angle_deg=(8.0, 12.0))


def _lidar_increments(st):
    """q_lidar of frame k >= 1 as the mirror forms it: Quaterniond(R_{k-1}^T R_k), x y z w."""
    return [None] + [np.array(X.m2q(X.mul33(st["L0"][k - 1][:3, :3].T, st["L0"][k][:3, :3]))) for k in range(1, len(st["L0"]))]


def test_handheld_stream_calibrates_and_initialises(gpu_ctx, handheld, tmp_path):
    import lmono_amd
    from workloads import s7
    st = handheld
    frm, odo, cal = _run(st, tmp_path, "s7", "estimate_laser=2")
    assert len(frm) == 25 and len(cal) == 1
    w = cal[0].split()
    assert int(w[1]) == 10
    rlc = np.array([float(v) for v in w[2:11]])
    # the restatement on the same pairs: success on frame 10, and whether every Huber weight was 1
    ql = _lidar_increments(st)
    ref = X.Calibrator(10)
    dev = lmono_amd.ExtrinsicCalibrator(gpu_ctx, 1, 10)
    all_one = True
    for k in range(1, 11):
        P = s7.frame_pairs(st, k)
        assert 9 <= len(P) <= 512
        r = ref.step(P, ql[k])
        assert abs(ref.info["deg"] - 5.0) > 1e-6
        all_one = all_one and r[4] == 1.0
        got = dev.step([P], [ql[k]])
        assert bool(got["ok"][0]) == r[5] == (k == 10), k
    assert abs(r[3][2] - 0.25) > 1e-3
    # both sides ran on the device, so bytes whether or not a Huber weight was below 1; against the restatement, which says which
    # weights were, bytes where all were 1 and 1e-9 behind a healthy eigen gap otherwise
    assert got["rlc"][0].tobytes() == rlc.tobytes()
    if all_one:
        assert r[2].tobytes() == rlc.tobytes()
    else:
        assert ref.info["eig"][1] - ref.info["eig"][0] >= 1e-3
        assert np.abs(r[2] - rlc).max() <= 1e-9
    dev.close()
    assert C.angle_between(rlc.reshape(3, 3), st["tlc_true"][:3, :3]) < 1e-6
    # INITED on that frame, odometry rows from it on
    stage = [int(ln.split()[3]) for ln in frm]
    assert stage == [0] * 10 + [1] * 15 and len(odo) == 15

    # consistency: a run that is given the calibrated rotation from the start (ESTIMATE_LASER = 1) prints the same frames and trajectory
    st2 = dict(st)
    st2["tlc"] = st["tlc"].copy(); st2["tlc"][:3, :3] = rlc.reshape(3, 3)
    frm2, odo2, cal2 = _run(st2, tmp_path, "s7_given", "estimate_laser=1")
    assert cal2 == [] and frm2 == frm and odo2 == odo


def test_yaw_only_stream_never_calibrates(tmp_path):
    from workloads import s7
    st = s7.make_stream(25, seed=1, angle_deg=(8.0, 12.0), yaw_only=True)
    frm, odo, cal = _run(st, tmp_path, "s7_yaw", "estimate_laser=2")
    assert len(frm) == 25 and cal == [] and odo == []
    assert all(int(ln.split()[3]) == 0 for ln in frm)
