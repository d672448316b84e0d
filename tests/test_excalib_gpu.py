"""The camera-LiDAR rotation calibration on the device (lmono_relative_rotation, lmono_excalib_*) against the CPU
restatement tests/excalib_ref.py: equal bytes wherever every Huber weight is 1, 1e-9 behind the device's atan2 where one is below."""
import numpy as np
import pytest

from tests import excalib_cases as C
from tests import excalib_ref as X

pytestmark = pytest.mark.gpu


def _error_code(exc):
    return int(str(exc.value).split("lmono error ")[1].split(":")[0])


def _same_state(got, ref):
    return got[0] == ref[0] and got[1].tobytes() == ref[1].tobytes() and got[2].tobytes() == ref[2].tobytes()


@pytest.mark.parametrize("m", [8, 9, 10, 64, 65, 150, 512])
def test_relative_rotation_equals_restatement(gpu_ctx, m):
    import lmono_amd
    P, Rc, _ = C.scene(20 + m, m, 1, 3.0, 6.0)[0]
    R, stats = lmono_amd.relative_rotation(gpu_ctx, [P])
    rR, rstats = X.relative_rotation(P)
    assert stats[0].tolist() == rstats.tolist(), (stats, rstats)
    assert R[0].tobytes() == rR.tobytes()
    if m == 8:
        assert stats[0].tolist() == [8, 0, 0, 0, 0, -1] and (R[0] == np.eye(3)).all()      # fewer than 9 pairs: the identity by rule
    else:
        assert C.angle_between(R[0], Rc) < 1e-8


def test_relative_rotation_degenerate_inputs(gpu_ctx):
    import lmono_amd
    cases = C.degenerate_cases()
    names = sorted(cases)
    R, stats = lmono_amd.relative_rotation(gpu_ctx, [cases[k] for k in names])      # one launch
    for i, k in enumerate(names):
        rR, rstats = X.relative_rotation(cases[k])
        assert stats[i].tolist() == rstats.tolist(), (k, stats[i], rstats)
        assert R[i].tobytes() == rR.tobytes(), k
        assert np.isfinite(R[i]).all(), k
    i = names.index("one_nan")
    assert stats[i][0] == len(cases["one_nan"]) - 1
    assert stats[names.index("empty")].tolist() == [0, 0, 0, 0, 0, -1]
    assert stats[names.index("identical")][5] == -1


def test_full_sequence_equals_restatement(gpu_ctx):
    """14 frames of rotations below 2.5 degrees: every Huber weight is exactly 1 whatever rlc is, so everything is bytes."""
    import lmono_amd
    frames = C.scene(30, (40, 64, 150), 14, 0.5, 2.4)
    cal = lmono_amd.ExtrinsicCalibrator(gpu_ctx, 1, 10)
    ref = X.Calibrator(10)
    for k, (P, Rc, ql) in enumerate(frames):
        got = cal.step([P], [ql])
        R, stats, rlc, sv, huber, ok = ref.step(P, ql)
        assert huber == 1.0 and abs(ref.info["deg"] - 5.0) > 1e-6
        assert got["stats"][0].tolist() == stats.tolist(), k
        assert got["R_cam"][0].tobytes() == R.tobytes(), k
        assert got["rlc"][0].tobytes() == rlc.tobytes(), k           # frame 1 included: a two-dimensional null space, the same vector of it
        assert got["sv"][0].tobytes() == sv.tobytes(), k
        assert got["huber"][0] == 1.0 and bool(got["ok"][0]) == ok, k
        assert _same_state(cal.state(0), (ref.frame_count, ref.M, ref.rlc)), k
    cal.close()


def test_huber_below_one(gpu_ctx):
    """Three frames of small turns (weights exactly 1: bytes), then 8-12 degrees with the camera rotation of frame 4 off by 20 degrees."""
    import lmono_amd
    pairs = C.rotation_pairs(14, 14, outlier_at=3, small_first=3)
    cal = lmono_amd.ExtrinsicCalibrator(gpu_ctx, 1, 10)
    ref = X.Calibrator(10)
    oks = []
    for k, (qc, ql) in enumerate(pairs):
        got = cal.push([qc], [ql])
        rlc, sv, huber, ok = ref.push(qc, ql)
        assert abs(ref.info["deg"] - 5.0) > 1e-6, "an angular distance within 1e-6 degrees of 5: choose another seed"
        if ref.frame_count >= 10:
            assert abs(sv[2] - 0.25) > 1e-3, "sv[2] within 1e-3 of 0.25 on a deciding frame: choose another seed"
        fc, M, r = cal.state(0)
        assert fc == ref.frame_count and bool(got["ok"][0]) == ok
        assert (got["huber"][0] < 1.0) == (huber < 1.0)                 # the 5 degree decision
        if k < 3:
            assert huber == 1.0
            assert got["rlc"][0].tobytes() == rlc.tobytes() and got["sv"][0].tobytes() == sv.tobytes() and M.tobytes() == ref.M.tobytes(), k
        else:
            assert ref.info["eig"][1] - ref.info["eig"][0] >= 1e-3, "eigen gap below 1e-3 where a tolerance is used: choose another seed"
            assert abs(got["huber"][0] - huber) <= 1e-9
            assert np.abs(got["rlc"][0].reshape(9) - rlc).max() <= 1e-9, k
            assert np.abs(got["sv"][0] - sv).max() <= 1e-9 and np.abs(M - ref.M).max() <= 1e-9 and np.abs(r.reshape(9) - rlc).max() <= 1e-9, k
        if k == 3:
            assert huber < 1.0 and got["huber"][0] < 1.0
        oks.append(ok)
    assert any(oks)
    cal.close()


@pytest.mark.parametrize("n", [1, 3, 70])
def test_batch_equals_one_stream_handles(gpu_ctx, n):
    import lmono_amd
    rng = np.random.default_rng(400 + n)
    n_frames = 3
    seqs = C.batch_scenes(n, n_frames)
    batch = lmono_amd.ExtrinsicCalibrator(gpu_ctx, n, 2)
    single = lmono_amd.ExtrinsicCalibrator(gpu_ctx, 1, 2)
    want = []
    for s in range(n):
        single.reset()
        want.append([(single.step([P], [ql]), single.state(0)) for P, _, ql in seqs[s]])
    for k in range(n_frames):
        order = rng.permutation(n)
        got = batch.step([seqs[s][k][0] for s in order], [seqs[s][k][2] for s in order], streams=order)
        for i, s in enumerate(order):
            w, wstate = want[s][k]
            for key in ("R_cam", "stats", "rlc", "sv", "huber", "ok"):
                assert got[key][i].tobytes() == w[key][0].tobytes(), (n, k, s, key)
            assert _same_state(batch.state(int(s)), wstate), (n, k, s)
    if n > 1:
        before = [batch.state(s) for s in range(n)]
        batch.reset(1)
        fc, M, rlc = batch.state(1)
        assert fc == 0 and (M == 0).all() and (rlc == np.eye(3)).all()
        for s in range(n):
            if s != 1:
                assert _same_state(batch.state(s), before[s]), s
    batch.close(); single.close()


def test_error_returns_change_nothing(gpu_ctx):
    import lmono_amd
    frames = C.scene(40, 30, 3, 4.0, 9.0)
    cal = lmono_amd.ExtrinsicCalibrator(gpu_ctx, 2, 10)
    P0, _, q0 = frames[0]
    cal.step([P0, P0], [q0, q0])
    before = [cal.state(0), cal.state(1)]
    big = np.zeros((513, 4))
    nanq = np.array([0.0, np.nan, 0.0, 1.0])

    def refused(code, fn):
        with pytest.raises(lmono_amd.LmonoError) as e:
            fn()
        assert _error_code(e) == code
        for s in range(2):
            assert _same_state(cal.state(s), before[s])

    refused(-4, lambda: cal.step([big], [q0]))                                    # m > 512: LMONO_ECAPACITY
    refused(-4, lambda: lmono_amd.relative_rotation(gpu_ctx, [P0, big]))
    refused(-1, lambda: cal.step([P0], [q0], streams=[2]))                        # stream index out of range
    refused(-1, lambda: cal.step([P0], [q0], streams=[-1]))
    refused(-1, lambda: cal.step([P0, P0], [q0, q0], streams=[1, 1]))             # named twice in one call
    refused(-1, lambda: cal.push([q0, q0], [q0, q0], streams=[0, 0]))
    refused(-1, lambda: cal.step([P0], [nanq]))                                   # a quaternion that is not finite
    refused(-1, lambda: cal.push([nanq], [q0]))
    refused(-1, lambda: cal.push([q0], [nanq * 0 + np.inf]))
    cal.count = 0
    refused(-1, lambda: cal.step([P0], [q0]))                                     # count < 1
    cal.count = 10
    # a negative m cannot be written as a list of arrays: the C entry point directly
    L = gpu_ctx.L
    m = np.array([-1], np.int32); st = np.array([0], np.int32)
    assert L.lmono_excalib_step(cal.h, 1, st.ctypes.data, m.ctypes.data, P0.ctypes.data, q0.ctypes.data, 10, None, None, None, None, None, None) == -1
    assert L.lmono_relative_rotation(gpu_ctx.h, 1, m.ctypes.data, P0.ctypes.data, None, None) == -1
    for s in range(2):
        assert _same_state(cal.state(s), before[s])
    # the next good call works, and gives what a handle that saw no refused call gives
    P1, _, q1 = frames[1]
    got = cal.step([P1], [q1], streams=[1])
    ref = X.Calibrator(10)
    ref.step(P0, q0)
    R, stats, rlc, sv, huber, ok = ref.step(P1, q1)
    assert got["R_cam"][0].tobytes() == R.tobytes() and got["stats"][0].tolist() == stats.tolist()
    assert cal.state(1)[0] == 2 and cal.state(0)[0] == 1
    cal.close()
