"""The tracker's epipolar rejection on the device (k_trk_reject, lmono_tracker_set_reject_f / _reject_stats / _reject_f, DESIGN.md 6e
item 4a) against its CPU restatement tests/track_reject_ref.py: equal bytes, the standard of tests/test_track_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import track_ref as R
from tests import track_reject_ref as RR
from tests import test_track_reject_cpu as CPU
from workloads import s5, s6

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


def _cams(w, h, fx, cx, cy, dist=(0.0, 0.0, 0.0, 0.0)):
    import lmono_amd
    return lmono_amd.Camera(w, h, fx, fx, cx, cy, dist[0], dist[1], dist[2], dist[3], 5, 0, 0), R.Camera(w, h, fx, fx, cx, cy, *dist)


def _same(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.dtype == b.dtype, (what, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), what


def _prm(p):
    return RR.RejectParams(p["f_threshold"], p["f_dis"], p.get("focal_length", 460.0), p.get("n_hyp", 256), p.get("seed", 0))


@pytest.mark.parametrize("dist", [None, CPU.DIST])
@pytest.mark.parametrize("thr", [CPU.LOOSE, CPU.TIGHT])
@pytest.mark.parametrize("m", [8, 9, 150, 512])
def test_reject_f_diagnostic_equals_restatement(gpu_ctx, m, thr, dist):
    import lmono_amd
    gc, rc = _cams(CPU.W, CPU.H, CPU.FX, 620.5, 188.0, dist or (0.0, 0.0, 0.0, 0.0))
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 150, 30)
    for seed, sideways, n_hyp in ((0, False, 256), (1, True, 100), (2, False, 1024)):
        _, p, c, outlier = CPU.correspondences(m, seed, dist, sideways)
        tr.set_reject_f(thr[0], thr[1], n_hyp=n_hyp, seed=seed + 40)
        st, stats, F = tr.reject_f(p, c, frame_key=seed + 3)
        rst, rstats, rF = RR.reject(rc, p, c, RR.RejectParams(thr[0], thr[1], n_hyp=n_hyp, seed=seed + 40), seed + 3)
        _same(stats, rstats, "stats m %d seed %d" % (m, seed))
        _same(st, rst, "status m %d seed %d" % (m, seed))
        _same(F, rF, "F m %d seed %d" % (m, seed))
        assert stats[0] > 0
    # degenerate input: all pairs identical -> all dropped, no valid hypothesis
    p = np.tile(np.array([[300.0, 200.0]], np.float32), (20, 1))
    st, stats, F = tr.reject_f(p, p + np.float32(1.0), 0)
    rst, rstats, rF = RR.reject(rc, p, p + np.float32(1.0), RR.RejectParams(thr[0], thr[1], n_hyp=1024, seed=42), 0)
    _same(st, rst, "degenerate status"); _same(stats, rstats, "degenerate stats"); _same(F, rF, "degenerate F")
    assert not st.any()
    tr.close()


def _run_pair(gpu_ctx, gc, rc, frames, prm, max_cnt=150, min_dist=15):
    import lmono_amd
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, max_cnt, min_dist)
    tr.set_reject_f(**prm)
    ref = RR.TrackerRejectRef(rc, max_cnt, min_dist, reject=_prm(prm))
    ran = dropped = 0
    for f, img in enumerate(frames):
        g = tr.track(0.1 * f, img); r = ref.track(0.1 * f, img)
        _same(g, r, "frame %d" % f)
        stats, F = tr.reject_stats()
        _same(stats, ref.last_stats, "stats of frame %d" % f)
        _same(F, ref.last_F, "F of frame %d" % f)
        if stats[0] >= 0:
            ran += 1; dropped += int(ref.last_status.sum()) - int(stats[3])
    tr.close()
    return ran, dropped


def test_s6_sequence_records_equal_restatement(gpu_ctx):
    seq = CPU.s6_sequence()
    gc, rc = _cams(640, 480, 460.0, 319.5, 239.5)
    ran, dropped = _run_pair(gpu_ctx, gc, rc, seq.frames, dict(f_threshold=1.0, f_dis=0.5))
    assert ran == seq.n_frames - 1 and dropped >= 10


@pytest.mark.parametrize("dist", [(0.0, 0.0, 0.0, 0.0), (-0.28, 0.07, 0.0002, -0.0003)])
def test_s5_occluder_sequence_records_equal_restatement(gpu_ctx, dist):
    seq = s5.Sequence(W, H, 30, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001, occluder=(110, 70, 210, 170), occluder_from=15)
    fx = 0.9 * W
    gc, rc = _cams(W, H, fx, 0.5 * W - 3.0, 0.5 * H + 2.0, dist)
    ran, _ = _run_pair(gpu_ctx, gc, rc, seq.frames, dict(f_threshold=0.15, f_dis=0.15, seed=9, n_hyp=200))
    assert ran == seq.n_frames - 1


def _batch_params(s):
    if s % 2 == 0:
        return None
    return dict(f_threshold=(1.0, 0.5, 0.15)[s % 3], f_dis=(0.5, 0.15)[s % 2 if s % 4 == 1 else 0], n_hyp=64 + 32 * (s % 5), seed=100 + s)


@pytest.mark.parametrize("n_streams", [1, 3, 64])
def test_batch_equals_single_stream(gpu_ctx, n_streams):
    import torch
    import lmono_amd
    n_frames = 4
    gc, _ = _cams(W, H, 0.9 * W, 0.5 * W - 3.0, 0.5 * H + 2.0)
    seqs = [s6.Sequence(W, H, n_frames, seed=10 + s % 7, flow_far=2.0 + 0.25 * (s % 5), mover_step=2.0 + 0.5 * (s % 3), margin=64) for s in range(min(n_streams, 7))]
    frames = [seqs[s % 7].frames for s in range(n_streams)]
    cnts = [40 + (37 * s) % 111 for s in range(n_streams)]
    prms = [_batch_params(s + (1 if n_streams == 1 else 0)) for s in range(n_streams)]
    single, single_stats = [], []
    for s in range(n_streams):
        tr = lmono_amd.FeatureTracker(gpu_ctx, gc, cnts[s], 12)
        if prms[s] is not None:
            tr.set_reject_f(**prms[s])
        recs, sts = [], []
        for f in range(n_frames):
            recs.append(tr.track(0.05 * f * (1 + s % 2), frames[s][f])); sts.append(tr.reject_stats())
        single.append(recs); single_stats.append(sts)
        tr.close()
    batch = lmono_amd.FeatureTrackerBatch(gpu_ctx, [gc] * n_streams, cnts, 12, reject_f=prms)
    ran = 0
    for f in range(n_frames):
        dev = [torch.from_numpy(frames[s][f]).to("cuda:0") for s in range(n_streams)]
        torch.cuda.synchronize()
        out = batch.track([0.05 * f * (1 + s % 2) for s in range(n_streams)], [d.data_ptr() for d in dev])
        stats = batch.reject_stats()
        for s in range(n_streams):
            _same(out[s], single[s][f], "stream %d frame %d" % (s, f))
            _same(stats[s][0], single_stats[s][f][0], "stats stream %d frame %d" % (s, f))
            _same(stats[s][1], single_stats[s][f][1], "F stream %d frame %d" % (s, f))
            if prms[s] is None:
                assert (stats[s][0] == -1).all()
            elif stats[s][0][0] >= 0:
                ran += 1
    assert ran >= n_frames - 1
    batch.close()


def test_switch_off_and_on_and_reset(gpu_ctx):
    import lmono_amd
    seq = s6.Sequence(W, H, 8, seed=3, margin=64)
    gc, rc = _cams(W, H, 300.0, 159.5, 119.5)
    prm = dict(f_threshold=1.0, f_dis=0.5, seed=5)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 120, 12)
    ref = RR.TrackerRejectRef(rc, 120, 12)

    def run():
        out = []
        for f in range(8):
            on = f < 3 or f >= 5
            if on:
                tr.set_reject_f(**prm)
            else:
                tr.set_reject_f(None)
            ref.set_reject_f(_prm(prm) if on else None)
            g = tr.track(0.1 * f, seq.frames[f]); r = ref.track(0.1 * f, seq.frames[f])
            _same(g, r, "frame %d (rejection %s)" % (f, "on" if on else "off"))
            stats, F = tr.reject_stats()
            _same(stats, ref.last_stats, "stats frame %d" % f); _same(F, ref.last_F, "F frame %d" % f)
            assert (stats[0] >= 0) == (on and f > 0)
            out.append((g, stats, F))
        return out
    first = run()
    tr.reset(); ref.reset()
    again = run()
    for f, (a, b) in enumerate(zip(first, again)):
        _same(a[0], b[0], "records after reset, frame %d" % f); _same(a[1], b[1], "stats after reset"); _same(a[2], b[2], "F after reset")
    tr.close()


def test_rejection_off_equals_plain_tracker(gpu_ctx):
    import lmono_amd
    seq = s6.Sequence(W, H, 6, seed=4, margin=64)
    gc, rc = _cams(W, H, 300.0, 159.5, 119.5)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 120, 12)
    tr.set_reject_f(1.0, 0.5)
    tr.set_reject_f(None)
    ref = R.TrackerRef(rc, 120, 12)
    for f in range(6):
        _same(tr.track(0.1 * f, seq.frames[f]), ref.track(0.1 * f, seq.frames[f]), "frame %d" % f)
        assert (tr.reject_stats()[0] == -1).all()
    tr.close()


def test_error_returns(gpu_ctx):
    import lmono_amd
    gc, _ = _cams(W, H, 300.0, 159.5, 119.5)
    with pytest.raises(lmono_amd.LmonoError, match="lmono_tracker_set_reject_f"):
        lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15, flags=1)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15)
    pts = np.zeros((20, 2), np.float32)
    with pytest.raises(lmono_amd.LmonoError, match="set_reject_f"):
        tr.reject_f(pts, pts, 0)                        # rejection is off
    for bad in (dict(f_threshold=0.0, f_dis=0.5), dict(f_threshold=-1.0, f_dis=0.5), dict(f_threshold=float("nan"), f_dis=0.5),
                dict(f_threshold=1.0, f_dis=0.0), dict(f_threshold=1.0, f_dis=float("inf")), dict(f_threshold=1.0, f_dis=0.5, n_hyp=1025)):
        with pytest.raises(lmono_amd.LmonoError, match="f_threshold"):
            tr.set_reject_f(**bad)
    tr.set_reject_f(1.0, 0.5, focal_length=0.0, n_hyp=0)            # the defaults: 460, 256
    for n in (7, 513):
        p = np.zeros((n, 2), np.float32)
        with pytest.raises(lmono_amd.LmonoError, match="8..512"):
            tr.reject_f(p, p, 0)
    L = gpu_ctx.L
    assert L.lmono_tracker_set_reject_f(gpu_ctx.h, None, None) == -1
    assert L.lmono_tracker_reject_stats(gpu_ctx.h, None, None, None) == -1
    tr.close()


def test_host_mirror_track_test_with_rejection(gpu_ctx):
    exe = os.path.join(ROOT, "lmono_amd", "host", "track_test")
    assert os.path.exists(exe), "build() makes lmono_amd/host/track_test"
    res = subprocess.run([exe, "24", "0", "reject"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("TRK ")]
    assert len(lines) == 24 and "track_test ok: 24 frames" in res.stdout and "rejectWithF on" in res.stdout
    assert len([l for l in res.stdout.splitlines() if l.startswith("REJ ")]) == 24


def test_example_track_sequence_with_rejection_into_estimator(gpu_ctx, tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "track_sequence.py"), "--synthetic", "20", "--reject-f", "1.0", "0.5", "--estimator",
                          "--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "estimator ok: 20 frames accepted" in res.stdout
    assert len([l for l in res.stdout.splitlines() if "rejectWithF:" in l]) == 19
