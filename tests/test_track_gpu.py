"""Device feature tracker (lmono_tracker_*) against its CPU restatement tests/track_ref.py: equal bytes."""
import os

import numpy as np
import pytest

from tests import track_ref as R
from workloads import s5

pytestmark = pytest.mark.gpu

W, H = 320, 240
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cam(w, h, dist=(0.0, 0.0, 0.0, 0.0)):
    import lmono_amd
    fx = 0.9 * w
    return (lmono_amd.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, dist[0], dist[1], dist[2], dist[3], 5, 0, 0),
            R.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, *dist))


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def _occluder_sequence(seed=1, n=30):
    return s5.Sequence(W, H, n, seed=seed, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001, occluder=(110, 70, 210, 170), occluder_from=n // 2)


@pytest.mark.parametrize("w,h", [(1241, 376), (640, 480), (63, 47)])
def test_pyramid_and_derivative_planes(gpu_ctx, w, h):
    import lmono_amd
    if w > 100:
        img = s5.Sequence(w, h, 1, seed=3, margin=8).frames[0]
    else:
        img = np.random.default_rng(2).integers(0, 256, (h, w), dtype=np.uint8)
    gc, rc = _cam(w, h)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 40, 10)
    rt = R.TrackerRef(rc, 40, 10)
    g0 = tr.track(0.0, img); r0 = rt.track(0.0, img)
    # neither size is a multiple of the 64 x 16 response tile: the partial right / bottom tiles and their REFLECT_101 cells
    _same(tr.response(), rt.last_resp, "corner response")
    _same(g0, r0, "corners of the first frame")
    assert len(r0) > 0
    ref = R.build_pyramid(img)
    assert tr.n_levels() == len(ref) == R.n_levels(w, h)
    assert len(ref) == (4 if w > 100 else 2)
    for l, (ri, rdx, rdy) in enumerate(ref):
        gi, gdx, gdy = tr.pyramid(l)
        _same(gi, ri, "image level %d" % l); _same(gdx, rdx, "dx level %d" % l); _same(gdy, rdy, "dy level %d" % l)
    tr.close()


@pytest.mark.parametrize("max_cnt", [1, 150, 512])
def test_response_and_selected_corners(gpu_ctx, max_cnt):
    import lmono_amd
    w, h = 640, 480
    seq = s5.Sequence(w, h, 2, seed=4, step=(2.0, -1.0), margin=16)
    gc, rc = _cam(w, h)
    min_dist = 30 if max_cnt <= 150 else 9
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, max_cnt, min_dist)
    ref = R.TrackerRef(rc, max_cnt, min_dist)
    g0 = tr.track(0.0, seq.frames[0]); r0 = ref.track(0.0, seq.frames[0])
    _same(tr.response(), ref.last_resp, "corner response, no mask")
    # this image may hold fewer than 512 corners; all 512 slots live is tests/test_track_edges_gpu.py::test_all_512_slots_live
    assert len(r0) == max_cnt or max_cnt == 512
    _same(g0, r0, "corners of the first frame (position and order)")
    # second frame: the kept points mask part of the image
    g1 = tr.track(0.1, seq.frames[1]); r1 = ref.track(0.1, seq.frames[1])
    if max_cnt - int((r1["track_cnt"] > 1).sum()) > 0:
        _same(tr.response(), ref.last_resp, "corner response, second frame")
    _same(g1, r1, "second frame: survivors, then corners found under the mask")
    tr.close()


def test_lk_fixed_point_set(gpu_ctx):
    import lmono_amd
    # a flat rectangle in both frames (min-eigenvalue failures), a 14 px shift (points near the border leave the image)
    seq = s5.Sequence(W, H, 2, seed=5, motion=[(0, 0, 0, 1), (-14.0, 9.0, 0.01, 1.0)], occluder=(130, 90, 200, 160), occluder_from=0, occluder_fill=120)
    gc, rc = _cam(W, H)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 50, 15)
    tr.track(0.0, seq.frames[0]); tr.track(0.1, seq.frames[1])
    corners = np.array(R.detect(R.response(seq.frames[0]), np.ones((H, W), bool), 150, 12), np.float32)
    xs = np.linspace(0.0, W - 1.0, 23); ys = np.linspace(0.0, H - 1.0, 17)
    border = [(x, y) for x in xs for y in (0.0, 3.3, 11.5, 20.75, H - 21.5, H - 9.25, H - 1.0)] + \
             [(x, y) for y in ys for x in (0.0, 2.5, 10.25, 20.5, W - 20.75, W - 8.5, W - 1.0)]
    flat = [(150.5, 110.25), (165.0, 125.0), (180.75, 140.5), (160.0, 100.0)]
    outside = [(-5.0, 30.0), (W + 4.0, 50.0), (40.0, -8.5), (70.0, H + 6.0), (-40.0, -40.0), (1e6, 1e6)]
    pts = np.vstack([corners, np.array(border + flat + outside, np.float32)])[:512]
    fwd, rev, st = tr.lk(pts)
    p0, p1 = R.build_pyramid(seq.frames[0]), R.build_pyramid(seq.frames[1])
    rf, rs = R.lk_track(p0, p1, pts, R.MAX_LEVEL)
    assert np.array_equal(st[:, 0], rs)
    _same(fwd, rf, "forward positions")
    live = np.nonzero(rs)[0]
    rr, rbs = R.lk_track(p1, p0, rf[live], 1, init=pts[live])
    assert np.array_equal(st[live, 1], rbs) and not st[rs == 0, 1].any()
    _same(rev[live], rr, "backward positions")
    assert 0 < rs.sum() < len(pts) and (rs[len(corners) + len(border):len(corners) + len(border) + 4] == 0).all()
    tr.close()


@pytest.mark.parametrize("dist", [(0.0, 0.0, 0.0, 0.0), (-0.28, 0.07, 0.0002, -0.0003)])
def test_sequence_records_equal_restatement(gpu_ctx, dist):
    import lmono_amd
    seq = _occluder_sequence()
    gc, rc = _cam(W, H, dist)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 150, 15)
    ref = R.TrackerRef(rc, 150, 15)
    replaced = 0
    for f in range(seq.n_frames):
        g = tr.track(0.1 * f, seq.frames[f]); r = ref.track(0.1 * f, seq.frames[f])
        _same(g, r, "frame %d" % f)
        replaced += int((r["track_cnt"] == 1).sum())
    assert replaced > 150
    frame = tr.track_image(3.0, seq.frames[-1])
    assert all(len(v) == 1 and v[0][0] == 0 and v[0][1].shape == (6,) for v in frame.values())
    tr.close()


@pytest.mark.parametrize("n_streams", [1, 3, 64])
def test_batch_equals_single_stream(gpu_ctx, n_streams):
    import torch
    import lmono_amd
    n_frames = 4
    gc, _ = _cam(W, H)
    seqs = [s5.Sequence(W, H, n_frames, seed=10 + s % 7, step=(1.0 + 0.25 * (s % 5), -0.5 + 0.2 * (s % 3)), rot_step=0.001 * (s % 4),
                        occluder=(40 + 3 * s, 60, 100 + 3 * s, 120), occluder_from=2) for s in range(n_streams)]
    cnts = [20 + (37 * s) % 131 for s in range(n_streams)]
    single = []
    for s in range(n_streams):
        tr = lmono_amd.FeatureTracker(gpu_ctx, gc, cnts[s], 12)
        single.append([tr.track(0.05 * f * (1 + s % 2), seqs[s].frames[f]) for f in range(n_frames)])
        tr.close()
    batch = lmono_amd.FeatureTrackerBatch(gpu_ctx, [gc] * n_streams, cnts, 12)
    for f in range(n_frames):
        dev = [torch.from_numpy(seqs[s].frames[f]).to("cuda:0") for s in range(n_streams)]
        torch.cuda.synchronize()
        out = batch.track([0.05 * f * (1 + s % 2) for s in range(n_streams)], [d.data_ptr() for d in dev])
        for s in range(n_streams):
            _same(out[s], single[s][f], "stream %d frame %d" % (s, f))
    batch.close()


def test_host_mirror_track_test_runs(gpu_ctx):
    """lmono_amd/host/track_test: synthetic frames -> FeatureTracker::trackImage -> FeatureManager::featureCheck, every frame taken in full."""
    import os
    import subprocess
    exe = os.path.join(ROOT, "lmono_amd", "host", "track_test")
    assert os.path.exists(exe), "build() makes lmono_amd/host/track_test"
    res = subprocess.run([exe, "24"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("TRK ")]
    assert len(lines) == 24 and "track_test ok: 24 frames" in res.stdout
    assert int(lines[-1].split()[5]) >= 50          # survivors of the last frame


def test_example_track_sequence_into_estimator(gpu_ctx, tmp_path):
    """examples/track_sequence.py --synthetic 20 --estimator: every frame's tracks are accepted by Estimator::processImage."""
    import os
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "track_sequence.py"), "--synthetic", "20", "--estimator", "--out", str(tmp_path)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-2000:])
    assert "estimator ok: 20 frames accepted" in res.stdout
    assert len([l for l in res.stdout.splitlines() if l.startswith("estimator frame ")]) == 20
    first = np.loadtxt(str(tmp_path / "000000.txt")); last = np.loadtxt(str(tmp_path / "000019.txt"))
    assert first.shape[1] == 8 and (first[:, 7] == 1).all() and last[:, 7].max() == 20
    # the estimator's track store holds what the tracker gave: the FRM line's last field is feature_manager.feature.size()
    frm0 = [l for l in res.stdout.splitlines() if l.startswith("estimator frame 0:")][0]
    assert int(frm0.split()[-1]) == len(first)


def test_bgr_reset_and_error_returns(gpu_ctx):
    import lmono_amd
    seq = s5.Sequence(W, H, 3, seed=6)
    gc, rc = _cam(W, H)
    tr = lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15)
    tg = lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15)
    first = []
    for f in range(3):
        bgr = s5.bgr_of(seq.frames[f], seed=f)
        a = tr.track(0.1 * f, bgr); b = tg.track(0.1 * f, R.bgr_to_grey(bgr))
        _same(a, b, "BGR8 input against grey input of the converted image, frame %d" % f)
        _same(tr.pyramid(0)[0], R.bgr_to_grey(bgr), "BGR2GRAY")
        first.append(a)
    tr.reset()
    for f in range(3):
        _same(tr.track(0.1 * f, s5.bgr_of(seq.frames[f], seed=f)), first[f], "after reset, frame %d" % f)
    assert first[0]["id"][0] == 0 and first[2]["track_cnt"].max() == 3
    # the error returns
    with pytest.raises(lmono_amd.LmonoError, match="rejectWithF"):
        lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15, flags=1)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.FeatureTracker(gpu_ctx, gc, 513, 15)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.FeatureTracker(gpu_ctx, gc, 0, 15)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 0)
    small, _ = _cam(21, 40)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.FeatureTracker(gpu_ctx, small, 80, 15)
    with pytest.raises(lmono_amd.LmonoError):
        tr.track(0.0, np.zeros((H, W + 1), np.uint8))
    L = gpu_ctx.L
    n = np.zeros(1, np.int32)
    img = np.zeros((H, W), np.uint8)
    assert L.lmono_tracker_track(gpu_ctx.h, tr.h, 0.0, img.ctypes.data, 7, None, 0, n.ctypes.data) == -1
    assert L.lmono_tracker_track(gpu_ctx.h, None, 0.0, img.ctypes.data, 0, None, 0, n.ctypes.data) == -1
    rec = np.zeros(8, lmono_amd.capi.TRACK_RECORD)
    assert L.lmono_tracker_track(gpu_ctx.h, tr.h, 0.0, img.ctypes.data, 0, rec.ctypes.data, 8, n.ctypes.data) == -4
    fresh = lmono_amd.FeatureTracker(gpu_ctx, gc, 80, 15)
    with pytest.raises(lmono_amd.LmonoError):
        fresh.lk(np.zeros((3, 2), np.float32))
    for t in (tr, tg, fresh):
        t.close()


def test_lead_tracker_job_table_grows_and_is_reused(gpu_ctx):
    """One lead tracker drives batches of 1, 3, 5 and 1 streams: its job table grows twice (1 -> 4 -> 8 entries) and is then reused.  The
    other trackers of a batch are fresh, the lead goes on from the batch before; every stream's records at every frame equal those of a
    single-stream tracker fed the same frames.  63 x 47 is the smallest image of this file (two pyramid levels)."""
    import ctypes
    import torch
    import lmono_amd
    w, h, n_frames, sizes = 63, 47, 3, (1, 3, 5, 1)
    gc, _ = _cam(w, h)
    rng = np.random.default_rng(41)
    # blocky noise moved by (1, 0.5) px per frame: corners at the block joints, tracked from frame to frame
    worlds = [np.kron(rng.integers(0, 256, (16, 20), dtype=np.uint8), np.ones((4, 4), np.uint8)) for _ in range(max(sizes))]
    frames = [[np.ascontiguousarray(wd[f // 2:f // 2 + h, f:f + w]) for f in range(n_frames)] for wd in worlds]
    cnts = [30, 17, 40, 8, 25]

    def single(s, n_rounds):
        tr = lmono_amd.FeatureTracker(gpu_ctx, gc, cnts[s], 4)
        out = [tr.track(0.05 * k, frames[s][k % n_frames]) for k in range(n_rounds * n_frames)]
        tr.close()
        return out
    ref = [single(s, len(sizes) if s == 0 else 1) for s in range(max(sizes))]
    assert all(len(r) > 0 for r in ref[0]) and any((r["track_cnt"] > 1).any() for r in ref[0])
    lead = lmono_amd.FeatureTracker(gpu_ctx, gc, cnts[0], 4)
    for rnd, n in enumerate(sizes):
        batch = lmono_amd.FeatureTrackerBatch(gpu_ctx, [gc] * n, cnts[:n], 4)
        batch.trackers[0].close()
        batch.trackers[0] = lead
        batch._handles = (ctypes.c_void_p * n)(*[t.h for t in batch.trackers])
        for f in range(n_frames):
            dev = [torch.from_numpy(frames[s][f]).to("cuda:0") for s in range(n)]
            torch.cuda.synchronize()
            out = batch.track([0.05 * (rnd * n_frames + f)] + [0.05 * f] * (n - 1), [d.data_ptr() for d in dev])
            _same(out[0], ref[0][rnd * n_frames + f], "lead, batch of %d, frame %d" % (n, f))
            for s in range(1, n):
                _same(out[s], ref[s][f], "stream %d of %d, frame %d" % (s, n, f))
        for t in batch.trackers[1:]:
            t.close()
    lead.close()
