"""Device feature tracker (lmono_tracker_*) against its CPU restatement tests/track_ref.py on the inputs of
tests/track_cases.py: pyramids of one, two and three levels and one the height ends early, tied corner responses, MIN_DIST at both ends of
its range, all 512 point slots live, a stream that starts empty and empties again, and one batch of streams unlike in every grid-sizing
quantity.  Equal bytes throughout; tests/test_track_cases_cpu.py shows what each input is good for."""
import ctypes

import numpy as np
import pytest

from tests import track_cases as TC
from tests import track_ref as R

pytestmark = pytest.mark.gpu


def _gpu_cam(w, h):
    import lmono_amd
    fx, fy, cx, cy = TC.cam_params(w, h)
    return lmono_amd.Camera(w, h, fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 5, 0, 0)


def _tracker(ctx, case):
    import lmono_amd
    return lmono_amd.FeatureTracker(ctx, _gpu_cam(case.w, case.h), case.max_cnt, case.min_dist)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def _run_against_reference(ctx, case, after=None):
    """Every frame of the case through a fresh tracker, records compared to the restatement frame by frame."""
    run = TC.reference(case.name)
    tr = _tracker(ctx, case)
    try:
        for k, f in enumerate(case.frames):
            _same(tr.track(TC.DT * k, f), run.records[k], "%s: records of frame %d" % (case, k))
            if k == 0:
                _same(tr.response(), run.resp0, "%s: corner response of frame 0" % case)
        if after is not None:
            after(tr, run)
    finally:
        tr.close()
    return run


@pytest.mark.parametrize("case", TC.PYRAMID_CASES, ids=repr)
def test_short_and_lopsided_pyramids(gpu_ctx, case):
    def after(tr, run):
        assert tr.n_levels() == R.n_levels(case.w, case.h) == TC.LEVELS[(case.w, case.h)] == len(run.tracker.cur_pyr)
        for l, (ri, rdx, rdy) in enumerate(run.tracker.cur_pyr):
            gi, gdx, gdy = tr.pyramid(l)
            _same(gi, ri, "image level %d" % l); _same(gdx, rdx, "dx level %d" % l); _same(gdy, rdy, "dy level %d" % l)
        _same(tr.response(), run.tracker.last_resp, "corner response of the last frame that had a quota")
    run = _run_against_reference(gpu_ctx, case, after)
    assert len(run.records) == 3 and run.survivors[-1] >= 1


@pytest.mark.parametrize("size", TC.LK_SHAPES, ids=lambda s: "%dx%d" % s)
def test_lk_diagnostic_on_short_pyramids(gpu_ctx, size):
    case, pts, rf, rs, live, rr, rbs = TC.lk_reference(*size)
    tr = _tracker(gpu_ctx, case)
    tr.track(0.0, case.frames[0]); tr.track(TC.DT, case.frames[1])
    assert tr.n_levels() == TC.LEVELS[size]
    fwd, rev, st = tr.lk(pts)
    tr.close()
    print("%s: %d points, forward status 1 on %d, backward status 1 on %d" % (case, len(pts), int(rs.sum()), int(rbs.sum())))
    assert np.array_equal(st[:, 0], rs)
    _same(fwd, rf, "forward positions")
    assert np.array_equal(st[live, 1], rbs) and not st[rs == 0, 1].any()
    _same(rev[live], rr, "backward positions")
    # both status values occur
    assert 0 < rs.sum() < len(pts) and set(st[:, 1].tolist()) == {0, 1}


@pytest.mark.parametrize("case", TC.TIED_CASES, ids=repr)
def test_tied_responses_pick_the_same_corners_in_the_same_order(gpu_ctx, case):
    # frame 0: order among equal responses by pixel index alone; frame 1: the same under a mask of kept points
    run = _run_against_reference(gpu_ctx, case)
    assert len(run.records) == 2 and len(run.records[0]) >= 100


@pytest.mark.parametrize("case", TC.RADIUS_CASES, ids=repr)
def test_mask_radius_extremes(gpu_ctx, case):
    run = _run_against_reference(gpu_ctx, case)
    assert len(run.records) == 3 and case.min_dist in (1, 100, 128)


def test_all_512_slots_live(gpu_ctx):
    """Every slot of k_trk_update's rank, sort and suppress loops is live on frames 1 and 2; frame 2 runs with quota == 0 and must report the
    512 survivors in setMask's order with nothing new.  tests/test_track_gpu.py::test_response_and_selected_corners[512] may fill fewer."""
    run = _run_against_reference(gpu_ctx, TC.FULL_TABLE)
    assert run.counts == [512, 512, 512] and run.survivors[2] == 512


def test_stream_that_starts_empty_and_empties_again(gpu_ctx):
    run = _run_against_reference(gpu_ctx, TC.FLAT)
    assert run.counts == [0, 0, 30, 30, 0, 30]
    assert run.records[5]["id"].min() > run.records[3]["id"].max()          # ids continue after the flat frame


N_BATCH_FRAMES = 6
_single = {}


def _single_stream(ctx, case):
    """The case's six (cycled) frames through a single-stream tracker, once per session."""
    if case.name not in _single:
        tr = _tracker(ctx, case)
        _single[case.name] = [tr.track(TC.DT * k, f) for k, f in enumerate(TC.cycled(case, N_BATCH_FRAMES))]
        tr.close()
    return _single[case.name]


@pytest.mark.parametrize("order", ["smallest_first", "largest_first"])
def test_batch_of_unlike_streams(gpu_ctx, order):
    """One lmono_tracker_track_batch call per frame over seven streams that differ in image size, level count, max_cnt and min_dist: every
    grid is sized from a maximum over the streams, so every stream but one relies on its early exits.  The lead tracker (stream 0, whose job
    table is used) is once the smallest and once the largest stream."""
    import torch
    import lmono_amd
    cases = TC.BATCH_CASES if order == "smallest_first" else TC.BATCH_CASES[::-1]
    n = len(cases)
    single = [_single_stream(gpu_ctx, c) for c in cases]
    # FeatureTrackerBatch takes one min_dist: the trackers are built one by one and the handle array is assembled from them
    batch = lmono_amd.FeatureTrackerBatch(gpu_ctx, [_gpu_cam(c.w, c.h) for c in cases], [c.max_cnt for c in cases], 1)
    for t in batch.trackers:
        t.close()
    batch.trackers = [_tracker(gpu_ctx, c) for c in cases]
    batch._handles = (ctypes.c_void_p * n)(*[t.h for t in batch.trackers])
    assert [t.n_levels() for t in batch.trackers] == [R.n_levels(c.w, c.h) for c in cases]
    try:
        for f in range(N_BATCH_FRAMES):
            dev = [torch.from_numpy(np.array(TC.cycled(c, N_BATCH_FRAMES)[f])).to("cuda:0") for c in cases]
            torch.cuda.synchronize()
            out = batch.track([TC.DT * f] * n, [d.data_ptr() for d in dev])
            for s, c in enumerate(cases):
                _same(out[s], single[s][f], "%s (stream %d, %s), frame %d: batch against single stream" % (c, s, order, f))
                if f < 3:
                    _same(out[s], TC.reference_first3(c.name)[f], "%s (stream %d, %s), frame %d: batch against the restatement" % (c, s, order, f))
    finally:
        batch.close()
