"""The inputs of tests/test_track_edges_gpu.py (tests/track_cases.py) judged on the CPU restatement alone (tests/track_ref.py):
each case has the property it is run for -- the level count, ties among the selected corners, a full table with quota 0, an empty stream --
so an edit of a builder cannot silently empty it; and each tie, border and mask rule the device tests are meant to pin changes the
restatement's answer on a named case when it is deliberately broken, so a kernel broken the same way cannot equal the restatement."""
import numpy as np
import pytest

from tests import track_cases as TC
from tests import track_ref as R


def _differs(a, b):
    return a.shape != b.shape or a.tobytes() != b.tobytes()


def _runs_differ(a, b):
    return any(_differs(x, y) for x, y in zip(a.records, b.records))


# ---------------------------------------------------------------- conditions on the inputs

@pytest.mark.parametrize("size", sorted(TC.LEVELS))
def test_level_counts(size):
    w, h = size
    assert R.n_levels(w, h) == TC.LEVELS[size]
    img = np.zeros((h, w), np.uint8)
    pyr = R.build_pyramid(img)
    assert len(pyr) == TC.LEVELS[size] and all(min(l[0].shape) > R.WIN for l in pyr)


def test_the_case_table_covers_every_level_count_and_a_lopsided_stop():
    assert sorted({TC.LEVELS[(c.w, c.h)] for c in TC.PYRAMID_CASES}) == [1, 2, 3, 4]
    assert {TC.LEVELS[s] for s in TC.LK_SHAPES} == {1, 2, 3}
    # 169 x 43: the width alone would carry four levels, the height ends the pyramid at two
    assert R.n_levels(169, 169) == 4 and R.n_levels(43, 43) == 2 and R.n_levels(169, 43) == 2
    assert len(TC.ONE_LEVEL_CASES) == 4
    b = TC.BATCH_CASES
    assert len(b) == 7 and len({(c.w, c.h) for c in b}) == 7 and len({c.max_cnt for c in b}) >= 4 and len({c.min_dist for c in b}) >= 3
    assert sorted({TC.LEVELS.get((c.w, c.h), R.n_levels(c.w, c.h)) for c in b}) == [1, 2, 3, 4]
    assert [c.w * c.h for c in b] == sorted(c.w * c.h for c in b)


@pytest.mark.parametrize("case", TC.PYRAMID_CASES + TC.TIED_CASES + TC.RADIUS_CASES + [TC.FULL_TABLE, TC.FLAT], ids=repr)
def test_lk_results_reach_the_records(case):
    run = TC.reference(case.name)
    assert len(run.records) == len(case.frames) >= 2
    assert max(run.survivors[1:]) >= 1
    if case is not TC.FLAT:
        assert run.survivors[-1] >= 1 and run.counts[0] >= 1


@pytest.mark.parametrize("case", TC.TIED_CASES, ids=repr)
def test_tied_cases_are_tied(case):
    resp, sel = TC.first_selection(case)
    rec = TC.reference(case.name).records[0]
    assert [(int(u), int(v)) for u, v in zip(rec["u"], rec["v"])] == sel
    v = np.array([resp[y, x] for x, y in sel])
    tied = int((v[1:] == v[:-1]).sum())
    print("%s: %d selected, %d of %d consecutive pairs tied" % (case, len(sel), tied, len(sel) - 1))
    assert 2 * tied >= len(sel) - 1 and len(sel) >= 100
    if case.name.startswith("checker"):
        assert tied == len(sel) - 1


def test_tied_inputs_have_few_distinct_responses():
    for case, n_cand, n_val, n_top in ((TC.TIED_CASES[0], 754, 32, 28), (TC.TIED_CASES[3], 660, 1, 660)):
        resp = R.response(case.frames[0])
        _, pix = R.detect_candidates(resp, np.ones(resp.shape, bool))
        _, counts = np.unique(resp.reshape(-1)[pix], return_counts=True)
        assert (len(pix), len(counts), int(counts.max())) == (n_cand, n_val, n_top)


def test_full_table_fills_and_runs_a_frame_with_quota_zero():
    run = TC.reference(TC.FULL_TABLE.name)
    assert run.counts == [512, 512, 512]
    assert run.survivors[0] == 0 and 0 < run.survivors[1] < 512 and run.survivors[2] == 512
    print("full table: survivors", run.survivors)
    # quota == 0 on the third frame: nothing new, the 512 survivors of the second frame in setMask's order
    assert (run.records[2]["track_cnt"] >= 2).all() and set(run.records[2]["id"]) == set(run.records[1]["id"])


def test_radius_extremes():
    big = TC.reference(TC.pyramid_name(320, 240, 150, 128))
    assert all(2 <= n <= 8 for n in big.counts)
    assert TC.reference(TC.pyramid_name(320, 240, 150, 1)).counts == [150, 150, 150]
    # the circle covers the whole 63 x 47 image wherever its centre lies: one corner
    assert TC.reference(TC.pyramid_name(63, 47, 150, 128)).counts == [1, 1, 1]
    assert R.circle_spans(128).min() >= 0 and R.circle_spans(128)[0] == 128 and 2 * 100 > 63


def test_stream_that_starts_empty_and_empties_again():
    run = TC.reference(TC.FLAT.name)
    assert run.counts == [0, 0, 30, 30, 0, 30]
    assert run.survivors == [0, 0, 0, 28, 0, 0]
    ids = [set(r["id"].tolist()) for r in run.records]
    assert min(ids[2]) == 0 and min(ids[5]) > max(ids[3]), "ids continue after the flat frame"
    assert sorted(ids[5]) == list(range(min(ids[5]), min(ids[5]) + 30))


@pytest.mark.parametrize("size", TC.LK_SHAPES)
def test_lk_point_sets_have_both_status_values(size):
    w, h = size
    case, pts, fwd, st, live, rev, rst = TC.lk_reference(w, h)
    print("%s: %d points, forward status 1 on %d, backward status 1 on %d" % (case, len(pts), int(st.sum()), int(rst.sum())))
    assert 0 < st.sum() < len(pts) and rst.sum() >= 10
    assert st[-8:].sum() < 8 and not st[-4:-2].any()          # (-40, -40) and (1e6, 1e6) have no window origin at level 0
    for v in (0.0, 2.5, 10.25):
        assert (pts[:, 0] == v).any() and (pts[:, 1] == v).any()
    assert (pts[:, 0] == w - 1).any() and (pts[:, 1] == h - 1).any()
    assert (pts[:, 0] < -21).any() and (pts[:, 0] >= w).any() and (pts[:, 1] < 0).any() and (pts[:, 1] >= h).any()


# ---------------------------------------------------------------- sensitivity: deliberately wrong variants of the restatement

def _candidates(resp, mask, higher_pixel_first=False, strict=False):
    """R.detect_candidates with one rule changed."""
    h, w = resp.shape
    m = resp[mask]
    maxv = R.F32(max(float(m.max()), 0.0)) if m.size else R.F32(0)
    thr = R.F32(np.float64(maxv) * 0.01)
    c = resp[1:-1, 1:-1]
    nb = np.full(c.shape, -np.inf, np.float32)
    for i in range(3):
        for j in range(3):
            if not (strict and i == 1 and j == 1):
                nb = np.maximum(nb, resp[i:i + h - 2, j:j + w - 2])
    ok = (c > thr) & ((c > nb) if strict else (c == nb)) & mask[1:-1, 1:-1]
    ys, xs = np.nonzero(ok)
    pix = (ys + 1) * w + (xs + 1)
    vals = resp.reshape(-1)[pix]
    return thr, pix[np.lexsort((-pix if higher_pixel_first else pix, -vals.astype(np.float64)))]


def _detect_closed(resp, mask, quota, min_dist):
    """R.detect that suppresses at <= r^2."""
    w = resp.shape[1]
    _, pix = R.detect_candidates(resp, mask)
    out = []
    for p in pix:
        if len(out) >= quota:
            break
        x, y = int(p % w), int(p // w)
        if all((a - x) ** 2 + (b - y) ** 2 > min_dist * min_dist for a, b in out):
            out.append((x, y))
    return out


_set_mask = R.set_mask
_lk_track = R.lk_track


def _set_mask_reversed(pts, ids, cnt, r, w, h):
    """R.set_mask with equal counts in reversed order."""
    n = len(pts)
    keep, mask = _set_mask(pts[::-1], ids[::-1], cnt[::-1], r, w, h)
    return [n - 1 - i for i in keep], mask


def _lk_backward_from_level_0(pyr_i, pyr_j, prev_pts, max_level, init=None):
    return _lk_track(pyr_i, pyr_j, prev_pts, 0 if init is not None else max_level, init=init)


def _open_disc_spans(r):
    """Row half widths of the open Euclidean disc dx^2 + dy^2 < r^2, the rule of the selection step, used for the mask."""
    return np.array([int(np.ceil(np.sqrt(r * r - d * d))) - 1 for d in range(r + 1)], np.int32)


def test_the_midpoint_circle_is_the_closed_euclidean_disc():
    """OpenCV's filled midpoint circle carries err = dx^2 + dy^2 - r^2 exactly and steps dx down when it is positive, so its raster is the
    closed disc dx^2 + dy^2 <= r^2 for every radius the tracker takes.  A mask variant therefore has to differ from the closed disc to be a
    variant at all: variant 6 below is the open disc."""
    for r in range(1, 129):
        d = np.arange(-r, r + 1)
        assert np.array_equal(R.circle_mask(r), d[:, None] ** 2 + d[None, :] ** 2 <= r * r), r
        assert (_open_disc_spans(r)[:r] <= R.circle_spans(r)[:r]).all() and _open_disc_spans(r)[0] == r - 1


def test_variant_1_ties_to_the_higher_pixel_index(monkeypatch):
    monkeypatch.setattr(R, "detect_candidates", lambda resp, mask: _candidates(resp, mask, higher_pixel_first=True))
    for case in TC.TIED_CASES:
        assert _differs(TC.Run(case, 1).records[0], TC.reference(case.name).records[0]), case


def test_variant_2_strict_maximum_drops_plateaus(monkeypatch):
    monkeypatch.setattr(R, "detect_candidates", lambda resp, mask: _candidates(resp, mask, strict=True))
    case = TC.TIED_CASES[3]                 # the checkerboard: every corner is a 2 x 2 plateau
    assert len(TC.Run(case, 1).records[0]) == 0 and len(TC.reference(case.name).records[0]) == 165


@pytest.mark.parametrize("case", [TC.TIED_CASES[1], TC.CASES[TC.pyramid_name(42, 42, 20, 4)]], ids=repr)
def test_variant_3_unstable_set_mask(monkeypatch, case):
    monkeypatch.setattr(R, "set_mask", _set_mask_reversed)
    assert _runs_differ(TC.Run(case), TC.reference(case.name))


@pytest.mark.parametrize("case", [TC.CASES[TC.pyramid_name(42, 42, 20, 4)], TC.TIED_CASES[1]], ids=repr)
def test_variant_4_selection_suppresses_at_r_squared(monkeypatch, case):
    monkeypatch.setattr(R, "detect", _detect_closed)
    assert _differs(TC.Run(case, 1).records[0], TC.reference(case.name).records[0])


@pytest.mark.parametrize("size", TC.LK_SHAPES + [(22, 22), (130, 22)])
def test_variant_5_backward_pass_from_level_0(monkeypatch, size):
    """The backward pass decides only which points are kept, so the variant is judged on what lk() returns: the backward positions."""
    case = [c for c in TC.PYRAMID_CASES if (c.w, c.h) == size][0]
    p0, p1 = R.build_pyramid(case.frames[0]), R.build_pyramid(case.frames[1])
    rec = TC.reference(case.name).records[0]
    pts = np.stack([rec["u"], rec["v"]], 1)
    fwd, st = R.lk_track(p0, p1, pts, R.MAX_LEVEL)
    live = np.nonzero(st)[0]
    assert len(live) >= 5
    want = R.lk_track(p1, p0, fwd[live], 1, init=pts[live])
    monkeypatch.setattr(R, "lk_track", _lk_backward_from_level_0)
    got = R.lk_track(p1, p0, fwd[live], 1, init=pts[live])
    changed = _differs(got[0], want[0]) or _differs(got[1], want[1])
    assert changed == (TC.LEVELS[size] > 1)
    if TC.LEVELS[size] == 1:
        assert not _runs_differ(TC.Run(case), TC.reference(case.name))


@pytest.mark.parametrize("case", [TC.TIED_CASES[1], TC.CASES[TC.pyramid_name(42, 42, 20, 4)]], ids=repr)
def test_variant_6_open_disc_mask(monkeypatch, case):
    monkeypatch.setattr(R, "circle_spans", _open_disc_spans)
    assert _runs_differ(TC.Run(case), TC.reference(case.name))
