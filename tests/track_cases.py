"""Inputs for the edge-case tests of the device feature tracker (tests/test_track_cases_cpu.py, tests/test_track_edges_gpu.py):
short and lopsided pyramids, tied corner responses, the ends of the MIN_DIST range, a full 512-slot point table, streams that start empty and
empty again.  No GPU here: seeded builders, the case table, and the restatement's answer per case (tests/track_ref.py), computed once per
session and shared.  What reference() returns is read-only."""
import functools

import numpy as np

from tests import track_ref as R

DT = 0.05          # frame k of every case is tracked at time DT * k


def cam_params(w, h):
    """The camera convention of tests/test_track_gpu.py: fx = 0.9 w, fy = 1.01 fx, cx = w / 2 - 3, cy = h / 2 + 2."""
    fx = 0.9 * w
    return fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0


def ref_cam(w, h):
    return R.Camera(w, h, *cam_params(w, h))


def _crops(world, w, h, n):
    assert world.shape[0] >= h + (n - 1) // 2 and world.shape[1] >= w + n - 1
    return [np.ascontiguousarray(world[k // 2:k // 2 + h, k:k + w]) for k in range(n)]


def blocky(seed, w, h, n, block=4):
    """n frames of a world of block x block constant squares of uniform random bytes; frame k is the crop at offset (k, k // 2): corners at
    the block joints, moving by (1, 0.5) px per frame."""
    rng = np.random.default_rng(seed)
    world = np.kron(rng.integers(0, 256, (-(-h // block) + 4, -(-w // block) + 4), dtype=np.uint8), np.ones((block, block), np.uint8))
    return _crops(world, w, h, n)


TILE_SEED = 7
FLAT_SEED = 5


def tiled(w, h):
    """Two frames of a 20 x 24 tile of 4 x 4 blocks repeated over the image; frame 1 is the pattern one pixel down and right.  Every corner
    of the tile recurs once per repeat, so many candidates share one response value exactly."""
    rng = np.random.default_rng(TILE_SEED)
    tile = np.kron(rng.integers(0, 256, (6, 5), dtype=np.uint8), np.ones((4, 4), np.uint8))          # 24 rows x 20 columns
    world = np.tile(tile, ((h + 1) // 24 + 1, (w + 1) // 20 + 1))
    return [np.ascontiguousarray(world[k:k + h, k:k + w]) for k in range(2)]


def checker(w, h, cell=8):
    """Two frames of a 0 / 255 checkerboard, frame 1 rolled by one column: one single response value at every corner candidate."""
    yy, xx = np.mgrid[0:h, 0:w]
    f0 = ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)
    return [f0, np.ascontiguousarray(np.roll(f0, 1, axis=1))]


def flat_then_texture():
    """64 x 48: flat 77, flat 77, blocky f0, blocky f1, flat 200, blocky f2 -- a stream that starts empty, fills, empties and fills again."""
    w, h = 64, 48
    b = blocky(FLAT_SEED, w, h, 3)
    return [np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8), b[0], b[1], np.full((h, w), 200, np.uint8), b[2]]


class Case:
    def __init__(self, name, w, h, max_cnt, min_dist, build):
        self.name, self.w, self.h, self.max_cnt, self.min_dist, self._build = name, w, h, max_cnt, min_dist, build

    @property
    def frames(self):
        return _frames(self.name)

    def __repr__(self):
        return self.name


# (w, h) -> pyramid levels; 169 x 43: the height ends the pyramid before the width does
LEVELS = {(22, 22): 1, (42, 42): 1, (130, 22): 1, (40, 30): 1, (43, 43): 2, (169, 43): 2, (100, 90): 3, (168, 168): 3, (169, 169): 4}

# (w, h, max_cnt, min_dist): three blocky frames each
PYRAMID_SHAPES = [(22, 22, 8, 3), (40, 30, 20, 4), (42, 42, 20, 4), (130, 22, 30, 4), (169, 43, 40, 5), (100, 90, 40, 6), (168, 168, 60, 8),
                  (169, 169, 60, 8)]
LK_SHAPES = [(40, 30), (169, 43), (100, 90)]
# (builder, w, h, max_cnt, min_dist): two frames each
TIED_SHAPES = [("tiled", 140, 96, 512, 1), ("tiled", 140, 96, 512, 3), ("tiled", 140, 96, 100, 7), ("checker", 128, 96, 200, 6)]
# (w, h, max_cnt, min_dist): three blocky frames each; at 63 x 47 the circle of radius 128 is larger than the image
RADIUS_SHAPES = [(320, 240, 150, 1), (320, 240, 150, 128), (320, 240, 150, 100), (63, 47, 150, 128)]


def pyramid_name(w, h, max_cnt, min_dist):
    return "blocky_%dx%d_c%d_r%d" % (w, h, max_cnt, min_dist)


def tied_name(kind, w, h, max_cnt, min_dist):
    return "%s_%dx%d_c%d_r%d" % (kind, w, h, max_cnt, min_dist)


def _table():
    cases = {}

    def add(name, w, h, max_cnt, min_dist, build):
        assert name not in cases
        cases[name] = Case(name, w, h, max_cnt, min_dist, build)
    for i, (w, h, c, r) in enumerate(PYRAMID_SHAPES):
        add(pyramid_name(w, h, c, r), w, h, c, r, functools.partial(blocky, 100 + i, w, h, 3))
    for kind, w, h, c, r in TIED_SHAPES:
        add(tied_name(kind, w, h, c, r), w, h, c, r, functools.partial(tiled if kind == "tiled" else checker, w, h))
    for i, (w, h, c, r) in enumerate(RADIUS_SHAPES):
        add(pyramid_name(w, h, c, r), w, h, c, r, functools.partial(blocky, 200 + i, w, h, 3))
    add("full_table", 320, 240, 512, 4, functools.partial(blocky, 3, 320, 240, 3))
    add("flat_then_texture", 64, 48, 30, 4, flat_then_texture)
    return cases


CASES = _table()
FULL_TABLE = CASES["full_table"]
FLAT = CASES["flat_then_texture"]
PYRAMID_CASES = [CASES[pyramid_name(*s)] for s in PYRAMID_SHAPES]
TIED_CASES = [CASES[tied_name(*s)] for s in TIED_SHAPES]
RADIUS_CASES = [CASES[pyramid_name(*s)] for s in RADIUS_SHAPES]
ONE_LEVEL_CASES = [c for c in PYRAMID_CASES if LEVELS[(c.w, c.h)] == 1]
# the streams of the mixed batch, smallest image first: they differ in size, level count, max_cnt and min_dist
BATCH_CASES = [CASES[pyramid_name(22, 22, 8, 3)], CASES[pyramid_name(130, 22, 30, 4)], FLAT, CASES[pyramid_name(169, 43, 40, 5)],
               CASES[pyramid_name(100, 90, 40, 6)], CASES[tied_name("tiled", 140, 96, 512, 3)], FULL_TABLE]


@functools.lru_cache(maxsize=None)
def _frames(name):
    frames = CASES[name]._build()
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


class Run:
    """The restatement's answer for one case: records per frame, the number of survivors (track_cnt > 1) per frame, the corner response of
    frame 0 and the tracker after the last frame (its cur_pyr and last_resp are what the device's diagnostics return)."""

    def __init__(self, case, n_frames=None):
        self.tracker = R.TrackerRef(ref_cam(case.w, case.h), case.max_cnt, case.min_dist)
        self.records, self.resp0 = [], None
        for k, f in enumerate(cycled(case, n_frames or len(case.frames))):
            self.records.append(self.tracker.track(DT * k, f))
            if k == 0:
                self.resp0 = self.tracker.last_resp
        self.counts = [len(r) for r in self.records]
        self.survivors = [int((r["track_cnt"] > 1).sum()) for r in self.records]


def cycled(case, n):
    """n frames of a case, starting over where the case has fewer."""
    return [case.frames[k % len(case.frames)] for k in range(n)]


@functools.lru_cache(maxsize=None)
def reference(name):
    return Run(CASES[name])


@functools.lru_cache(maxsize=None)
def reference_first3(name):
    """The records of the first three frames of cycled(case, ...)."""
    return reference(name).records[:3] if len(CASES[name].frames) >= 3 else Run(CASES[name], 3).records


def first_selection(case):
    """-> (response of frame 0, [(x, y)] selected on it, in order) of a case, by the restatement's detect()."""
    resp = R.response(case.frames[0])
    return resp, R.detect(resp, np.ones(resp.shape, bool), case.max_cnt, case.min_dist)


def lk_points(w, h, corners):
    """The point set of the LK diagnostic: the given corners, a lattice over the image that includes rows and columns 0, 2.5, 10.25 and
    side - 1, and points outside the image on each side.  -> ([n, 2] fp32, number of points inside the image)."""
    xs = sorted(set([0.0, 2.5, 10.25, w - 1.0] + list(np.linspace(0.0, w - 1.0, 7))))
    ys = sorted(set([0.0, 2.5, 10.25, h - 1.0] + list(np.linspace(0.0, h - 1.0, 6))))
    lattice = [(x, y) for y in ys for x in xs]
    outside = [(-5.0, 0.4 * h), (w + 4.0, 0.6 * h), (0.3 * w, -5.0), (0.7 * w, h + 4.0), (-40.0, -40.0), (1e6, 1e6), (w + 4.0, -5.0), (-40.0, h + 4.0)]
    inside = np.vstack([np.asarray(corners, np.float32).reshape(-1, 2), np.array(lattice, np.float32)])
    pts = np.vstack([inside, np.array(outside, np.float32)])
    assert len(pts) <= R.MAX_POINTS
    return pts, len(inside)


@functools.lru_cache(maxsize=None)
def lk_reference(w, h):
    """What lk() must return after the first two frames of the blocky case of this size: -> (case, pts, forward positions, forward status,
    indices of the points alive after the forward pass, their backward positions, their backward status).  The split is the tracker's own:
    forward with levels <= 3, backward with levels <= 1 started at the points themselves."""
    case = [c for c in PYRAMID_CASES if (c.w, c.h) == (w, h)][0]
    rec0 = reference(case.name).records[0]
    pts, _ = lk_points(w, h, np.stack([rec0["u"], rec0["v"]], 1))
    p0, p1 = R.build_pyramid(case.frames[0]), R.build_pyramid(case.frames[1])
    fwd, st = R.lk_track(p0, p1, pts, R.MAX_LEVEL)
    live = np.nonzero(st)[0]
    rev, rst = R.lk_track(p1, p0, fwd[live], 1, init=pts[live])
    return case, pts, fwd, st, live, rev, rst
