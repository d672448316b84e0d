"""tests/keyframe_ref.py -- CPU restatement of the device keyframe descriptors, numpy only.  Test infrastructure:
the kernels of lmono_amd/csrc/keyframe.hip and this file implement one written definition (items 1-6 of 6f); everything but the
normalised keypoints is integer arithmetic, so "equal" means equal bytes.  Restates KeyFrame::computeBRIEFPoint /
computeWindowBRIEFPoint / searchByBRIEFDes (mono_lidar_mapping/src/loop_detection/KeyFrame.cc:172-267) and DVision's BRIEF::compute
(src/loop_detection/DVision/BRIEF.cpp:39-106)."""
import numpy as np

from tests.track_ref import bgr_to_grey

F32 = np.float32
FAST_THRESHOLD = 20
MATCH_START = 128            # searchInAera: bestDist = 128, strict <
MATCH_LIMIT = 80             # ... && bestDist < 80
MIN_BRIEF_LOOP_NUM = 25      # kitti_config_00.yaml:48
# Bresenham circle of radius 3, (dx, dy), in the order of the definition
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
BLUR_WEIGHTS = np.array([7, 17, 32, 46, 52, 46, 32, 17, 7], np.int64)      # exp(-k^2 / 8) normalised, in 1/256

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def grey_of(image):
    image = np.asarray(image, np.uint8)
    return bgr_to_grey(image) if image.ndim == 3 else image


def fast_score(grey, threshold=FAST_THRESHOLD):
    """Item 2: score image, uint8 [h, w]: A - 1 where A > threshold, else 0 (A: the best 9-arc of the 16-circle, either sign)."""
    h, w = grey.shape
    score = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return score
    g = grey.astype(np.int32)
    v = g[3:h - 3, 3:w - 3]
    d = np.stack([v - g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
    best = np.full(v.shape, -256, np.int32)
    for start in range(16):
        arc = d[[(start + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    score[3:h - 3, 3:w - 3] = np.where(best > threshold, best - 1, 0).astype(np.uint8)
    return score


def fast_keypoints(score):
    """Non-maximum suppression: a corner is kept iff its score is strictly greater than its eight neighbours'; row-major order.
    -> float32 [n, 2] (x, y)."""
    s = np.pad(score.astype(np.int32), 1)
    h, w = score.shape
    c = s[1:h + 1, 1:w + 1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > s[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    yx = np.argwhere(keep)
    return np.stack([yx[:, 1], yx[:, 0]], 1).astype(np.float32).reshape(-1, 2)


def blur(grey):
    """Item 3: separable 9-tap Gaussian in 1/256, REFLECT_101, unrounded 16-bit rows, 32-bit columns, one rounding."""
    h, w = grey.shape
    p = np.pad(grey.astype(np.int64), ((0, 0), (4, 4)), mode="reflect")
    rows = sum(int(BLUR_WEIGHTS[k]) * p[:, k:k + w] for k in range(9))
    assert rows.max() <= 65535
    p = np.pad(rows, ((4, 4), (0, 0)), mode="reflect")
    cols = sum(int(BLUR_WEIGHTS[k]) * p[k:k + h, :] for k in range(9))
    return ((cols + 32768) >> 16).astype(np.uint8)


def brief(blurred, pts, pattern):
    """Item 4.  pts: float32 [n, 2]; pattern: (x1, y1, x2, y2), integer arrays of one length (256 in the product).
    -> uint32 [n, ceil(bits / 32)]: bit i is bit (i & 31) of word (i >> 5)."""
    h, w = blurred.shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    x1, y1, x2, y2 = (np.asarray(a).astype(np.float32)[None, :] for a in pattern)
    nbits = x1.shape[1]
    px = pts[:, 0:1]; py = pts[:, 1:2]
    with np.errstate(invalid="ignore", over="ignore"):
        c = [np.trunc((px + x1).astype(np.float32)), np.trunc((py + y1).astype(np.float32)),      # fp32 add, conversion toward zero
             np.trunc((px + x2).astype(np.float32)), np.trunc((py + y2).astype(np.float32))]
        inside = (c[0] >= 0) & (c[0] < w) & (c[1] >= 0) & (c[1] < h) & (c[2] >= 0) & (c[2] < w) & (c[3] >= 0) & (c[3] < h)
    ix = [np.where(inside, a, 0).astype(np.int64) for a in c]
    bit = inside & (blurred[ix[1], ix[0]] < blurred[ix[3], ix[2]])
    words = np.zeros((len(pts), (nbits + 31) // 32), np.uint32)
    for i in range(nbits):
        words[:, i >> 5] |= bit[:, i].astype(np.uint32) << np.uint32(i & 31)
    return words


def hamming(a, b):
    """[m, k] x [n, k] uint32 -> int32 [m, n]."""
    x = (a[:, None, :] ^ b[None, :, :]).view(np.uint8)
    return _POP8[x].sum(-1).astype(np.int32)


def search_by_brief(win_desc, old_desc, old_kp, old_norm):
    """Item 6: searchByBRIEFDes -> status u8 [m], index i32 [m] (-1: no distance below 128), distance i32 [m] (128 then),
    old pixel f32 [m, 2], old normalised point f32 [m, 2] ((0, 0) when unmatched), count."""
    m = len(win_desc)
    status = np.zeros(m, np.uint8); index = np.full(m, -1, np.int32); dist = np.full(m, MATCH_START, np.int32)
    uv = np.zeros((m, 2), np.float32); nm = np.zeros((m, 2), np.float32)
    if m and len(old_desc):
        d = hamming(np.asarray(win_desc, np.uint32), np.asarray(old_desc, np.uint32))
        for i in range(m):
            best, at = MATCH_START, -1
            row = d[i]
            lo = int(row.min())
            if lo < best:
                best, at = lo, int(np.nonzero(row == lo)[0][0])
            index[i] = at; dist[i] = best
            if at != -1 and best < MATCH_LIMIT:
                status[i] = 1; uv[i] = old_kp[at]; nm[i] = old_norm[at]
    return status, index, dist, uv, nm, int(status.sum())


class KeyFrameRef:
    """One keyframe: FAST keypoints, their normalised points and descriptors, the window points' descriptors."""

    def __init__(self, cam, pattern, image, window_uv, threshold=FAST_THRESHOLD):
        self.grey = grey_of(image)
        assert self.grey.shape == (cam.height, cam.width)
        self.blur = blur(self.grey)
        self.score = fast_score(self.grey, threshold)
        self.keypoints = fast_keypoints(self.score)
        self.norm = np.array([cam.lift(x, y) for x, y in self.keypoints], np.float32).reshape(-1, 2)
        self.descriptors = brief(self.blur, self.keypoints, pattern)
        self.window_uv = np.asarray(window_uv, np.float32).reshape(-1, 2)
        self.window_descriptors = brief(self.blur, self.window_uv, pattern)

    def match(self, old):
        return search_by_brief(self.window_descriptors, old.descriptors, old.keypoints, old.norm)
