"""tests/keyframe_ref.py (the CPU restatement of DESIGN.md 6f) against things that are not the restatement: a brute-force FAST written
with explicit loops, scipy's correlate1d, hand-built BRIEF cases, unpackbits distances, and the known flow of workloads/s5."""
import os

import numpy as np
import pytest

from tests import keyframe_ref as K
from tests import track_ref as R
from workloads import s5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")


def _pattern():
    import lmono_amd
    return lmono_amd.load_brief_pattern(PATTERN_FILE)


# ---- FAST ----------------------------------------------------------------------------------------------------------------------

def _fires(img, x, y, t):
    """The 9-arc test with explicit loops at threshold t."""
    v = int(img[y, x])
    c = [int(img[y + dy, x + dx]) for dx, dy in K.CIRCLE]
    for start in range(16):
        brighter = darker = True
        for k in range(9):
            q = c[(start + k) % 16]
            if not v - q > t:
                brighter = False
            if not q - v > t:
                darker = False
        if brighter or darker:
            return True
    return False


def _brute_score(img, threshold):
    """Per pixel the largest t' in 0..255 at which the 9-arc test still fires; a corner iff it fires at `threshold`."""
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if not _fires(img, x, y, threshold):
                continue
            best = threshold
            for t in range(threshold + 1, 256):
                if not _fires(img, x, y, t):
                    break
                best = t
            out[y, x] = best
    return out


def _brute_keypoints(score):
    h, w = score.shape
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            s = score[y, x]
            if s > 0 and all(s > score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                out.append((x, y))
    return np.array(out, np.float32).reshape(-1, 2)


@pytest.mark.parametrize("which", ["random", "s5"])
def test_fast_equals_brute_force(which):
    if which == "random":
        rng = np.random.default_rng(7)
        img = rng.integers(0, 256, (40, 56), dtype=np.uint8)
        img[10:30, 8:40] = (img[10:30, 8:40] // 8 + 100).astype(np.uint8)       # a calmer patch: fewer, weaker corners
    else:
        img = s5.Sequence(320, 240, 1, seed=2).frames[0][60:130, 100:200]
    score = K.fast_score(img, 20)
    brute = _brute_score(img, 20)
    assert np.array_equal(score.astype(np.int32), brute)
    assert (score > 0).sum() > 10
    kp = K.fast_keypoints(score)
    assert np.array_equal(kp, _brute_keypoints(brute))
    assert len(kp) > 3
    assert (np.diff(kp[:, 1] * 10000 + kp[:, 0]) > 0).all()           # row-major


def test_fast_known_answers():
    flat = np.full((32, 32), 90, np.uint8)
    assert not K.fast_score(flat).any()
    dot = np.full((32, 32), 10, np.uint8); dot[16, 16] = 200
    s = K.fast_score(dot)
    assert (s > 0).sum() == 1 and s[16, 16] == 200 - 10 - 1              # every arc differs by 190: A = 190, score A - 1
    assert np.array_equal(K.fast_keypoints(s), np.array([[16, 16]], np.float32))
    # a bright quadrant: its apex is a corner (12 of 16 circle pixels are darker), its straight edges are not (at most 8 contiguous ones)
    quad = np.full((48, 48), 20, np.uint8); quad[24:, 24:] = 220
    s = K.fast_score(quad)
    assert s[24, 24] > 0
    assert not s[24, 34:44].any() and not s[34:44, 24].any() and not s[23, 34:44].any() and not s[34:44, 23].any()
    # nothing within 3 pixels of the border
    rng = np.random.default_rng(1)
    s = K.fast_score(rng.integers(0, 256, (30, 41), dtype=np.uint8))
    assert s[3:-3, 3:-3].any()
    assert not s[:3].any() and not s[-3:].any() and not s[:, :3].any() and not s[:, -3:].any()
    # two adjacent corners of equal score both vanish under the strict test
    pair = np.full((32, 32), 10, np.uint8); pair[16, 15] = 200; pair[16, 16] = 200
    s = K.fast_score(pair)
    assert s[16, 15] > 0 and s[16, 15] == s[16, 16]
    kp = K.fast_keypoints(s)
    assert not any((kp == np.array([15, 16], np.float32)).all(1)) and not any((kp == np.array([16, 16], np.float32)).all(1))


# ---- blur ----------------------------------------------------------------------------------------------------------------------

def test_blur_weights_and_scipy():
    from scipy.ndimage import correlate1d
    g = np.exp(-np.arange(-4, 5) ** 2 / 8.0)
    wts = np.rint(256.0 * g / g.sum()).astype(np.int64)
    assert np.array_equal(wts, K.BLUR_WEIGHTS) and wts.sum() == 256
    rng = np.random.default_rng(3)
    for img in (rng.integers(0, 256, (37, 53), dtype=np.uint8), s5.Sequence(320, 240, 1, seed=5).frames[0], np.full((20, 20), 255, np.uint8)):
        rows = correlate1d(img.astype(np.int64), wts, axis=1, mode="mirror")
        cols = correlate1d(rows, wts, axis=0, mode="mirror")
        assert np.array_equal(K.blur(img), ((cols + 32768) >> 16).astype(np.uint8))
    assert (K.blur(np.full((20, 20), 255, np.uint8)) == 255).all()


# ---- BRIEF ---------------------------------------------------------------------------------------------------------------------

def test_brief_toy_pattern_bits_and_layout():
    img = np.zeros((64, 64), np.uint8)
    img[:, 32:] = 200                                  # dark left half, bright right half
    toy = (np.array([-5, 5, 0, -5]), np.array([0, 0, -3, 0]), np.array([5, -5, 0, -4]), np.array([0, 0, 3, 0]))
    # at (32, 20): test 0 compares (27, 20) = 0 < (37, 20) = 200 -> 1; test 1 the reverse -> 0; test 2 equal columns -> 0; test 3 0 < 0 -> 0
    d = K.brief(img, np.array([[32.0, 20.0]], np.float32), toy)
    assert d.shape == (1, 1) and d[0, 0] == 0b0001
    # at (35, 20): test 3 compares (30, 20) = 0 < (31, 20) = 0 -> 0; at (36, 20): (31, 20) = 0 < (32, 20) = 200 -> 1
    assert K.brief(img, np.array([[35.0, 20.0]], np.float32), toy)[0, 0] == 0b0001
    assert K.brief(img, np.array([[36.0, 20.0]], np.float32), toy)[0, 0] == 0b1001
    # word layout: bit i is bit i & 31 of word i >> 5
    n = 70
    pat = (np.full(n, -5), np.zeros(n, np.int64), np.full(n, 5), np.zeros(n, np.int64))
    pat[0][[0, 33, 69]] = 5; pat[2][[0, 33, 69]] = -5            # these three tests read bright < dark: 0
    d = K.brief(img, np.array([[32.0, 20.0]], np.float32), pat)
    assert d.shape == (1, 3)
    assert d[0, 0] == 0xFFFFFFFE and d[0, 1] == 0xFFFFFFFF & ~(1 << 1) and d[0, 2] == 0b011111


def test_brief_truncation_and_range():
    img = np.zeros((64, 64), np.uint8)
    img[:, 0] = 10; img[:, 1:] = 50
    # x = 0.4 with offset -1: (int)(-0.6) = 0, in range, reads column 0 (10) < column 5 (50) -> 1
    pat = (np.array([-1]), np.array([0]), np.array([5]), np.array([0]))
    assert K.brief(img, np.array([[0.4, 30.0]], np.float32), pat)[0, 0] == 1
    # x = -1.2 with offset 0: (int)(-1.2) = -1, out of range -> 0
    pat0 = (np.array([0]), np.array([0]), np.array([5]), np.array([0]))
    assert K.brief(img, np.array([[-1.2, 30.0]], np.float32), pat0)[0, 0] == 0
    assert K.brief(img, np.array([[-0.7, 30.0]], np.float32), pat0)[0, 0] == 1          # (int)(-0.7) = 0
    # every bit whose sample leaves the image is 0: compare with a run on an image padded so that nothing leaves
    rng = np.random.default_rng(4)
    big = rng.integers(0, 256, (200, 220), dtype=np.uint8)
    small = np.ascontiguousarray(big[70:130, 70:150])
    pat = _pattern()
    pts = np.stack([rng.uniform(-2, 82, 300), rng.uniform(-2, 62, 300)], 1).astype(np.float32)
    ds = K.brief(small, pts, pat)
    db = K.brief(big, pts + np.float32(70.0), pat)          # compared below only where the shifted coordinates truncate alike
    x1, y1, x2, y2 = (a.astype(np.float32)[None] for a in pat)
    c = [np.trunc(pts[:, 0:1] + x1), np.trunc(pts[:, 1:2] + y1), np.trunc(pts[:, 0:1] + x2), np.trunc(pts[:, 1:2] + y2)]
    inside = (c[0] >= 0) & (c[0] < 80) & (c[2] >= 0) & (c[2] < 80) & (c[1] >= 0) & (c[1] < 60) & (c[3] >= 0) & (c[3] < 60)
    bits = ((ds[:, np.arange(256) >> 5] >> (np.arange(256) & 31).astype(np.uint32)) & 1).astype(bool)
    assert not bits[~inside].any() and (~inside).sum() > 1000
    # where nothing leaves and the shifted coordinates truncate alike, the descriptor bits are those of the padded image
    cb = [np.trunc(pts[:, 0:1] + np.float32(70.0) + x1), np.trunc(pts[:, 1:2] + np.float32(70.0) + y1),
          np.trunc(pts[:, 0:1] + np.float32(70.0) + x2), np.trunc(pts[:, 1:2] + np.float32(70.0) + y2)]
    alike = inside & np.logical_and.reduce([cb[k] == c[k] + 70 for k in range(4)])
    bits_b = ((db[:, np.arange(256) >> 5] >> (np.arange(256) & 31).astype(np.uint32)) & 1).astype(bool)
    assert np.array_equal(bits[alike], bits_b[alike]) and alike.sum() > 10000


# ---- match ---------------------------------------------------------------------------------------------------------------------

def _unpack_dist(a, b):
    ab = np.unpackbits(a.view(np.uint8), axis=1).astype(np.int32); bb = np.unpackbits(b.view(np.uint8), axis=1).astype(np.int32)
    return (ab[:, None, :] != bb[None, :, :]).sum(-1)


def test_match_equals_unpackbits_argmin():
    rng = np.random.default_rng(5)
    old = rng.integers(0, 2 ** 32, (300, 8), dtype=np.uint64).astype(np.uint32)
    cur = old[rng.integers(0, 300, 120)].copy()
    for i in range(120):                                     # flip 0..140 random bits
        for b in rng.choice(256, int(rng.integers(0, 141)), replace=False):
            cur[i, b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    old[17] = old[3]                                         # a tie: the lowest index wins
    kp = rng.uniform(0, 300, (300, 2)).astype(np.float32); nm = rng.uniform(-1, 1, (300, 2)).astype(np.float32)
    st, ix, di, uv, nrm, count = K.search_by_brief(cur, old, kp, nm)
    d = _unpack_dist(cur, old)
    am = d.argmin(1); dm = d.min(1)
    found = dm < 128
    assert np.array_equal(ix[found], am[found]) and (ix[~found] == -1).all()
    assert np.array_equal(di, np.minimum(dm, 128))
    assert np.array_equal(st.astype(bool), dm < 80) and count == int((dm < 80).sum()) and 0 < count < 120
    assert np.array_equal(uv[st == 1], kp[am[st == 1]]) and np.array_equal(nrm[st == 1], nm[am[st == 1]])
    assert not uv[st == 0].any() and not nrm[st == 0].any()
    assert 17 not in ix


@pytest.mark.parametrize("flips,status,index,dist", [(79, 1, 0, 79), (80, 0, 0, 80), (127, 0, 0, 127), (128, 0, -1, 128), (200, 0, -1, 128)])
def test_match_limits(flips, status, index, dist):
    base = np.zeros((1, 8), np.uint32)
    other = np.zeros((1, 8), np.uint32)
    for b in range(flips):
        other[0, b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    st, ix, di, uv, nm, count = K.search_by_brief(other, base, np.array([[7.0, 9.0]], np.float32), np.array([[0.5, 0.25]], np.float32))
    assert (int(st[0]), int(ix[0]), int(di[0]), count) == (status, index, dist, status)
    assert tuple(uv[0]) == ((7.0, 9.0) if status else (0.0, 0.0)) and tuple(nm[0]) == ((0.5, 0.25) if status else (0.0, 0.0))
    # no old descriptors at all
    st, ix, di, uv, nm, count = K.search_by_brief(other, np.zeros((0, 8), np.uint32), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert (int(st[0]), int(ix[0]), int(di[0]), count) == (0, -1, 128, 0)


# ---- pattern parser ------------------------------------------------------------------------------------------------------------

def test_pattern_parser(tmp_path):
    import lmono_amd
    pat = _pattern()
    assert pat.shape == (4, 256) and np.abs(pat).max() <= 63 and np.issubdtype(pat.dtype, np.integer)
    assert pat[0, :5].tolist() == [0, 4, 11, -4, 24]
    lines = open(PATTERN_FILE).read().split("\n")
    bad = tmp_path / "short.yml"
    bad.write_text("\n".join(lines[:100] + lines[101:]))               # one entry of x1 missing
    with pytest.raises(lmono_amd.LmonoError, match="exactly 256"):
        lmono_amd.load_brief_pattern(str(bad))
    bad.write_text("\n".join(l for l in lines if not l.startswith("y2")))     # a key missing: its entries run into x2
    with pytest.raises(lmono_amd.LmonoError, match="exactly 256"):
        lmono_amd.load_brief_pattern(str(bad))
    bad.write_text("\n".join(lines[:50] + ["  - four"] + lines[50:]))
    with pytest.raises(lmono_amd.LmonoError, match="not an integer"):
        lmono_amd.load_brief_pattern(str(bad))


# ---- physical: keyframes of a sequence with known flow -------------------------------------------------------------------------

W, H = 320, 240
DELTA = 6
# r: a match is correct when the matched old keypoint lies within R_PX of the window point's true position in the old frame.  R_PX comes
# from the spacing of the FAST keypoints: the median distance from a keypoint of these frames to its nearest neighbour is 5 px, and
# within half of that, 2.5 px, of a position there is as a rule one keypoint only, so "the keypoint at the true position" is unambiguous.
# The test checks the spacing it relies on.
R_PX = 2.5


def _sequence_keyframes(seq, k0, k1):
    cam = R.Camera(W, H, 0.9 * W, 0.9 * W * 1.01, 0.5 * W - 3.0, 0.5 * H + 2.0)
    trk = R.TrackerRef(cam, 150, 15)
    rec = None
    for k in range(k1 + 1):
        rec = trk.track(0.1 * k, seq.frames[k])
    uv = np.stack([rec["u"], rec["v"]], 1).astype(np.float32)
    pat = _pattern()
    old = K.KeyFrameRef(cam, pat, seq.frames[k0], np.zeros((0, 2), np.float32))
    cur = K.KeyFrameRef(cam, pat, seq.frames[k1], uv)
    return old, cur, uv


def _shares(seq, k0, k1):
    old, cur, uv = _sequence_keyframes(seq, k0, k1)
    st, ix, di, muv, _, count = cur.match(old)
    truth = seq.flow(k1, k0, uv)
    visible = (truth[:, 0] >= 0) & (truth[:, 0] < W) & (truth[:, 1] >= 0) & (truth[:, 1] < H)
    err = np.hypot(muv[:, 0] - truth[:, 0], muv[:, 1] - truth[:, 1])
    matched = st == 1
    wrong = int((matched & ~(err <= R_PX)).sum())
    kp = old.keypoints
    d = np.hypot(kp[:, None, 0] - kp[None, :, 0], kp[:, None, 1] - kp[None, :, 1])
    np.fill_diagonal(d, np.inf)
    assert np.median(d.min(1)) >= 2 * R_PX
    return count, len(uv), int(visible.sum()), wrong


# measured on the restatement (written into DESIGN.md 6f), r = 2.5 px: translation: 150 window points, 145 matched, 35 wrong (24.1 %);
# rotation + zoom: 150 window points, 149 matched, 40 wrong (26.8 %).  Most wrong matches are far from the truth (> 50 px): a window point
# without a FAST keypoint on it still finds some descriptor below 80 among ~700, which is what PnPRANSAC removes in the reference.
# The asserted error share is twice the measured one.
@pytest.mark.parametrize("motion,max_wrong_share", [("translation", 0.482), ("rot_zoom", 0.536)])
def test_matches_follow_the_known_flow(motion, max_wrong_share):
    if motion == "translation":
        seq = s5.Sequence(W, H, DELTA + 3, seed=1, step=(1.5, 0.5))
    else:
        seq = s5.Sequence(W, H, DELTA + 3, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001)      # the rotation + zoom case of 6e
    count, n, visible, wrong = _shares(seq, 2, 2 + DELTA)
    print("%s: %d window points, %d visible in the old frame, %d matched, %d wrong (share %.3f)" % (motion, n, visible, count, wrong, wrong / max(count, 1)))
    assert count > K.MIN_BRIEF_LOOP_NUM
    assert wrong / count <= max_wrong_share


def test_frames_of_two_worlds():
    """Frames of two different s5 worlds.  The restatement does NOT separate this case from a true revisit by the match count: measured
    137 of 150 window points matched (a true revisit: 145), far above MIN_BRIEF_LOOP_NUM = 25 -- the minimum over ~700 descriptors of a
    256-bit distance is below 80 for almost any query on these textures.  The count gate alone is no loop test (the reference follows it
    with PnPRANSAC); DESIGN.md 6f says so.  What the restatement does show, and what is asserted: the matched distances of a true
    revisit are smaller (medians compared, no threshold)."""
    a = s5.Sequence(W, H, DELTA + 3, seed=1, step=(1.5, 0.5))
    b = s5.Sequence(W, H, 3, seed=2, step=(1.5, 0.5))
    cam = R.Camera(W, H, 0.9 * W, 0.9 * W * 1.01, 0.5 * W - 3.0, 0.5 * H + 2.0)
    old, cur, _ = _sequence_keyframes(a, 2, 2 + DELTA)
    other = K.KeyFrameRef(cam, _pattern(), b.frames[2], np.zeros((0, 2), np.float32))
    st_o, _, di_o, _, _, count_o = cur.match(other)
    st_s, _, di_s, _, _, count_s = cur.match(old)
    print("two worlds: %d matched, median distance %.1f; same world: %d matched, median distance %.1f"
          % (count_o, np.median(di_o[st_o == 1]), count_s, np.median(di_s[st_s == 1])))
    assert np.median(di_s[st_s == 1]) < np.median(di_o[st_o == 1])
