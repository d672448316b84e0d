"""Device keyframe descriptors (lmono_keyframes_*) against the CPU restatement tests/keyframe_ref.py: equal bytes."""
import os

import numpy as np
import pytest

from tests import keyframe_ref as K
from tests import track_ref as R
from workloads import s5, s6

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")


def _pattern():
    import lmono_amd
    return lmono_amd.load_brief_pattern(PATTERN_FILE)


def _cam(w, h, dist=(0.0, 0.0, 0.0, 0.0)):
    import lmono_amd
    fx = 0.9 * w
    return (lmono_amd.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, dist[0], dist[1], dist[2], dist[3], 5, 0, 0),
            R.Camera(w, h, fx, fx * 1.01, 0.5 * w - 3.0, 0.5 * h + 2.0, *dist))


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def _window_points(w, h, n, seed):
    """Fractional positions all over the image, some within a pattern's reach of the border, a few on and just outside it."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1)
    pts[:8] = [(0.4, 0.4), (-0.6, 5.0), (w - 0.5, h - 0.5), (w + 2.0, 10.0), (3.25, h - 1.0), (-1.2, -1.2), (w - 1.0, 0.0), (0.0, h + 70.0)]
    pts[8:24, 0] = rng.uniform(-2, 30, 16); pts[24:40, 1] = rng.uniform(h - 30, h + 2, 16)
    return pts.astype(np.float32)


def _error_code(exc):
    return int(str(exc.value).split("lmono error ")[1].split(":")[0])


def _check_keyframe(got, ref, what):
    _same(got["keypoints"], ref.keypoints, what + ": keypoints (position and order)")
    _same(got["norm"], ref.norm, what + ": normalised keypoints")
    _same(got["descriptors"], ref.descriptors, what + ": descriptors")
    _same(got["window_uv"], ref.window_uv, what + ": window points")
    _same(got["window_descriptors"], ref.window_descriptors, what + ": window descriptors")


def _case(name):
    if name == "s5_320x240":
        return s5.Sequence(320, 240, 1, seed=1).frames[0], (0.0, 0.0, 0.0, 0.0)
    if name == "s6_640x480":
        return s6.Sequence(640, 480, 1, seed=2).frames[0], (-0.28, 0.07, 0.0002, -0.0003)
    if name == "synthetic_1241x376":
        return s5.Sequence(1241, 376, 1, seed=3, margin=8).frames[0], (0.0, 0.0, 0.0, 0.0)
    if name == "bgr_320x240":
        return s5.bgr_of(s5.Sequence(320, 240, 1, seed=4).frames[0], seed=4), (0.0, 0.0, 0.0, 0.0)
    assert name == "odd_333x251"              # neither side a multiple of the 64 x 16 tile
    return s5.Sequence(333, 251, 1, seed=5).frames[0], (-0.1, 0.02, 0.0, 0.0)


@pytest.mark.parametrize("name", ["s5_320x240", "s6_640x480", "synthetic_1241x376", "bgr_320x240", "odd_333x251"])
def test_keyframe_equals_restatement(gpu_ctx, name):
    import lmono_amd
    img, dist = _case(name)
    h, w = img.shape[:2]
    gc, rc = _cam(w, h, dist)
    pat = _pattern()
    uv = _window_points(w, h, 150, 11)
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 16384)
    idx, nkp = kf.add(img, uv)
    ref = K.KeyFrameRef(rc, pat, img, uv)
    blur, score = kf.images()
    _same(blur, ref.blur, "blurred image")
    _same(score, ref.score, "score image")
    assert idx == 0 and nkp == len(ref.keypoints) and nkp > 100 and len(kf) == 1
    _check_keyframe(kf.get(0), ref, name)
    kf.close()


def test_fast_threshold_argument(gpu_ctx):
    import lmono_amd
    img = s5.Sequence(320, 240, 1, seed=6).frames[0]
    gc, rc = _cam(320, 240)
    pat = _pattern()
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 2, 16384, fast_threshold=35)
    kf.add(img, np.zeros((0, 2), np.float32))
    ref = K.KeyFrameRef(rc, pat, img, np.zeros((0, 2), np.float32), threshold=35)
    _same(kf.images()[1], ref.score, "score image at threshold 35")
    _check_keyframe(kf.get(0), ref, "threshold 35, no window points")
    assert 0 < len(ref.keypoints) < len(K.fast_keypoints(K.fast_score(img, 20)))
    kf.close()


def _random_old(rng, n):
    return (rng.uniform(0, 300, (n, 2)).astype(np.float32), rng.uniform(-1, 1, (n, 2)).astype(np.float32),
            rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32))


def _check_match(got, cur_desc, olds):
    for o, (kp, nm, de) in enumerate(olds):
        st, ix, di, uv, nrm, count = K.search_by_brief(cur_desc, de, kp, nm)
        what = "old keyframe %d (%d keypoints)" % (o, len(kp))
        _same(got["status"][o], st, what + ": status"); _same(got["index"][o], ix, what + ": index"); _same(got["dist"][o], di, what + ": distance")
        _same(got["old_uv"][o], uv, what + ": old pixel"); _same(got["old_norm"][o], nrm, what + ": old normalised point")
        assert got["counts"][o] == count, what


@pytest.mark.parametrize("n_window", [150, 300, 512])
def test_match_equals_restatement(gpu_ctx, n_window):
    import lmono_amd
    rng = np.random.default_rng(20 + n_window)
    gc, _ = _cam(320, 240)
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, _pattern(), 70, 1500)
    sizes = [700, 0, 1, 255, 256, 257, 1500] + [int(v) for v in rng.integers(2, 900, 57)]
    olds = [_random_old(rng, n) for n in sizes]
    # the window descriptors: old descriptors of several keyframes with 1..140 flipped bits
    cur = np.zeros((n_window, 8), np.uint32)
    for i in range(n_window):
        src = olds[[0, 6, 3, 10][i % 4]][2]
        cur[i] = src[rng.integers(0, len(src))]
        for b in rng.choice(256, int(rng.integers(1, 141)), replace=False):
            cur[i, b >> 5] ^= np.uint32(1) << np.uint32(b & 31)
    # constructed ties: copies of a matched descriptor at higher indices, within a 256-share and across shares
    olds[0][2][5] = cur[0]; olds[0][2][40] = cur[0]; olds[0][2][300] = cur[0]; olds[0][2][699] = cur[0]
    olds[6][2][1400] = cur[1]; olds[6][2][100] = cur[1]
    for kp, nm, de in olds:
        kf.load(kp, nm, de)
    uv = rng.uniform(0, 300, (n_window, 2)).astype(np.float32)
    ci = kf.load(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 8), np.uint32), uv, cur)
    assert ci == 64 and len(kf) == 65
    for n_old in (1, 4, 64):
        got = kf.match(ci, list(range(n_old)))
        assert got["status"].shape == (n_old, n_window)
        _check_match(got, cur, olds[:n_old])
        assert got["index"][0][0] == 5 and got["dist"][0][0] == 0             # the tie went to the lowest index
        if n_old >= 2:
            assert not got["status"][1].any() and (got["index"][1] == -1).all() and (got["dist"][1] == 128).all() and got["counts"][1] == 0
    got = kf.match(ci, [6, 0, 6])                                                  # any order, repeats allowed
    _check_match(got, cur, [olds[6], olds[0], olds[6]])
    assert got["index"][0][1] == 100
    assert 0 < got["counts"][1] < n_window
    kf.close()


def test_match_distance_limits(gpu_ctx):
    """Distances of 79, 80, 127, 128 and 200 against a one-descriptor keyframe: matched below 80, found below 128, nothing at 128."""
    import lmono_amd
    gc, _ = _cam(320, 240)
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, _pattern(), 4, 16)
    old = (np.array([[7.0, 9.0]], np.float32), np.array([[0.5, 0.25]], np.float32), np.zeros((1, 8), np.uint32))
    kf.load(*old)
    flips = [79, 80, 127, 128, 200, 0]
    cur = np.zeros((len(flips), 8), np.uint32)
    for i, n in enumerate(flips):
        for b in range(n):
            cur[i, b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    ci = kf.load(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 8), np.uint32), np.zeros((len(flips), 2), np.float32), cur)
    got = kf.match(ci, [0])
    _check_match(got, cur, [old])
    assert got["status"][0].tolist() == [1, 0, 0, 0, 0, 1] and got["index"][0].tolist() == [0, 0, 0, -1, -1, 0]
    assert got["dist"][0].tolist() == [79, 80, 127, 128, 128, 0] and got["counts"][0] == 2
    kf.close()


def test_match_with_zero_keypoint_image(gpu_ctx):
    """An old keyframe whose image has no corner at all, added through the image path."""
    import lmono_amd
    gc, rc = _cam(320, 240)
    pat = _pattern()
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 4096)
    flat = np.full((240, 320), 77, np.uint8)
    assert kf.add(flat, np.zeros((0, 2), np.float32)) == (0, 0)
    img = s5.Sequence(320, 240, 1, seed=7).frames[0]
    uv = _window_points(320, 240, 100, 3)
    kf.add(img, uv)
    got = kf.match(1, [0, 1])
    ref_flat = K.KeyFrameRef(rc, pat, flat, np.zeros((0, 2), np.float32)); ref = K.KeyFrameRef(rc, pat, img, uv)
    _check_match(got, ref.window_descriptors, [(ref_flat.keypoints, ref_flat.norm, ref_flat.descriptors), (ref.keypoints, ref.norm, ref.descriptors)])
    assert got["counts"][0] == 0 and got["counts"][1] > 0
    assert kf.match(0, [1])["status"].shape == (1, 0)                             # a current keyframe without window points
    kf.close()


def test_add_batch_equals_single_streams(gpu_ctx):
    import torch
    import lmono_amd
    n = 8
    pat = _pattern()
    seqs = [s5.Sequence(320, 240, 8, seed=30 + s, step=(1.5 + 0.2 * s, 0.5), rot_step=0.001 * s) for s in range(n)]
    gc, rc = _cam(320, 240)
    batch = [lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192) for _ in range(n)]
    single = [lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192) for _ in range(n)]
    for f in (0, 7):
        uvs = [_window_points(320, 240, 60 + 20 * s, 100 * f + s) for s in range(n)]
        imgs = [torch.from_numpy(np.ascontiguousarray(seqs[s].frames[f])).to("cuda:0") for s in range(n)]
        idx, nkp = lmono_amd.KeyFrames.add_batch(batch, [t.data_ptr() for t in imgs], uvs)
        for s in range(n):
            i1, n1 = single[s].add(seqs[s].frames[f], uvs[s])
            assert (idx[s], nkp[s]) == (i1, n1)
            a, b = batch[s].get(i1), single[s].get(i1)
            for key in a:
                _same(a[key], b[key], "stream %d frame %d: %s" % (s, f, key))
            for x, y in zip(batch[s].images(), single[s].images()):
                _same(x, y, "stream %d frame %d: work image" % (s, f))
        if f == 7:
            ref = K.KeyFrameRef(rc, pat, seqs[3].frames[7], uvs[3])
            _check_keyframe(batch[3].get(1), ref, "stream 3 against the restatement")
    # match against n old keyframes == n single matches
    for s in (0, 5):
        both = batch[s].match(1, [0, 1])
        for o in (0, 1):
            one = single[s].match(1, [o])
            for key in both:
                _same(both[key][o], one[key][0], "stream %d: match output %s against old keyframe %d" % (s, key, o))
    for k in batch + single:
        k.close()


def test_capacity_and_bad_arguments(gpu_ctx):
    import lmono_amd
    gc, rc = _cam(320, 240)
    pat = _pattern()
    img = s5.Sequence(320, 240, 1, seed=8).frames[0]
    uv = _window_points(320, 240, 50, 9)
    ref = K.KeyFrameRef(rc, pat, img, uv)
    n = len(ref.keypoints)
    assert n > 100
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 2, n)             # exactly enough
    assert kf.add(img, uv) == (0, n)
    before = kf.get(0)
    kf.close()
    kf = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 2, n - 1)         # one too few: refused, nothing truncated
    flat = np.full((240, 320), 50, np.uint8)
    kf.add(flat, uv[:3])
    kept = kf.get(0)
    with pytest.raises(lmono_amd.LmonoError) as e:
        kf.add(img, uv)
    assert _error_code(e) == -4 and kf.last_n_keypoints == n and len(kf) == 1
    after = kf.get(0)
    for key in kept:
        _same(kept[key], after[key], "the store after a refused image: " + key)
    with pytest.raises(lmono_amd.LmonoError):
        kf.get(1)
    assert kf.add(flat, uv) == (1, 0)                            # the store still works, and is now full
    with pytest.raises(lmono_amd.LmonoError) as e:
        kf.add(flat, uv)
    assert _error_code(e) == -4 and len(kf) == 2
    with pytest.raises(lmono_amd.LmonoError) as e:
        kf.load(before["keypoints"], before["norm"], before["descriptors"])
    assert _error_code(e) == -4
    kf.clear()
    assert len(kf) == 0
    with pytest.raises(lmono_amd.LmonoError) as e:               # more keypoints than a slot holds
        kf.load(before["keypoints"], before["norm"], before["descriptors"])
    assert _error_code(e) == -4 and len(kf) == 0
    kf.add(flat, uv)
    for bad in (lambda: kf.match(0, []), lambda: kf.match(1, [0]), lambda: kf.match(0, [3]), lambda: kf.match(0, [-1]),
                lambda: kf.add(flat, np.zeros((513, 2), np.float32))):
        with pytest.raises(lmono_amd.LmonoError) as e:
            bad()
        assert _error_code(e) == -1
    kf.close()
    bad_pat = pat.copy(); bad_pat[2, 17] = 64
    with pytest.raises(lmono_amd.LmonoError, match="outside -63..63"):
        lmono_amd.KeyFrames(gpu_ctx, gc, bad_pat, 2, 100)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.KeyFrames(gpu_ctx, gc, pat, 2, 65536)
    with pytest.raises(lmono_amd.LmonoError):
        lmono_amd.KeyFrames(gpu_ctx, gc, pat, 0, 100)


def test_load_then_match_equals_add_then_match(gpu_ctx):
    import lmono_amd
    gc, rc = _cam(320, 240)
    pat = _pattern()
    seq = s5.Sequence(320, 240, 7, seed=1, step=(1.5, 0.5))
    trk = R.TrackerRef(rc, 150, 15)
    rec = [trk.track(0.1 * k, seq.frames[k]) for k in range(7)]
    uv0 = np.stack([rec[0]["u"], rec[0]["v"]], 1); uv6 = np.stack([rec[6]["u"], rec[6]["v"]], 1)
    a = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192)
    a.add(seq.frames[0], uv0); a.add(seq.frames[6], uv6)
    b = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192)
    for i in (0, 1):
        g = a.get(i)
        assert b.load(g["keypoints"], g["norm"], g["descriptors"], g["window_uv"], g["window_descriptors"]) == i
        h = b.get(i)
        for key in g:
            _same(g[key], h[key], "loaded keyframe %d: %s" % (i, key))
    ma, mb = a.match(1, [0]), b.match(1, [0])
    for key in ma:
        _same(ma[key], mb[key], "match output " + key)
    ref0 = K.KeyFrameRef(rc, pat, seq.frames[0], uv0); ref6 = K.KeyFrameRef(rc, pat, seq.frames[6], uv6)
    _check_match(ma, ref6.window_descriptors, [(ref0.keypoints, ref0.norm, ref0.descriptors)])
    a.close(); b.close()


def test_add_batch_one_stream_refused(gpu_ctx):
    """When one stream of a batch is over capacity no store advances: the others keep their keyframes and take the next add."""
    import torch
    import lmono_amd
    gc, rc = _cam(320, 240)
    pat = _pattern()
    seq = s5.Sequence(320, 240, 3, seed=9)
    uv = _window_points(320, 240, 40, 5)
    n = len(K.KeyFrameRef(rc, pat, seq.frames[1], uv).keypoints)
    stores = [lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192), lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, n - 1), lmono_amd.KeyFrames(gpu_ctx, gc, pat, 4, 8192)]
    flat = np.full((240, 320), 60, np.uint8)
    first = [seq.frames[0], flat, seq.frames[0]]
    for s, img in zip(stores, first):
        s.add(img, uv)
    before = [s.get(0) for s in stores]
    dev = [torch.from_numpy(np.ascontiguousarray(seq.frames[1])).to("cuda:0") for _ in stores]
    with pytest.raises(lmono_amd.LmonoError) as e:
        lmono_amd.KeyFrames.add_batch(stores, [t.data_ptr() for t in dev], [uv] * 3)
    assert _error_code(e) == -4
    assert [len(s) for s in stores] == [1, 1, 1] and [s.last_n_keypoints for s in stores] == [n, n, n]
    for s, b in zip(stores, before):
        a = s.get(0)
        for key in b:
            _same(a[key], b[key], "keyframe 0 after a refused batch: " + key)
        with pytest.raises(lmono_amd.LmonoError):
            s.get(1)
    # a later add works and gives what a fresh store gives
    dev2 = [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in (seq.frames[2], flat, seq.frames[2])]
    idx, nkp = lmono_amd.KeyFrames.add_batch(stores, [t.data_ptr() for t in dev2], [uv[:20]] * 3)
    assert idx.tolist() == [1, 1, 1] and nkp[1] == 0
    ref = K.KeyFrameRef(rc, pat, seq.frames[2], uv[:20])
    _check_keyframe(stores[0].get(1), ref, "the add after a refused batch")
    _check_keyframe(stores[2].get(1), ref, "the add after a refused batch")
    _check_match(stores[0].match(1, [0, 1]), ref.window_descriptors,
                 [(before[0]["keypoints"], before[0]["norm"], before[0]["descriptors"]), (ref.keypoints, ref.norm, ref.descriptors)])
    for s in stores:
        s.close()


def test_host_mirror_keyframe_test_equals_python_path(gpu_ctx, tmp_path):
    """lmono_amd/host/keyframe_test: tracker frames of an s5 sequence -> KeyFrame of frame k and of frame k + delta -> findConnection up to
    the MIN_BRIEF_LOOP_NUM gate; its printed matches equal the Python path's on the same frames."""
    import subprocess
    import lmono_amd
    exe = os.path.join(ROOT, "lmono_amd", "host", "keyframe_test")
    assert os.path.exists(exe), "build() makes lmono_amd/host/keyframe_test"
    w, h, k, delta = 320, 240, 2, 6
    seq = s5.Sequence(w, h, k + delta + 1, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001)
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(("%d %d %d\n" % (w, h, len(seq.frames))).encode())
        for img in seq.frames:
            f.write(np.ascontiguousarray(img).tobytes())
    res = subprocess.run([exe, str(raw), PATTERN_FILE, str(k), str(delta)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    # the Python path with the camera and limits of keyframe_test.cpp
    cam = lmono_amd.Camera(w, h, 300.0, 300.0, 0.5 * w, 0.5 * h, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0)
    trk = lmono_amd.FeatureTracker(gpu_ctx, cam, 150, 15)
    kf = lmono_amd.KeyFrames(gpu_ctx, cam, _pattern(), 8, 16384)
    lines, recs = [], {}
    for f in range(k + delta + 1):
        rec = trk.track(0.1 * f, seq.frames[f])
        if f in (k, k + delta):
            uv = np.stack([rec["u"], rec["v"]], 1)
            idx, nkp = kf.add(seq.frames[f], uv)
            recs[idx] = rec
            lines.append("KF %d frame %d keypoints %d window %d" % (idx, f, nkp, len(uv)))
    m = kf.match(1, [0])
    rec = recs[1]
    for i in np.nonzero(m["status"][0])[0]:
        lines.append("MATCH %d cur %.9g %.9g old %.9g %.9g old_norm %.9g %.9g" % (rec["id"][i], rec["u"][i], rec["v"][i], m["old_uv"][0][i][0], m["old_uv"][0][i][1],
                                                                                 m["old_norm"][0][i][0], m["old_norm"][0][i][1]))
    count = int(m["counts"][0])
    lines.append("keyframe_test ok: %d of %d window points matched, gate %d" % (count, len(rec), 1 if count > K.MIN_BRIEF_LOOP_NUM else 0))
    assert res.stdout.splitlines() == lines
    assert count > 0
    trk.close(); kf.close()


def test_lead_store_tables_grow_and_are_reused(gpu_ctx):
    """add_batch led by one store with 1, then 3, then 5 stores (its job table grows 1 -> 4 -> 8 entries), then on that store matches
    against 3, 9, 17 and 3 old keyframes (the eight match arrays grow 4 -> 16 -> 32 entries and are reused): every result equals the
    restatement.  320 x 240 is the smallest image of this file."""
    import torch
    import lmono_amd
    w, h, n = 320, 240, 5
    pat = _pattern()
    gc, rc = _cam(w, h)
    imgs = [s5.Sequence(w, h, 1, seed=50 + s).frames[0] for s in range(n)]
    uvs = [_window_points(w, h, 40 + 10 * s, 60 + s) for s in range(n)]
    refs = [K.KeyFrameRef(rc, pat, imgs[s], uvs[s]) for s in range(n)]
    dev = [torch.from_numpy(np.ascontiguousarray(i)).to("cuda:0") for i in imgs]
    torch.cuda.synchronize()
    lead = lmono_amd.KeyFrames(gpu_ctx, gc, pat, 24, 4096)
    for rnd, n_stores in enumerate((1, 3, 5)):
        stores = [lead] + [lmono_amd.KeyFrames(gpu_ctx, gc, pat, 1, 4096) for _ in range(n_stores - 1)]
        idx, nkp = lmono_amd.KeyFrames.add_batch(stores, [t.data_ptr() for t in dev[:n_stores]], uvs[:n_stores])
        for s in range(n_stores):
            assert (idx[s], nkp[s]) == (rnd if s == 0 else 0, len(refs[s].keypoints))
            _check_keyframe(stores[s].get(idx[s]), refs[s], "%d stores, stream %d" % (n_stores, s))
        for k in stores[1:]:
            k.close()
    rng = np.random.default_rng(61)
    olds = [(refs[0].keypoints, refs[0].norm, refs[0].descriptors)] * 3 + [_random_old(rng, int(v)) for v in rng.integers(1, 600, 17)]
    for kp, nm, de in olds[3:]:
        lead.load(kp, nm, de)
    cur = np.stack([olds[3 + i % 17][2][i % len(olds[3 + i % 17][2])] for i in range(64)])
    cur[::2, 3] ^= np.uint32(0x00f0f00f)                     # every other one 12 bits away from its source
    ci = lead.load(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 8), np.uint32), rng.uniform(0, 300, (64, 2)).astype(np.float32), cur)
    assert ci == 20
    for n_old in (3, 9, 17, 3):
        which = list(range(20 - n_old, 20))
        got = lead.match(ci, which)
        _check_match(got, cur, [olds[o] for o in which])
        assert got["counts"].sum() > 0
    lead.close()
