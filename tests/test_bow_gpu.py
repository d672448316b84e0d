"""Loop detection on the device (lmono_brief_vocabulary_*, lmono_keyframes_bow / _query / _detect_loop*) against the CPU
restatement tests/bow_ref.py: equal bytes.  Descriptors go into the stores through KeyFrames.load, without images."""
import os

import numpy as np
import pytest

from tests import bow_cases as K
from tests import bow_ref as R
from workloads import s5

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")
EINVAL, ECAPACITY = "lmono error -1", "lmono error -4"


def _store(ctx, max_kf, max_kp):
    import lmono_amd
    cam = lmono_amd.Camera(32, 32, 30.0, 30.0, 16.0, 16.0, 0.0, 0.0, 0.0, 0.0, 5, 0, 0)
    return lmono_amd.KeyFrames(ctx, cam, lmono_amd.load_brief_pattern(PATTERN_FILE), max_kf, max_kp)


def _load(kf, desc):
    desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
    z = np.zeros((len(desc), 2), np.float32)
    return kf.load(z, z, desc)


def _same(got, want, what):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, g, w)


@pytest.fixture(scope="module")
def voc3(gpu_ctx):
    import lmono_amd
    v = lmono_amd.BriefVocabulary(gpu_ctx, K.v3())
    yield v
    v.close()


@pytest.fixture(scope="module")
def scene_store(gpu_ctx, voc3):
    kf = _store(gpu_ctx, 96, 257)
    kf.set_vocabulary(voc3)
    for d in K.scene():
        _load(kf, d)
    yield kf
    kf.close()


@pytest.mark.parametrize("name", ["v1", "v2", "v3"])
def test_transform_equals_restatement(gpu_ctx, name):
    import lmono_amd
    voc = getattr(K, name)()
    tree = R.Tree(voc)
    dev = lmono_amd.BriefVocabulary(gpu_ctx, voc)
    for n in (1, 63, 64, 65, 300):
        d = K.transform_inputs(voc, n)
        _same(dev.transform(d), R.words(tree, d), (name, n))
    d = np.concatenate([[K.ZERO, K.ONES], np.asarray(voc["descriptors"], np.uint32)[:257]])          # distance 0 to a node of every level that fits
    _same(dev.transform(d), R.words(tree, d), (name, "nodes"))
    w, wt = dev.transform(np.zeros((0, 8), np.uint32))
    assert len(w) == 0 and len(wt) == 0
    dev.close()


@pytest.mark.parametrize("max_kp", [100, 257, 4096])
def test_bow_vector_equals_restatement(gpu_ctx, voc3, max_kp):
    tree, pw, pool = R.Tree(K.v3()), K.pool_words(), K.pool()
    rng = np.random.default_rng(max_kp)
    kf = _store(gpu_ctx, 8, max_kp)
    kf.set_vocabulary(voc3)
    picks = [rng.integers(0, 1000, n) for n in (0, 1, max_kp - 1, max_kp)]
    picks.append(np.arange(min(max_kp, 790)))                        # every word once or a few times
    for it in picks:
        _load(kf, pool[it])
    for i, it in enumerate(picks):
        _same(kf.bow(i), R.bow_vector(tree, pool[it], pw[it]), (max_kp, i))
    kf.close()


def test_bow_vector_stop_words_and_repeated_descriptor(gpu_ctx):
    import lmono_amd
    voc = K.v2()
    tree = R.Tree(voc)
    dev = lmono_amd.BriefVocabulary(gpu_ctx, voc)
    kf = _store(gpu_ctx, 8, 512)
    kf.set_vocabulary(dev)
    de = {int(n): d for n, d in zip(voc["node_id"], voc["descriptors"])}
    frames = [np.repeat(de[7][None], 5, 0),                                               # only the stop word
              np.repeat(de[8][None], 300, 0),                                             # one word 300 times: 1/3 added to itself 299 times
              np.concatenate([np.repeat(de[8][None], 300, 0), np.repeat(de[9][None], 7, 0), de[7][None], de[1][None]]),
              K.transform_inputs(voc, 65)]
    for d in frames:
        _load(kf, d)
    for i, d in enumerate(frames):
        _same(kf.bow(i), R.bow_vector(tree, d), i)
    assert len(kf.bow(0)[0]) == 0
    third = 1.0 / 3.0
    acc = third
    for _ in range(299):
        acc = acc + third
    assert acc != 300 * third                 # the sequential add is what the definition asks for, and it shows
    kf.close(); dev.close()


def test_query_equals_restatement_on_the_scene(scene_store):
    vectors = K.scene_vectors()
    for cur in (0, 1, 19, 20, 30, 59, 60, 69):
        for max_id in (-1, -5, 0, cur, cur + 10):
            for max_results in (1, 4, 16):
                _same(scene_store.query(cur, max_results, max_id), R.query(vectors, cur, max_results, max_id), (cur, max_id, max_results))
    for cur in (1, 64, 65):                    # 1, 64 and 65 entries admitted: one thread, one full workgroup of k_bow_score, one more
        got = scene_store.query(cur, 16, -1)
        _same(got, R.query(vectors, cur, 16, -1), cur)
    assert len(scene_store.query(1, 4, -1)[0]) == 1 and len(scene_store.query(0, 4, -1)[0]) == 0          # fewer results than max_results


def test_query_tie_goes_to_the_lower_id(gpu_ctx, voc3):
    items, vectors = K.twin_store()
    kf = _store(gpu_ctx, 4, 200)
    kf.set_vocabulary(voc3)
    for it in items:
        _load(kf, K.pool()[it])
    ids, sc = kf.query(3, 4, -1)
    _same((ids, sc), R.query(vectors, 3, 4, -1), "twins")
    assert list(ids[:2]) == [0, 1] and sc[0] == sc[1]
    kf.close()


def test_detect_loop_equals_restatement(gpu_ctx, voc3, scene_store):
    vectors = K.scene_vectors()
    found = 0
    for cur in range(70):
        loop, ids, sc = scene_store.detect_loop(cur, K.LOOP_SEARCH_GAP)
        want = R.detect_loop(vectors, cur, K.LOOP_SEARCH_GAP)
        assert loop == want[0], cur
        _same((ids, sc), want[1:], cur)
        found += loop >= 0
    assert found >= 10
    items, lv = K.lonely_store()
    kf = _store(gpu_ctx, 32, 200)
    kf.set_vocabulary(voc3)
    for it in items:
        _load(kf, K.pool()[it])
    cur = len(items) - 1
    loop, ids, sc = kf.detect_loop(cur, K.LOOP_SEARCH_GAP)
    assert loop == -1 and list(ids) == [cur - 1] and sc[0] > 0.05          # ret[0] passes, find_loop is false
    _same((ids, sc), R.detect_loop(lv, cur, K.LOOP_SEARCH_GAP)[1:], "lonely")
    kf.close()


def test_detect_loop_is_a_pure_function_of_the_store(gpu_ctx, voc3):
    scene, vectors = K.scene(), K.scene_vectors()
    kf = _store(gpu_ctx, 80, 200)
    kf.set_vocabulary(voc3)
    for d in scene[:60]:
        _load(kf, d)
    curs = (25, 45, 59)
    first = [kf.detect_loop(c, K.LOOP_SEARCH_GAP) for c in curs]
    for c, f in zip(curs, first):
        assert f[0] == R.detect_loop(vectors, c, K.LOOP_SEARCH_GAP)[0]
    for d in scene[60:]:
        _load(kf, d)
    for c, f in zip(curs, first):
        again = kf.detect_loop(c, K.LOOP_SEARCH_GAP)
        assert again[0] == f[0]
        _same(again[1:], f[1:], ("ten more", c))
    kf.clear()
    for d in scene[:60]:
        _load(kf, d)
    for c, f in zip(curs, first):
        again = kf.detect_loop(c, K.LOOP_SEARCH_GAP)
        assert again[0] == f[0]
        _same(again[1:], f[1:], ("reloaded", c))
    kf.set_vocabulary(voc3)                    # re-attached: the watermark goes back to 0 and every vector is built again
    for c, f in zip(curs, first):
        again = kf.detect_loop(c, K.LOOP_SEARCH_GAP)
        assert again[0] == f[0]
        _same(again[1:], f[1:], ("re-attached", c))
    kf.close()


def test_detect_loop_batch_equals_single_calls(gpu_ctx, voc3):
    import lmono_amd
    scene = K.scene()
    sizes = (70, 31, 7)
    stores = [_store(gpu_ctx, 70, 200) for _ in sizes]
    singles = [_store(gpu_ctx, 70, 200) for _ in sizes]
    for group in (stores, singles):
        for kf, n in zip(group, sizes):
            kf.set_vocabulary(voc3)
            for d in scene[:n]:
                _load(kf, d)
    curs = [n - 1 for n in sizes]
    got = lmono_amd.KeyFrames.detect_loop_batch(stores, curs, K.LOOP_SEARCH_GAP)
    for kf, c, g in zip(singles, curs, got):
        want = kf.detect_loop(c, K.LOOP_SEARCH_GAP)
        assert g[0] == want[0]
        _same(g[1:], want[1:], c)
    assert got[0][0] >= 0
    # refused with every store unchanged: a repeated store, a store without a vocabulary
    with pytest.raises(lmono_amd.LmonoError, match="distinct"):
        lmono_amd.KeyFrames.detect_loop_batch([stores[0], stores[1], stores[0]], [5, 5, 5], K.LOOP_SEARCH_GAP)
    bare = _store(gpu_ctx, 8, 200)
    _load(bare, scene[0])
    with pytest.raises(lmono_amd.LmonoError, match="no vocabulary"):
        lmono_amd.KeyFrames.detect_loop_batch([stores[0], bare], [5, 0], K.LOOP_SEARCH_GAP)
    assert [len(s) for s in stores] == list(sizes) and len(bare) == 1
    again = lmono_amd.KeyFrames.detect_loop_batch(stores, curs, K.LOOP_SEARCH_GAP)
    for g, a in zip(got, again):
        assert g[0] == a[0]
        _same(a[1:], g[1:], "after the refusals")
    for kf in stores + singles + [bare]:
        kf.close()


def test_refusals(gpu_ctx, voc3):
    import lmono_amd
    kf = _store(gpu_ctx, 4, 200)
    _load(kf, K.scene()[0])
    for call in (lambda: kf.query(0), lambda: kf.bow(0), lambda: kf.detect_loop(0)):
        with pytest.raises(lmono_amd.LmonoError, match=EINVAL + ".*no vocabulary"):
            call()
    kf.set_vocabulary(voc3)
    for cur in (-1, 1, 4):
        with pytest.raises(lmono_amd.LmonoError, match=EINVAL + ".*not a stored keyframe"):
            kf.query(cur)
        with pytest.raises(lmono_amd.LmonoError, match=EINVAL):
            kf.detect_loop(cur)
    for max_results in (0, 17):
        with pytest.raises(lmono_amd.LmonoError, match=EINVAL + ".*max_results outside 1..16"):
            kf.query(0, max_results)
    kf.set_vocabulary(None)
    with pytest.raises(lmono_amd.LmonoError, match=EINVAL + ".*no vocabulary"):
        kf.query(0)
    kf.close()
    big = _store(gpu_ctx, 1, 16385)
    with pytest.raises(lmono_amd.LmonoError, match=ECAPACITY):
        big.set_vocabulary(voc3)
    big.close()
    ok = _store(gpu_ctx, 1, 16384)
    ok.set_vocabulary(voc3)
    ok.close()
    for name, voc, reason in K.malformed():          # refused on the host: nothing of it reaches a kernel
        with pytest.raises(lmono_amd.LmonoError) as err:
            lmono_amd.BriefVocabulary(gpu_ctx, voc)
        assert reason in str(err.value), name


def test_store_keeps_the_vocabulary_alive(gpu_ctx):
    import lmono_amd
    vectors = K.scene_vectors()
    dev = lmono_amd.BriefVocabulary(gpu_ctx, K.v3())
    a, b = _store(gpu_ctx, 32, 200), _store(gpu_ctx, 32, 200)             # one vocabulary serves both
    for kf in (a, b):
        kf.set_vocabulary(dev)
        for d in K.scene()[:25]:
            _load(kf, d)
    _same(a.query(24, 4, -1), R.query(vectors, 24, 4, -1), "before")
    dev.close()                                # the handle goes first
    _same(b.query(24, 4, -1), R.query(vectors, 24, 4, -1), "b, vectors built after the handle went")
    _load(a, K.scene()[25])
    _same(a.query(25, 4, -1), R.query(vectors, 25, 4, -1), "a, one more keyframe")
    a.close(); b.close()


def test_host_mirror_detect_equals_python_path(gpu_ctx, tmp_path):
    """lmono_amd/host/keyframe_test ... detect: every frame of a short s5 sequence -> KeyFrame -> LoopDetector::addKeyFrame with a trained
    k = 4, L = 2 vocabulary; its printed loop indices and results equal the Python path's on the same frames."""
    import subprocess
    import lmono_amd
    exe = os.path.join(ROOT, "lmono_amd", "host", "keyframe_test")
    assert os.path.exists(exe), "build() makes lmono_amd/host/keyframe_test"
    w, h, n, gap = 320, 240, 10, 3
    seq = s5.Sequence(w, h, n, seed=1, step=(1.5, 0.5), rot_step=0.002, zoom_step=0.001)
    raw = tmp_path / "frames.raw"
    with open(raw, "wb") as f:
        f.write(("%d %d %d\n" % (w, h, len(seq.frames))).encode())
        for img in seq.frames:
            f.write(np.ascontiguousarray(img).tobytes())
    # the Python path with the camera and limits of keyframe_test.cpp; the vocabulary is trained on its descriptors
    cam = lmono_amd.Camera(w, h, 300.0, 300.0, 0.5 * w, 0.5 * h, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0)
    trk = lmono_amd.FeatureTracker(gpu_ctx, cam, 150, 15)
    kf = lmono_amd.KeyFrames(gpu_ctx, cam, lmono_amd.load_brief_pattern(PATTERN_FILE), n, 16384)
    nkps = []
    for f in range(n):
        rec = trk.track(0.1 * f, seq.frames[f])
        nkps.append(kf.add(seq.frames[f], np.stack([rec["u"], rec["v"]], 1))[1])
    voc = lmono_amd.train_brief_vocabulary([kf.get(f)["descriptors"][::7] for f in range(n)], 4, 2, seed=5)
    assert lmono_amd.check_brief_vocabulary(voc) is None
    voc_file = tmp_path / "voc.bin"
    lmono_amd.save_brief_vocabulary(voc_file, voc)
    dev = lmono_amd.BriefVocabulary(gpu_ctx, voc)
    kf.set_vocabulary(dev)
    lines, loops = [], 0
    for f in range(n):
        loop, ids, sc = kf.detect_loop(f, gap)
        lines.append("DETECT %d keypoints %d loop %d results %d" % (f, nkps[f], loop, len(ids)) + "".join(" %d:%.17g" % (i, s) for i, s in zip(ids, sc)))
        loops += loop >= 0
    res = subprocess.run([exe, str(raw), PATTERN_FILE, "detect", str(voc_file), str(gap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.splitlines() == lines
    assert loops > 0
    trk.close(); kf.close(); dev.close()
