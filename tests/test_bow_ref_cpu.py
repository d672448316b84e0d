"""The restatement tests/bow_ref.py of the loop detector's database pinned against things that are not the restatement: a
literal inverted-file statement of DBoW2's query, exact rational arithmetic, a brute-force descent; the vocabulary file layout, the
validator and the trainer of lmono_amd/brief_tools.py; and lmono_amd/host/bow_test, the kernel bodies of lmono_amd/csrc/bow.hip run as plain
C++.  No GPU."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from lmono_amd import capi
from tests import bow_cases as K
from tests import bow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOW_TEST = os.path.join(ROOT, "lmono_amd", "host", "bow_test")
QUERY_CURS = (0, 1, 19, 20, 30, 59, 60, 64, 65, 69)


# ---- a second statement of 6h: DBoW2's own data structures, literally (a map per keyframe, an inverted file, a map of pairs)
def _literal_vector(voc, desc):
    """TemplatedVocabulary::transform(features, v) + BowVector::addWeight / normalize with maps keyed by node and word."""
    kids, rows = {}, {}
    for r, (n, p) in enumerate(zip(voc["node_id"], voc["parent_id"])):
        kids.setdefault(int(p), []).append(int(n)); rows[int(n)] = r
    word = {int(n): int(w) for n, w in zip(voc["word_node_id"], voc["word_id"])}
    de = np.asarray(voc["descriptors"], np.uint32).reshape(-1, 8)
    v = {}
    for d in np.asarray(desc, np.uint32).reshape(-1, 8):
        node = 0
        while node in kids:
            dist = [sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(de[rows[c]], d)) for c in kids[node]]
            node = kids[node][dist.index(min(dist))]                    # list.index: the first minimum
        w, weight = word[node], float(voc["weight"][rows[node]])
        if weight > 0:
            v[w] = v[w] + weight if w in v else weight
    norm = 0.0
    for w in sorted(v):
        norm += abs(v[w])
    if norm > 0:
        for w in v:
            v[w] /= norm
    return v


def _literal_query(maps, cur, max_results, max_id):
    """TemplatedDatabase::queryL1 over an inverted file built from entries 0 .. cur - 1."""
    inverted = {}
    for e in range(cur):
        for w in sorted(maps[e]):
            inverted.setdefault(w, []).append((e, maps[e][w]))
    pairs = {}
    for w in sorted(maps[cur]):
        q = maps[cur][w]
        for e, d in inverted.get(w, []):
            if e < max_id or max_id == -1 or e == cur - 1:
                value = math.fabs(q - d) - math.fabs(q) - math.fabs(d)
                if e in pairs:
                    pairs[e] += value
                else:
                    pairs[e] = value
    ret = sorted((s, e) for e, s in pairs.items())[:max_results]
    return [e for _, e in ret], [-s / 2.0 for s, _ in ret]


@pytest.fixture(scope="module")
def literal_maps():
    # the scene's keyframes overlap: the literal descent runs once per pool item, the maps are assembled per keyframe in stored order
    voc, tree = K.v3(), R.Tree(K.v3())
    item_word = [next(iter(_literal_vector_words(voc, d))) for d in K.pool()[:790]]
    maps = []
    for p in K.POSITIONS:
        v = {}
        for i in range(10 * p, 10 * p + 200):
            w = item_word[i]
            weight = float(tree.weight[w])
            if weight > 0:
                v[w] = v[w] + weight if w in v else weight
        norm = 0.0
        for w in sorted(v):
            norm += abs(v[w])
        maps.append({w: (x / norm if norm > 0 else x) for w, x in v.items()})
    return maps


def _literal_vector_words(voc, d):
    """The word of one descriptor by the literal descent (weights ignored): a one-entry dict from a copy with unit weights."""
    unit = dict(voc); unit["weight"] = np.ones(len(voc["node_id"]))
    return _literal_vector(unit, d[None])


def test_vectors_equal_literal_statement(literal_maps):
    for t, (w, v) in enumerate(K.scene_vectors()):
        m = literal_maps[t]
        assert list(w) == sorted(m), t
        assert v.tobytes() == np.array([m[x] for x in sorted(m)], np.float64).tobytes(), t
    # and on the small irregular vocabulary, whole keyframes through the literal transform
    voc, tree = K.v2(), R.Tree(K.v2())
    for kf in K.host_cases()["v2"]["keyframes"]:
        w, v = R.bow_vector(tree, kf)
        m = _literal_vector(voc, kf)
        assert list(w) == sorted(m) and v.tobytes() == np.array([m[x] for x in sorted(m)], np.float64).tobytes()


def test_query_equals_inverted_file_statement(literal_maps):
    vectors = K.scene_vectors()
    for cur in QUERY_CURS:
        for max_results in (1, 4, 16):
            for max_id in (-1, -5, 0, cur, cur + 10, cur - K.LOOP_SEARCH_GAP):
                ids, sc = R.query(vectors, cur, max_results, max_id)
                lid, lsc = _literal_query(literal_maps, cur, max_results, max_id)
                assert list(ids) == lid, (cur, max_results, max_id)
                assert sc.tobytes() == np.array(lsc, np.float64).tobytes(), (cur, max_results, max_id)


def test_score_against_exact_l1_distance():
    """Score against 1 - 0.5 * |v - w|_1 in exact rational arithmetic (the stored doubles as fractions).  The bound is the one DESIGN.md 6h
    derives: s is a sequential fp64 sum over the `terms` common words and every partial sum lies in [-2, 0], where an ulp is at most
    2^-52, so the additions err by at most terms * 2^-52; the remaining 2 * 2^-52 covers what is not the additions (the two norms, 1 only
    to rounding, and the summands' own roundings); -s / 2 is exact.  Hence |Score - (1 - |v - w|_1 / 2)| <= (terms + 2) * 2^-52."""
    vectors = K.scene_vectors()
    worst = 0.0
    for cur in QUERY_CURS:
        ids, sc = R.query(vectors, cur, 16, -1)
        q = {int(w): Fraction(float(x)) for w, x in zip(*vectors[cur])}
        for e, score in zip(ids, sc):
            d = {int(w): Fraction(float(x)) for w, x in zip(*vectors[int(e)])}
            l1 = sum(abs(q.get(w, 0) - d.get(w, 0)) for w in set(q) | set(d))
            terms = len(set(q) & set(d))
            bound = (terms + 2) * 2.0 ** -52
            err = abs(Fraction(float(score)) - (1 - l1 / 2))
            worst = max(worst, float(err) / bound)
            assert err <= Fraction(bound), (cur, int(e), float(err), bound)
    print("largest error / bound: %.3f" % worst)


def test_descent_equals_brute_force_argmin():
    for voc in (K.v1(), K.v2(), K.v3()):
        tree = R.Tree(voc)
        de = np.asarray(voc["descriptors"], np.uint32)
        nid, par = voc["node_id"], voc["parent_id"]
        word_of = dict(zip(voc["word_node_id"].tolist(), voc["word_id"].tolist()))
        for d in K.transform_inputs(voc, 65):
            node = 0
            while (par == node).any():
                rows = np.nonzero(par == node)[0]                       # file order
                node = int(nid[rows[np.argmin(R.hamming(de[rows], d))]])
            assert tree.word(d) == word_of[node]


def test_tie_goes_to_the_first_child_in_file_order():
    voc = K.v2()
    tree = R.Tree(voc)
    same = voc["descriptors"][list(voc["node_id"]).index(5)]
    assert (same == voc["descriptors"][list(voc["node_id"]).index(4)]).all() and list(voc["node_id"]).index(5) < list(voc["node_id"]).index(4)
    w, wt = R.words(tree, same[None])
    assert w[0] == 4 and wt[0] == 1.5          # node 5 (word 4), not node 4 (word 2), which has the lower id
    w, _ = R.words(tree, K.flip(same, [200])[None])
    assert w[0] == 4


def test_scene_has_the_properties_the_gpu_tests_rely_on():
    vectors = K.scene_vectors()
    loops = [R.detect_loop(vectors, c, K.LOOP_SEARCH_GAP)[0] for c in range(70)]
    assert all(x == -1 for x in loops[:20])
    for c in range(60, 70):
        ids, sc = R.query(vectors, c, 4, c - K.LOOP_SEARCH_GAP)
        assert loops[c] >= 0 and sc[0] > 0.999 and ids[0] == c - 55         # the revisited keyframe: the same words, Score 1 to rounding
    items, lv = K.lonely_store()
    cur = len(items) - 1
    loop, ids, sc = R.detect_loop(lv, cur, K.LOOP_SEARCH_GAP)
    assert loop == -1 and list(ids) == [cur - 1] and sc[0] > R.ALPHA            # the neighbour alone: ret[0] passes, no ret[i >= 1]
    assert all(not set(lv[cur][0]) & set(lv[e][0]) for e in range(cur - 1))
    ids, sc = R.query(K.twin_store()[1], 3, 4, -1)
    assert list(ids[:2]) == [0, 1] and sc[0] == sc[1]                            # byte-identical keyframes: the lower id first
    assert len(R.query(vectors, 1, 16, -1)[0]) == 1 and len(R.query(vectors, 0, 4, -1)[0]) == 0


def test_vocabulary_file_round_trip(tmp_path):
    for name, voc in (("v1", K.v1()), ("v2", K.v2()), ("v3", K.v3())):
        path = tmp_path / (name + ".bin")
        capi.save_brief_vocabulary(path, voc)
        raw = open(path, "rb").read()
        assert len(raw) == 24 + 48 * len(voc["node_id"]) + 8 * len(voc["word_id"])
        assert raw == R.vocabulary_bytes(voc)
        back = capi.load_brief_vocabulary(path)
        for key in capi._VOC_KEYS:
            assert np.asarray(back[key]).tobytes() == np.asarray(voc[key]).tobytes() and np.asarray(back[key]).dtype == np.asarray(voc[key]).dtype, (name, key)
        again = tmp_path / (name + "_again.bin")
        capi.save_brief_vocabulary(again, back)
        assert open(again, "rb").read() == raw
    with pytest.raises(capi.LmonoError):
        open(tmp_path / "short.bin", "wb").write(raw[:-3])
        capi.load_brief_vocabulary(tmp_path / "short.bin")


def test_validator_accepts_the_good_and_names_every_fault():
    for voc in (K.v1(), K.v2(), K.v3()):
        assert capi.check_brief_vocabulary(voc) is None
    seen = set()
    for name, voc, reason in K.malformed():
        assert capi.check_brief_vocabulary(voc) == reason, name
        seen.add(reason)
    assert len(seen) == 11           # every refusal of 6h


def _training_sets(seed, n_sets=9, per=60):
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 1 << 32, (12, 8), dtype=np.uint64).astype(np.uint32)
    return [np.stack([K.flip(centres[rng.integers(12)], rng.choice(256, 10, replace=False)) for _ in range(per)]) for _ in range(n_sets)]


def test_trainer():
    sets = _training_sets(3)
    voc = capi.train_brief_vocabulary(sets, 4, 3, seed=7)
    assert capi.check_brief_vocabulary(voc) is None
    same = capi.train_brief_vocabulary(sets, 4, 3, seed=7)
    assert all(np.asarray(voc[k]).tobytes() == np.asarray(same[k]).tobytes() for k in capi._VOC_KEYS)
    other = capi.train_brief_vocabulary(sets, 4, 3, seed=8)
    assert any(np.asarray(voc[k]).tobytes() != np.asarray(other[k]).tobytes() for k in capi._VOC_KEYS)
    # idf: ln(N / N_i) over the sets, by the words the restatement's descent gives them
    tree = R.Tree(voc)
    n_i = np.zeros(len(voc["word_id"]), np.int64)
    for s in sets:
        n_i[np.unique(R.words(tree, s)[0])] += 1
    for w in range(len(n_i)):
        assert tree.weight[w] == (math.log(len(sets) / n_i[w]) if n_i[w] else 0.0), w
    assert (tree.weight > 0).any()
    # at most k descriptors: one leaf per distinct descriptor, under the root
    few = sets[0][[0, 1, 1, 2]]
    small = capi.train_brief_vocabulary([few[:2], few[2:]], 4, 3, seed=0)
    assert capi.check_brief_vocabulary(small) is None
    assert len(small["node_id"]) == 3 and (small["parent_id"] == 0).all() and len(small["word_id"]) == 3
    assert small["descriptors"].tobytes() == few[[0, 1, 3]].tobytes()


@pytest.mark.skipif(not os.path.exists(BOW_TEST), reason="lmono_amd/host/bow_test is not built (build() makes it)")
def test_bow_test_equals_restatement(tmp_path):
    stores = {"v3_scene": K.scene_vectors(), "v3_lonely": K.lonely_store()[1], "v3_twins": K.twin_store()[1]}
    jobs = [(name, R.case_bytes(case), R.result_bytes(case, stores.get(name))) for name, case in K.host_cases().items()]
    jobs += [("malformed_" + name, R.vocabulary_bytes(voc), R.refusal_bytes(reason)) for name, voc, reason in K.malformed()]
    for name, blob, want in jobs:
        src, dst = tmp_path / (name + ".bin"), tmp_path / (name + ".out")
        open(src, "wb").write(blob)
        res = subprocess.run([BOW_TEST, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert res.returncode == 0 and not res.stderr, (name, res.stderr[-1000:])
        assert open(dst, "rb").read() == want, name
