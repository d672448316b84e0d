"""tests/bow_cases.py -- inputs of the BoW tests: three vocabularies built by hand, the revisit scene, the two special
stores, and the malformed vocabularies the host must refuse.  Inputs only: every expected value comes from tests/bow_ref.py."""
import copy
import functools

import numpy as np

from tests import bow_ref as R

ZERO = np.zeros(8, np.uint32)
ONES = np.full(8, 0xFFFFFFFF, np.uint32)
LOOP_SEARCH_GAP = 20
POSITIONS = list(range(60)) + list(range(5, 15))          # 70 keyframes: 0..59, then 5..14 again


def _voc(k, L, node_id, parent_id, weight, desc, word_node_id, word_id):
    return {"k": k, "L": L, "scoring": 0, "weighting": 0, "node_id": np.array(node_id, np.int32), "parent_id": np.array(parent_id, np.int32),
            "weight": np.array(weight, np.float64), "descriptors": np.array(desc, np.uint32).reshape(-1, 8), "word_node_id": np.array(word_node_id, np.int32),
            "word_id": np.array(word_id, np.int32)}


def flip(d, bits):
    d = np.array(d, np.uint32)
    for b in bits:
        d[int(b) >> 5] ^= np.uint32(1 << (int(b) & 31))
    return d


def v1():
    """k = 2, L = 1: two words."""
    return _voc(2, 1, [1, 2], [0, 0], [0.5, 1.25], [ZERO, ONES], [1, 2], [0, 1])


def v2():
    """k = 3, L = 3, irregular, records not in id order: node 1 a leaf at level 1; node 3 an inner node with the one child 7 (weight 0: a
    stop word); nodes 5 and 4 siblings with one descriptor, 5 first in the file, so the tie rule picks 5; node 6 inner with leaves 8, 9."""
    a = flip(ZERO, range(0, 40))                # node 2's side
    b = flip(ZERO, range(128, 256))             # node 3's side
    same = flip(a, range(40, 50))
    rec = [  # (node, parent, weight, descriptor)
        (3, 0, 0.0, b), (1, 0, 0.75, ZERO), (2, 0, 0.0, a),
        (7, 3, 0.0, b),
        (5, 2, 1.5, same), (4, 2, 2.5, same), (6, 2, 0.0, flip(a, range(60, 100))),
        (9, 6, 0.3, flip(a, range(60, 128))), (8, 6, 1.0 / 3.0, flip(a, range(60, 100))),
    ]
    return _voc(3, 3, [r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec], [r[3] for r in rec], [9, 1, 4, 7, 5, 8], [0, 1, 2, 3, 4, 5])


@functools.lru_cache(maxsize=None)
def _v3_tree():
    rng = np.random.default_rng(20240611)
    node_id, parent, desc = [], [], []
    level = []
    for _ in range(10):
        node_id.append(len(node_id) + 1); parent.append(0); desc.append(rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32))
        level.append(node_id[-1])
    for nflip in (48, 20):
        nxt = []
        for p in level:
            for _ in range(10):
                node_id.append(len(node_id) + 1); parent.append(p); desc.append(flip(desc[p - 1], rng.choice(256, nflip, replace=False)))
                nxt.append(node_id[-1])
        level = nxt
    pool = np.stack([flip(desc[int(rng.choice(level)) - 1], rng.choice(256, 6, replace=False)) for _ in range(1000)])
    return node_id, parent, np.stack(desc), level, pool


def pool():
    """1000 descriptors: each a random V3 leaf descriptor with 6 bits flipped."""
    return _v3_tree()[4]


def keyframe(position):
    return pool()[10 * position:10 * position + 200]


@functools.lru_cache(maxsize=None)
def v3():
    """k = 10, L = 3, full (1110 nodes); idf weights ln(N / N_i) over the N = 70 keyframes of the scene, 0 for a word no keyframe has."""
    node_id, parent, desc, leaves, pl = _v3_tree()
    voc = _voc(10, 3, node_id, parent, np.zeros(len(node_id)), desc, leaves, list(range(len(leaves))))
    pool_word = R.words(R.Tree(voc), pl)[0]
    n_i = np.zeros(len(leaves), np.int64)
    for p in POSITIONS:
        n_i[np.unique(pool_word[10 * p:10 * p + 200])] += 1
    w = np.zeros(len(node_id))
    for word, leaf in enumerate(leaves):
        if n_i[word] > 0:
            w[leaf - 1] = float(np.log(len(POSITIONS) / n_i[word]))
    voc["weight"] = w
    return voc


@functools.lru_cache(maxsize=None)
def pool_words():
    return R.words(R.Tree(v3()), pool())[0]


def scene():
    """The 70 keyframes' descriptors ([200, 8] each)."""
    return [keyframe(p) for p in POSITIONS]


@functools.lru_cache(maxsize=None)
def scene_vectors():
    tree = R.Tree(v3())
    pw = pool_words()
    return [R.bow_vector(tree, keyframe(p), pw[10 * p:10 * p + 200]) for p in POSITIONS]


def _vectors_of(items_per_kf):
    tree = R.Tree(v3())
    pw = pool_words()
    return [R.bow_vector(tree, pool()[it], pw[it]) for it in items_per_kf]


@functools.lru_cache(maxsize=None)
def lonely_store():
    """30 keyframes, gap 20: 0..27 at positions 0..27 (pool items below 470); 28 and 29 hold those pool items of [600, 790) whose word no
    item below 470 has.  query(29, 4, 9) then finds the neighbour alone -> (items per keyframe, vectors)."""
    pw = pool_words()
    low = set(int(w) for w in pw[:470])
    own = np.array([i for i in range(600, 790) if int(pw[i]) not in low])
    items = [np.arange(10 * p, 10 * p + 200) for p in range(28)] + [own, own[1:]]
    return items, _vectors_of(items)


@functools.lru_cache(maxsize=None)
def twin_store():
    """Keyframes 0 and 1 byte-identical, 2 overlapping, 3 identical again: query(3) ties 0 and 1 -> (items per keyframe, vectors)."""
    items = [np.arange(0, 200), np.arange(0, 200), np.arange(100, 300), np.arange(0, 200)]
    return items, _vectors_of(items)


def transform_inputs(voc, n, seed=0):
    """n descriptors: random ones, then (as far as n allows) every node descriptor (distance 0), all zeros and all ones."""
    rng = np.random.default_rng(seed + n)
    d = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    special = np.concatenate([[ZERO, ONES], np.asarray(voc["descriptors"], np.uint32).reshape(-1, 8)])
    m = min((n + 1) // 2, len(special))
    pick = np.unique(np.concatenate([[0, 1], np.linspace(0, len(special) - 1, m).astype(int)]))[:m]       # the second half: special ones, from every level
    d[n - m:] = special[pick]
    return d


def malformed():
    """(name, vocabulary, the reason the host gives) -- every refusal of DESIGN.md 6h, one fault each."""
    out = []

    def add(name, reason, **changes):
        v = copy.deepcopy(v2())
        for key, val in changes.items():
            v[key] = np.array(val, v[key].dtype) if isinstance(v[key], np.ndarray) else val
        out.append((name, v, "brief vocabulary: " + reason))

    base = v2()
    nid, par, wt = base["node_id"].tolist(), base["parent_id"].tolist(), base["weight"].tolist()

    def put(lst, at, val):
        c = list(lst); c[at] = val
        return c

    add("k_low", "k outside 2..64", k=1)
    add("k_high", "k outside 2..64", k=65)
    add("L_low", "L outside 1..10", L=0)
    add("L_high", "L outside 1..10", L=11)
    add("scoring", "only L1_NORM scoring (0) with TF_IDF weighting (0) is built", scoring=1)
    add("weighting", "only L1_NORM scoring (0) with TF_IDF weighting (0) is built", weighting=2)
    out.append(("no_nodes", _voc(3, 3, [], [], [], np.zeros((0, 8)), [], []), "brief vocabulary: nNodes outside 1..16777215"))
    add("more_words_than_nodes", "nWords outside 1..nNodes", word_node_id=list(range(1, 11)), word_id=list(range(10)))
    add("node_id_twice", "nodeIds are not exactly 1..nNodes, each once", node_id=put(nid, 4, 4))
    add("node_id_zero", "nodeIds are not exactly 1..nNodes, each once", node_id=put(nid, 1, 0))
    add("node_id_high", "nodeIds are not exactly 1..nNodes, each once", node_id=put(nid, 1, 10))
    add("parent_high", "a parentId outside 0..nNodes or equal to its own nodeId", parent_id=put(par, 3, 10))
    add("parent_negative", "a parentId outside 0..nNodes or equal to its own nodeId", parent_id=put(par, 3, -1))
    add("parent_self", "a parentId outside 0..nNodes or equal to its own nodeId", parent_id=put(par, 3, 7))
    add("weight_negative", "a weight that is negative or not finite", weight=put(wt, 1, -0.5))
    add("weight_nan", "a weight that is negative or not finite", weight=put(wt, 1, float("nan")))
    add("weight_inf", "a weight that is negative or not finite", weight=put(wt, 1, float("inf")))
    add("too_many_children", "an inner node with more than k children", k=2)
    add("cycle", "a node unreachable from the root, or deeper than L", parent_id=put(put(par, 7, 8), 8, 9))        # 9 -> 8 -> 9
    add("too_deep", "a node unreachable from the root, or deeper than L", L=2)
    add("word_missing", "the words are not a bijection between 0..nWords-1 and the leaves", word_node_id=[9, 1, 4, 7, 5], word_id=[0, 1, 2, 3, 4])
    add("word_id_twice", "the words are not a bijection between 0..nWords-1 and the leaves", word_id=[0, 1, 2, 3, 4, 4])
    add("word_id_high", "the words are not a bijection between 0..nWords-1 and the leaves", word_id=[0, 1, 2, 3, 4, 6])
    add("word_on_inner_node", "the words are not a bijection between 0..nWords-1 and the leaves", word_node_id=[9, 1, 4, 7, 5, 6])
    add("leaf_twice", "the words are not a bijection between 0..nWords-1 and the leaves", word_node_id=[9, 1, 4, 7, 5, 5])
    return out


def host_cases():
    """name -> case of lmono_amd/host/bow_test (tests/bow_ref.case_bytes): the three vocabularies with small stores, and the scene."""
    cases = {}
    for name, voc in (("v1", v1()), ("v2", v2())):
        t = transform_inputs(voc, 65)
        kfs = [t[:0], t[:1], t[:64], t, np.repeat(t[3:4], 40, 0), np.repeat(flip(ZERO, range(128, 256))[None], 5, 0), t[10:40]]
        cases[name] = {"voc": voc, "transform": t, "max_kp": 65, "keyframes": kfs, "queries": [(c, m, i) for c in range(7) for m in (1, 16) for i in (-1, 2)],
                       "detections": [(c, 2) for c in range(7)]}
    cases["v3_scene"] = {"voc": v3(), "transform": transform_inputs(v3(), 300), "max_kp": 257, "keyframes": scene(),
                         "queries": [(c, m, i) for c in (0, 1, 19, 20, 30, 59, 60, 64, 65, 69) for m in (1, 4, 16) for i in (-1, -5, 0, c, c + 10)],
                         "detections": [(c, LOOP_SEARCH_GAP) for c in range(70)]}
    for name, store in (("v3_lonely", lonely_store()), ("v3_twins", twin_store())):
        items = store[0]
        cases[name] = {"voc": v3(), "transform": np.zeros((0, 8), np.uint32), "max_kp": 200, "keyframes": [pool()[it] for it in items],
                       "queries": [(len(items) - 1, 4, -1), (len(items) - 1, 16, 0)], "detections": [(c, LOOP_SEARCH_GAP) for c in range(len(items))]}
    return cases
