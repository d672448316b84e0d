"""tests/bow_ref.py -- CPU restatement of the loop detector's database, numpy and plain Python floats only.  Test
infrastructure: the kernels of lmono_amd/csrc/bow.hip and this file implement one written definition, and every fp64 sum below is a
sequential Python-float loop in the order 6h states, so "equal" means equal bytes.  Restates, for TF_IDF weighting and L1_NORM scoring,
DBoW2's TemplatedVocabulary::transform (TemplatedVocabulary.h:1217-1258, :1065-1121), BowVector (BowVector.cpp:34-84),
TemplatedDatabase::queryL1 (TemplatedDatabase.h:656-723) and LoopDetector::detectLoop (LoopDetector.cc:181-259, without DEBUG_IMAGE).
It works on the file's own records (node ids, parent ids, file order): nothing here is re-indexed the way the library does it."""
import struct

import numpy as np

ALPHA = 0.05       # LoopDetector.cc: ret[0].Score > 0.05
BETA = 0.015       # ... ret[i].Score > 0.015

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(desc, one):
    """[n, 8] uint32 x [8] uint32 -> int32 [n]."""
    return _POP8[(np.ascontiguousarray(desc, np.uint32) ^ np.asarray(one, np.uint32)[None, :]).view(np.uint8)].sum(1).astype(np.int32)


class Tree:
    """The vocabulary as loadBin builds it: children of every node id in file order, the word id and weight of every leaf."""

    def __init__(self, voc):
        self.k, self.L = int(voc["k"]), int(voc["L"])
        self.node_id = np.asarray(voc["node_id"], np.int32)
        self.desc = np.ascontiguousarray(voc["descriptors"], np.uint32).reshape(-1, 8)
        self.children = {}
        for row, parent in enumerate(np.asarray(voc["parent_id"], np.int32)):
            self.children.setdefault(int(parent), []).append(row)
        weight_of_node = {int(n): float(w) for n, w in zip(self.node_id, np.asarray(voc["weight"], np.float64))}
        self.word_of_node = {int(n): int(w) for n, w in zip(voc["word_node_id"], voc["word_id"])}
        self.weight = np.zeros(len(self.word_of_node))
        for n, w in self.word_of_node.items():
            self.weight[w] = weight_of_node[n]

    def word(self, d):
        node = 0
        while node in self.children:
            rows = self.children[node]
            dist = hamming(self.desc[rows], d)
            best, at = int(dist[0]), 0
            for c in range(1, len(rows)):
                if int(dist[c]) < best:              # strict <: the first of equal children stays
                    best, at = int(dist[c]), c
            node = int(self.node_id[rows[at]])
        return self.word_of_node[node]


def words(tree, desc):
    """-> (word int32 [n], weight float64 [n])."""
    desc = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
    w = np.array([tree.word(d) for d in desc], np.int32).reshape(-1)
    return w, tree.weight[w] if len(w) else np.zeros(0)


def bow_vector(tree, desc, word_ids=None):
    """-> (word int32 [m] ascending, value float64 [m]).  word_ids: the descriptors' words when the caller has them already."""
    w = words(tree, desc)[0] if word_ids is None else np.asarray(word_ids, np.int32)
    entries = {}
    for x in w:                                      # stored order
        x = int(x)
        wt = float(tree.weight[x])
        if not wt > 0:
            continue
        entries[x] = entries[x] + wt if x in entries else wt
    keys = sorted(entries)
    norm = 0.0
    for x in keys:
        norm = norm + entries[x]
    vals = [entries[x] / norm for x in keys] if norm > 0 else [entries[x] for x in keys]
    return np.array(keys, np.int32).reshape(-1), np.array(vals, np.float64).reshape(-1)


def query(vectors, cur, max_results=4, max_id=-1):
    """vectors: list of (word, value) per stored keyframe -> (id int32 [n], Score float64 [n])."""
    qw, qv = vectors[cur]
    q = {int(w): float(v) for w, v in zip(qw, qv)}
    found = []
    for e in range(cur):                             # m_nentries = cur: the reference queries before it adds
        if not (e < max_id or max_id == -1 or e == cur - 1):
            continue
        s, common = 0.0, False
        for w, d in zip(vectors[e][0], vectors[e][1]):          # ascending word id
            w, d = int(w), float(d)
            if w in q:
                t = (abs(q[w] - d) - abs(q[w])) - abs(d)
                s = s + t if common else t
                common = True
        if common:
            found.append((s, e))
    found.sort()                                     # s ascending, ties to the lower entry id
    found = found[:max_results]
    return np.array([e for _, e in found], np.int32).reshape(-1), np.array([-s / 2.0 for s, _ in found], np.float64).reshape(-1)


def detect_rule(cur, gap, ids, scores):
    if cur - gap < 0:
        return -1
    find_loop = len(ids) >= 1 and scores[0] > ALPHA and any(scores[i] > BETA for i in range(1, len(ids)))
    if not (find_loop and cur > 5):
        return -1
    low = -1
    for i in range(len(ids)):
        if low == -1 or (ids[i] < low and scores[i] > BETA):
            low = int(ids[i])
    return low


def detect_loop(vectors, cur, gap):
    ids, scores = query(vectors, cur, 4, cur - gap)
    return detect_rule(cur, gap, ids, scores), ids, scores


# ---- the files of lmono_amd/host/bow_test (its header comment states both layouts)
def vocabulary_bytes(voc):
    n, nw = len(voc["node_id"]), len(voc["word_id"])
    out = [struct.pack("<6i", int(voc["k"]), int(voc["L"]), int(voc["scoring"]), int(voc["weighting"]), n, nw)]
    de = np.ascontiguousarray(voc["descriptors"], np.uint32).reshape(-1, 8)
    for r in range(n):
        out.append(struct.pack("<iid", int(voc["node_id"][r]), int(voc["parent_id"][r]), float(voc["weight"][r])) + de[r].astype("<u4").tobytes())
    for r in range(nw):
        out.append(struct.pack("<ii", int(voc["word_node_id"][r]), int(voc["word_id"][r])))
    return b"".join(out)


def case_bytes(case):
    """case: dict voc, transform [n, 8], max_kp, keyframes (list of [n, 8]), queries [(cur, max_results, max_id)], detections [(cur, gap)]."""
    t = np.ascontiguousarray(case["transform"], np.uint32).reshape(-1, 8)
    out = [vocabulary_bytes(case["voc"]), struct.pack("<i", len(t)), t.astype("<u4").tobytes(), struct.pack("<ii", len(case["keyframes"]), int(case["max_kp"]))]
    for d in case["keyframes"]:
        d = np.ascontiguousarray(d, np.uint32).reshape(-1, 8)
        out += [struct.pack("<i", len(d)), d.astype("<u4").tobytes()]
    out.append(struct.pack("<i", len(case["queries"])))
    out += [struct.pack("<3i", *q) for q in case["queries"]]
    out.append(struct.pack("<i", len(case["detections"])))
    out += [struct.pack("<2i", *d) for d in case["detections"]]
    return b"".join(out)


def refusal_bytes(message):
    m = message.encode()
    return struct.pack("<ii", 1, len(m)) + m


def result_bytes(case, vectors=None):
    """What bow_test writes for a well-formed case.  vectors: the keyframes' BoW vectors when the caller has them already."""
    tree = Tree(case["voc"])
    w, wt = words(tree, case["transform"])
    out = [struct.pack("<i", 0), w.astype("<i4").tobytes(), np.asarray(wt, "<f8").tobytes()]
    if vectors is None:
        vectors = [bow_vector(tree, d) for d in case["keyframes"]]
    for vw, vv in vectors:
        out += [struct.pack("<i", len(vw)), vw.astype("<i4").tobytes(), vv.astype("<f8").tobytes()]
    for cur, max_results, max_id in case["queries"]:
        ids, sc = query(vectors, cur, max_results, max_id)
        out += [struct.pack("<i", len(ids)), ids.astype("<i4").tobytes(), sc.astype("<f8").tobytes()]
    for cur, gap in case["detections"]:
        loop, ids, sc = detect_loop(vectors, cur, gap)
        out += [struct.pack("<ii", loop, len(ids)), ids.astype("<i4").tobytes(), sc.astype("<f8").tobytes()]
    return b"".join(out)
