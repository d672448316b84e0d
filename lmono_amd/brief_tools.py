"""Offline BRIEF tooling in plain numpy (no library, no GPU): the pattern file reader, and the vocabulary of DESIGN.md 6h -- the file
layout of the reference's VocabularyBinary.hpp, the checks of lmono_brief_vocabulary_create, a trainer."""
import numpy as np

from .errors import LmonoError


def load_brief_pattern(path):
    """Read an OpenCV-YAML pattern file in the list layout of the reference's brief_pattern.yml (a line `x1:` followed by one
    `- <integer>` line per entry, likewise y1, x2, y2) -> int32 [4, 256] in the order x1, y1, x2, y2.  No YAML library."""
    keys = ("x1", "y1", "x2", "y2")
    got = {}
    cur = None
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            line = raw.split("#")[0].strip() if not raw.startswith("%") else ""
            if not line or line == "---":
                continue
            if line.endswith(":") and line[:-1].strip() in keys:
                cur = line[:-1].strip()
                if cur in got:
                    raise LmonoError("%s:%d: key %s appears twice" % (path, no, cur))
                got[cur] = []
            elif line.startswith("-") and cur is not None:
                try:
                    got[cur].append(int(line[1:].strip()))
                except ValueError:
                    raise LmonoError("%s:%d: not an integer entry: %r" % (path, no, raw.rstrip())) from None
            else:
                raise LmonoError("%s:%d: not a line of a BRIEF pattern list: %r" % (path, no, raw.rstrip()))
    for k in keys:
        if len(got.get(k, ())) != 256:
            raise LmonoError("%s: key %s has %d entries, a BRIEF pattern needs exactly 256" % (path, k, len(got.get(k, ()))))
    return np.array([got[k] for k in keys], np.int32)


_VOC_NODE = np.dtype([("node_id", "<i4"), ("parent_id", "<i4"), ("weight", "<f8"), ("descriptor", "<u4", (8,))])      # 48 B: 4 x uint64 little-endian = 8 x uint32
_VOC_WORD = np.dtype([("node_id", "<i4"), ("word_id", "<i4")])
_VOC_KEYS = ("k", "L", "scoring", "weighting", "node_id", "parent_id", "weight", "descriptors", "word_node_id", "word_id")
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _voc_arrays(voc):
    """The arrays of a vocabulary dict in the types the C ABI reads."""
    return (np.ascontiguousarray(voc["node_id"], np.int32).reshape(-1), np.ascontiguousarray(voc["parent_id"], np.int32).reshape(-1),
            np.ascontiguousarray(voc["weight"], np.float64).reshape(-1), np.ascontiguousarray(voc["descriptors"], np.uint32).reshape(-1, 8),
            np.ascontiguousarray(voc["word_node_id"], np.int32).reshape(-1), np.ascontiguousarray(voc["word_id"], np.int32).reshape(-1))


def check_brief_vocabulary(voc):
    """The checks lmono_brief_vocabulary_create makes on the host, in its order and words -> None for a well-formed vocabulary, else the
    reason.  voc: dict with k, L, scoring, weighting (ints), node_id, parent_id, weight [nNodes], descriptors [nNodes, 8] uint32,
    word_node_id, word_id [nWords]; node 0 is the root and has no record."""
    k, L = int(voc["k"]), int(voc["L"])
    nid, par, wt, de, wn, wi = _voc_arrays(voc)
    n, nw = len(nid), len(wn)
    if k < 2 or k > 64:
        return "brief vocabulary: k outside 2..64"
    if L < 1 or L > 10:
        return "brief vocabulary: L outside 1..10"
    if int(voc["scoring"]) != 0 or int(voc["weighting"]) != 0:
        return "brief vocabulary: only L1_NORM scoring (0) with TF_IDF weighting (0) is built"
    if n < 1 or n > 16777215:
        return "brief vocabulary: nNodes outside 1..16777215"
    if nw < 1 or nw > n:
        return "brief vocabulary: nWords outside 1..nNodes"
    if not (len(par) == len(wt) == len(de) == n) or len(wi) != nw:
        return "brief vocabulary: a null array"
    if not np.array_equal(np.sort(nid), np.arange(1, n + 1)):
        return "brief vocabulary: nodeIds are not exactly 1..nNodes, each once"
    if ((par < 0) | (par > n) | (par == nid)).any():
        return "brief vocabulary: a parentId outside 0..nNodes or equal to its own nodeId"
    if not (np.isfinite(wt) & (wt >= 0)).all():
        return "brief vocabulary: a weight that is negative or not finite"
    n_children = np.bincount(par, minlength=n + 1)
    if n_children.max() > k:
        return "brief vocabulary: an inner node with more than k children"
    depth = np.full(n + 1, -1, np.int64)
    depth[0] = 0
    level = np.array([0])
    for lv in range(1, L + 1):
        level = nid[np.isin(par, level)]
        depth[level] = lv
    if (depth < 0).any():
        return "brief vocabulary: a node unreachable from the root, or deeper than L"
    bad = "brief vocabulary: the words are not a bijection between 0..nWords-1 and the leaves"
    if int((n_children == 0).sum()) != nw or not np.array_equal(np.sort(wi), np.arange(nw)):
        return bad
    if ((wn < 1) | (wn > n)).any() or len(np.unique(wn)) != nw or (n_children[wn] != 0).any():
        return bad
    return None


def load_brief_vocabulary(path):
    """A vocabulary file in the layout of VocabularyBinary.hpp (6 int32 k, L, scoringType, weightingType, nNodes, nWords; nNodes records of
    48 B; nWords records of 8 B) -> dict of plain arrays (see check_brief_vocabulary).  The bytes are not judged here."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 24:
        raise LmonoError("%s: shorter than the header of a vocabulary file" % path)
    k, L, scoring, weighting, n, nw = (int(v) for v in np.frombuffer(raw, "<i4", 6))
    if n < 0 or nw < 0 or len(raw) != 24 + 48 * n + 8 * nw:
        raise LmonoError("%s: %d bytes, but the header (nNodes %d, nWords %d) asks for %d" % (path, len(raw), n, nw, 24 + 48 * n + 8 * nw))
    nodes = np.frombuffer(raw, _VOC_NODE, n, 24)
    words = np.frombuffer(raw, _VOC_WORD, nw, 24 + 48 * n)
    return {"k": k, "L": L, "scoring": scoring, "weighting": weighting, "node_id": nodes["node_id"].astype(np.int32), "parent_id": nodes["parent_id"].astype(np.int32),
            "weight": nodes["weight"].astype(np.float64), "descriptors": nodes["descriptor"].astype(np.uint32), "word_node_id": words["node_id"].astype(np.int32),
            "word_id": words["word_id"].astype(np.int32)}


def save_brief_vocabulary(path, voc):
    """The inverse of load_brief_vocabulary: 24 + 48 nNodes + 8 nWords bytes."""
    nid, par, wt, de, wn, wi = _voc_arrays(voc)
    nodes = np.zeros(len(nid), _VOC_NODE)
    nodes["node_id"] = nid; nodes["parent_id"] = par; nodes["weight"] = wt; nodes["descriptor"] = de
    words = np.zeros(len(wn), _VOC_WORD)
    words["node_id"] = wn; words["word_id"] = wi
    with open(path, "wb") as f:
        f.write(np.array([voc["k"], voc["L"], voc["scoring"], voc["weighting"], len(nid), len(wn)], "<i4").tobytes())
        f.write(nodes.tobytes())
        f.write(words.tobytes())


def _mix32(x):
    """The hash of DESIGN.md 6e (item 4a.2) on uint32."""
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _hamming_to(desc, centre):
    """[n, 8] uint32 x [8] uint32 -> int32 [n]."""
    return _POP8[(desc ^ centre[None, :]).view(np.uint8)].sum(1).astype(np.int32)


def _voc_words_of(voc, desc):
    """The word of every descriptor by the descent of 6h (the nearest child, ties to the first in file order) -> int32 [n]."""
    nid, par, wt, de, wn, wi = _voc_arrays(voc)
    kids = {}
    for r in range(len(nid)):
        kids.setdefault(int(par[r]), []).append(r)
    word_of = {int(a): int(b) for a, b in zip(wn, wi)}
    out = np.zeros(len(desc), np.int32)
    for i, d in enumerate(desc):
        node = 0
        while node in kids:
            rows = kids[node]
            node = int(nid[rows[int(np.argmin(_hamming_to(de[rows], d)))]])         # argmin: the first of equal distances
        out[i] = word_of[node]
    return out


def train_brief_vocabulary(descriptor_sets, k, L, seed=0):
    """A vocabulary from this project's own descriptors: hierarchical k-majority clustering of DESIGN.md 6h (a definition of this project,
    deterministic in seed; offline tooling, plain numpy).  descriptor_sets: a list of [n_i, 8] uint32 arrays (one per image) -> dict."""
    sets = [np.ascontiguousarray(s, np.uint32).reshape(-1, 8) for s in descriptor_sets]
    if not (2 <= int(k) <= 64) or not (1 <= int(L) <= 10):
        raise LmonoError("train_brief_vocabulary: k in 2..64 and L in 1..10")
    desc = np.concatenate(sets) if sets else np.zeros((0, 8), np.uint32)
    if len(desc) == 0:
        raise LmonoError("train_brief_vocabulary: no descriptors")
    nodes = []                       # (parent id, descriptor); node id = position + 1

    def new_node(parent, d):
        nodes.append((parent, np.array(d, np.uint32)))
        return len(nodes)

    def distinct(idx):
        seen, out = set(), []
        for i in idx:
            key = desc[i].tobytes()
            if key not in seen:
                seen.add(key); out.append(i)
        return out

    def split(node, idx, level):
        """The children of `node` (at `level`) over the descriptors idx."""
        if len(idx) <= k:
            for i in distinct(idx):
                new_node(node, desc[i])
            return
        d = desc[idx]
        first = _mix32(int(seed) ^ node) % len(idx)
        centres = [d[first].copy()]
        nearest = _hamming_to(d, centres[0])
        while len(centres) < k:
            far = int(np.argmax(nearest))                  # the farthest from its nearest centre, ties to the lowest index
            if nearest[far] == 0:
                break
            centres.append(d[far].copy())
            nearest = np.minimum(nearest, _hamming_to(d, centres[-1]))
        centres = np.stack(centres)
        bits = np.unpackbits(d.view(np.uint8), axis=1, bitorder="little")
        assign = None
        for _ in range(10):
            dist = np.stack([_hamming_to(d, c) for c in centres], 1)
            now = np.argmin(dist, 1)                       # ties to the lowest centre
            if assign is not None and np.array_equal(now, assign):
                break
            assign = now
            for c in range(len(centres)):
                members = bits[assign == c]
                if len(members):                           # an empty cluster keeps its centre
                    vote = (2 * members.sum(0) > len(members)).astype(np.uint8)      # a tie gives bit 0
                    centres[c] = np.packbits(vote, bitorder="little").view(np.uint32)
        groups = [(c, [idx[i] for i in np.nonzero(assign == c)[0]]) for c in range(len(centres))]
        groups = [(new_node(node, centres[c]), g) for c, g in groups if g]
        if level + 1 < L:
            for child, g in groups:
                if len(g) > 1:
                    split(child, g, level + 1)

    split(0, list(range(len(desc))), 0)
    parent = np.array([p for p, _ in nodes], np.int32)
    node_id = np.arange(1, len(nodes) + 1, dtype=np.int32)
    leaves = node_id[~np.isin(node_id, parent)]
    voc = {"k": int(k), "L": int(L), "scoring": 0, "weighting": 0, "node_id": node_id, "parent_id": parent, "weight": np.zeros(len(nodes)),
           "descriptors": np.stack([d for _, d in nodes]), "word_node_id": leaves.astype(np.int32), "word_id": np.arange(len(leaves), dtype=np.int32)}
    # setNodeWeights (TemplatedVocabulary.h:942-): idf over the descriptor sets, by the words the finished tree gives them
    n_i = np.zeros(len(leaves), np.int64)
    for s in sets:
        n_i[np.unique(_voc_words_of(voc, s))] += 1
    weight = np.zeros(len(nodes))
    for w, leaf in enumerate(leaves):
        weight[leaf - 1] = float(np.log(len(sets) / n_i[w])) if n_i[w] > 0 else 0.0
    voc["weight"] = weight
    return voc
