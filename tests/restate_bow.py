"""Restatement of the reference's ORB bag-of-words loop detector in numpy / pure Python: the
DBoW3 calls of loopClosureHandler::detectLoop (src/loop_closure_handler.cpp:127-188) for the
combination it runs (TF_IDF weights, L1_NORM scoring, no direct index), after the published
library (rmsalinas/DBoW3: Vocabulary.cpp, Database.cpp, BowVector.cpp, ScoringObject.cpp,
DescManip.cpp).  DBoW3 is on no machine of this project: this text is unpinned against the
library itself; the GPU (lislam_bow_*) is pinned against this text, by equality.

Two forms:
  * literal and stateful: ``Database`` (an ordered dict per BoW vector, a real inverted file) and
    ``detect_loop`` (query, then add, once per keyframe);
  * the closed form the kernels use: ``closed_form_detect`` queries entry k against the entries
    below ``query_limit(k, gap)`` by merging sorted lists.

Every sum is a sequence of Python float (IEEE double) operations in the order the library runs
them; Python does not contract a * b + c.  Equal scores: DBoW3 leaves their order to std::sort;
both forms here put the lower entry id first.
"""
from __future__ import annotations

import math

import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)

DEFAULTS = dict(min_loop_bow_threshold=0.0155, index_score_threshold=0.015, min_loop_search_gap=50, max_results=4,
                min_frame_index=5, loop_index_bound=6)


def hamming(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """DescManip::distance for ORB: popcount of the XOR over 256 bits (last axis = 32 bytes)."""
    return POPCOUNT[np.bitwise_xor(a, b)].sum(axis=-1)


class Vocabulary:
    """parent[n], descriptor[n][32], weight[n]; node 0 is the root.  A node's children in ascending
    node id; a leaf's word id = its rank among leaves in ascending node id (createWords)."""

    def __init__(self, parent, descriptor, weight):
        self.parent = np.asarray(parent, np.int32)
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64)
        n = self.parent.shape[0]
        self.children = [[] for _ in range(n)]
        for i in range(1, n):
            self.children[int(self.parent[i])].append(i)
        self.word_of = np.full(n, -1, np.int32)
        leaves = [i for i in range(n) if not self.children[i]]
        self.word_of[leaves] = np.arange(len(leaves), dtype=np.int32)
        self.word_weight = self.weight[leaves]
        self.leaf_node = np.array(leaves, np.int32)
        kmax = max(len(c) for c in self.children)
        self.child_table = np.full((n, kmax), -1, np.int32)
        for i, c in enumerate(self.children):
            self.child_table[i, :len(c)] = c

    def transform_one(self, feature):
        """Vocabulary::transform(feature, id, weight), literally."""
        feature = np.asarray(feature, np.uint8).reshape(32)
        node = 0
        while self.children[node]:
            best, best_d = -1, None
            for c in self.children[node]:
                d = int(hamming(feature, self.descriptor[c]))
                if best_d is None or d < best_d:  # strict <: the first child wins a tie
                    best, best_d = c, d
            node = best
        return int(self.word_of[node]), float(self.weight[node])

    def transform(self, features):
        """The same for many descriptors, level by level -> (word (n,) int32, weight (n,) float64)."""
        f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        node = np.zeros(f.shape[0], np.int64)
        while True:
            kids = self.child_table[node]                      # (n, kmax)
            inner = kids[:, 0] >= 0
            if not inner.any():
                break
            idx = np.nonzero(inner)[0]
            k = kids[idx]
            d = hamming(f[idx, None, :], self.descriptor[np.maximum(k, 0)])
            d = np.where(k >= 0, d, 1 << 20)
            node[idx] = k[np.arange(idx.shape[0]), np.argmin(d, axis=1)]  # argmin: the first minimum
        return self.word_of[node].astype(np.int32), self.weight[node].astype(np.float64)


def bow_vector(voc: Vocabulary, features) -> dict:
    """transform(features, v) with TF_IDF, then v.normalize(L1): {word: value} in ascending word id."""
    words, weights = voc.transform(features)
    v = {}
    for wid, w in zip(words.tolist(), weights.tolist()):
        if w > 0:
            if wid in v:
                v[wid] += w  # BowVector::addWeight: once per occurrence
            else:
                v[wid] = w
    v = dict(sorted(v.items()))
    norm = 0.0
    for x in v.values():
        norm += math.fabs(x)
    if norm > 0.0:
        for wid in v:
            v[wid] /= norm
    return v


def vector_arrays(v: dict):
    return np.array(list(v.keys()), np.int32), np.array(list(v.values()), np.float64)


def l1_score(v1: dict, v2: dict) -> float:
    """L1Scoring::score."""
    k1, k2 = list(v1.items()), list(v2.items())
    i = j = 0
    score = 0.0
    while i < len(k1) and j < len(k2):
        (w1, vi), (w2, wi) = k1[i], k2[j]
        if w1 == w2:
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            i += 1
            j += 1
        elif w1 < w2:
            i += 1
        else:
            j += 1
    return -score / 2.0


class Database:
    """DBoW3::Database without a direct index: an inverted file word -> [(entry id, value)]."""

    def __init__(self, voc: Vocabulary):
        self.voc = voc
        self.ifile = {}
        self.n = 0
        self.vectors = []

    def add_vector(self, v: dict) -> int:
        eid = self.n
        self.n += 1
        self.vectors.append(v)
        for wid, val in v.items():
            self.ifile.setdefault(wid, []).append((eid, val))
        return eid

    def add(self, features) -> int:
        return self.add_vector(bow_vector(self.voc, features))

    def query_vector(self, vec: dict, max_results: int, max_id: int):
        """Database::queryL1 -> [(entry id, score)], best first."""
        pairs = {}
        for wid, q in vec.items():  # ascending word id
            for eid, d in self.ifile.get(wid, ()):
                if eid < max_id or max_id == -1:
                    value = math.fabs(q - d) - math.fabs(q) - math.fabs(d)
                    if eid in pairs:
                        pairs[eid] += value
                    else:
                        pairs[eid] = value
        ret = sorted(pairs.items(), key=lambda r: (r[1], r[0]))  # ascending; equal scores: lower id first
        if max_results > 0:
            ret = ret[:max_results]
        return [(eid, -s / 2.0) for eid, s in ret]


def decide(ret, i: int, cfg: dict):
    """detectLoop after its query -> (loop id, the events it went through)."""
    gap, th = cfg["min_loop_search_gap"], cfg["min_loop_bow_threshold"]
    ev = set()
    if i - gap < 0:
        ev.add("before_gap")
        if i <= cfg["min_frame_index"]:
            ev.add("i_small")
        return -1, ev
    if len(ret) < 1:
        ev.add("empty")
    elif not ret[0][1] > th:
        ev.add("ret0_low")
    find = len(ret) >= 1 and ret[0][1] > th and any(r[1] > th for r in ret[1:])
    if len(ret) >= 1 and ret[0][1] > th and not find:
        ev.add("only_ret0")
    if i <= cfg["min_frame_index"]:
        ev.add("i_small")
    if find and i > cfg["min_frame_index"]:
        m = -1
        for eid, score in ret:
            if m == -1 or (eid < m and score > cfg["index_score_threshold"]):
                if m != -1:
                    ev.add("takeover")
                m = eid
            elif eid < m and score > th:
                ev.add("refused")
        if m < cfg["loop_index_bound"]:
            ev.add("loop")
            return m, ev
        ev.add("beyond_bound")
        return -1, ev
    return -1, ev


def detect_loop(db: Database, features, i: int, cfg: dict):
    """detectLoop(image, descriptors, i): query, add, decide -> (loop id, ret, events)."""
    vec = bow_vector(db.voc, features)
    ret = db.query_vector(vec, cfg["max_results"], i - cfg["min_loop_search_gap"])
    db.add_vector(vec)
    loop, ev = decide(ret, i, cfg)
    return loop, ret, ev


def query_limit(k: int, gap: int) -> int:
    """How many of the k earlier entries query(.., max_id = k - gap) considers."""
    max_id = k - gap
    if max_id == -1:
        return k
    return max(0, min(k, max_id))


def closed_form_detect(vectors, k: int, cfg: dict):
    """The same result from the stored vectors alone: entry k against the entries below its limit."""
    qw, qv = vector_arrays(vectors[k])
    cand = []
    for e in range(query_limit(k, cfg["min_loop_search_gap"])):
        ew, evals = vector_arrays(vectors[e])
        qp, acc, found = 0, 0.0, False
        for j in range(ew.shape[0]):
            while qp < qw.shape[0] and qw[qp] < ew[j]:
                qp += 1
            if qp == qw.shape[0]:
                break
            if qw[qp] == ew[j]:
                q, d = float(qv[qp]), float(evals[j])
                value = math.fabs(q - d) - math.fabs(q) - math.fabs(d)
                acc = acc + value if found else value
                found = True
        if found:
            cand.append((e, acc))
    cand.sort(key=lambda r: (r[1], r[0]))
    ret = [(e, -s / 2.0) for e, s in cand[:cfg["max_results"]]]
    loop, ev = decide(ret, k, cfg)
    return loop, ret, ev


def run_stateful(voc: Vocabulary, keyframes, cfg: dict):
    """detect_loop once per keyframe -> ([loop], [ret], [events], db)."""
    db = Database(voc)
    loops, rets, events = [], [], []
    for i, f in enumerate(keyframes):
        loop, ret, ev = detect_loop(db, f, i, cfg)
        loops.append(loop)
        rets.append(ret)
        events.append(ev)
    return loops, rets, events, db
