"""Seeded vocabularies, descriptor sets and keyframe sequences for the bag-of-words tests
(test_bow_cpu.py, test_gpu_bow.py).  Everything is built once per process and shared."""
from __future__ import annotations

import functools

import numpy as np

import restate_bow as RB

SCRIPT_CFG = dict(RB.DEFAULTS, min_loop_search_gap=5, min_loop_bow_threshold=0.013)
COUNTS = (0, 1, 63, 64, 65, 1000)


def _relabel(parent, descriptor, weight, rng):
    """Shuffle the node ids inside every level, so siblings are not contiguous and the children of
    different parents interleave; a parent keeps a smaller id than its children."""
    n = len(parent)
    depth = np.zeros(n, np.int64)
    for i in range(1, n):
        depth[i] = depth[parent[i]] + 1
    order = np.lexsort((rng.random(n), depth))  # old ids in their new order
    new_of = np.empty(n, np.int64)
    new_of[order] = np.arange(n)
    par = np.full(n, -1, np.int32)
    for old in range(1, n):
        par[new_of[old]] = new_of[parent[old]]
    return par, descriptor[order], weight[order]


def _weights(n, rng, lo, hi, zero_fraction):
    w = rng.uniform(lo, hi, n)
    w[rng.random(n) < zero_fraction] = 0.0
    return w


def balanced(k: int, L: int, seed: int, lo=0.2, hi=3.0, zero_fraction=0.1):
    """A full k-ary tree of depth L with random descriptors and weights."""
    rng = np.random.default_rng(seed)
    parent = [-1]
    level = [0]
    for _ in range(L):
        nxt = []
        for p in level:
            for _ in range(k):
                parent.append(p)
                nxt.append(len(parent) - 1)
        level = nxt
    n = len(parent)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return _relabel(np.array(parent, np.int32), desc, _weights(n, rng, lo, hi, zero_fraction), rng)


def unbalanced(seed: int = 7):
    """k = 4, L = 3: leaves at depth 1, 2 and 3, a node with a single child, two siblings with
    identical descriptors, some weight-0 words."""
    rng = np.random.default_rng(seed)
    #          0   1  2  3  4    5      6  7  8  9    10 11    12 13 14 15   16 17
    parent = [-1,  0, 0, 0, 0,   2,     3, 3, 3, 3,   4, 4,    5, 5, 5, 5,   10, 10]
    # node 1: a leaf at depth 1; node 2: a single child (5) whose four children are leaves at depth 3;
    # node 3: four leaf children at depth 2 (7 and 8 identical); node 4: a leaf (11) beside an inner
    # node (10) with two leaves at depth 3
    n = len(parent)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[8] = desc[7]
    desc[3] = desc[7]  # so desc[7] itself descends to node 3 and meets the tie there
    w = rng.uniform(0.2, 3.0, n)
    w[[6, 13, 17]] = 0.0
    return np.array(parent, np.int32), desc, w  # ids as written: siblings 7 and 8 must keep their order


@functools.lru_cache(maxsize=None)
def vocabulary(name: str):
    """-> (parent, descriptor, weight)."""
    if name == "k2L1":
        p, d, w = balanced(2, 1, 1, zero_fraction=0.0)
        w[2] = 0.0
        return p, d, w
    if name == "unbalanced":
        return unbalanced()
    if name == "k10L3":
        return balanced(10, 3, 3)
    if name == "k17L2":
        return balanced(17, 2, 4)
    if name == "k64L1":
        return balanced(64, 1, 5)
    if name == "k4L2":  # smoke-sized
        return balanced(4, 2, 6, zero_fraction=0.0)
    if name == "script":  # 100,000 words of nearly equal weight: two keyframes share the words they were given, no others
        return balanced(10, 5, 8, lo=0.95, hi=1.05, zero_fraction=0.02)
    raise KeyError(name)


VOCABULARIES = ("k2L1", "unbalanced", "k10L3", "k17L2", "k64L1")


@functools.lru_cache(maxsize=None)
def restated(name: str) -> RB.Vocabulary:
    return RB.Vocabulary(*vocabulary(name))


def equidistant(voc: RB.Vocabulary, rng, n: int = 8):
    """Descriptors at equal Hamming distance from two siblings (children of the root, then of its
    inner children): half of the bits the two differ in are taken from each."""
    out = []
    parents = [0] + [c for c in voc.children[0] if voc.children[c]]
    for p in parents:
        kids = voc.children[p]
        for a in range(len(kids)):
            for b in range(a + 1, len(kids)):
                if len(out) >= n:
                    break
                da = np.unpackbits(voc.descriptor[kids[a]])
                db = np.unpackbits(voc.descriptor[kids[b]])
                diff = np.nonzero(da != db)[0]
                if diff.shape[0] % 2:
                    continue
                x = da.copy()
                flip = rng.permutation(diff)[:diff.shape[0] // 2]
                x[flip] = db[flip]
                out.append(np.packbits(x))
    return np.array(out, np.uint8).reshape(-1, 32)


@functools.lru_cache(maxsize=None)
def descriptor_sets(name: str):
    """{set name: (n, 32) uint8} for one vocabulary."""
    voc = restated(name)
    rng = np.random.default_rng(100 + VOCABULARIES.index(name))
    sets = {f"random{c}": rng.integers(0, 256, (c, 32), dtype=np.uint8) for c in COUNTS}
    sets["nodes"] = voc.descriptor[1:].copy()
    sets["equidistant"] = equidistant(voc, rng)
    sets["zeros_ones"] = np.concatenate([np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)])
    sets["repeat1000"] = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 1000, axis=0)
    pool = rng.integers(0, 256, (4000, 32), dtype=np.uint8)
    sets["weight0"] = pool[voc.transform(pool)[1] == 0][:40]
    mixed = np.concatenate([sets["random65"], sets["repeat1000"][:30], sets["weight0"][:10], sets["equidistant"]])
    sets["mixed"] = mixed[rng.permutation(mixed.shape[0])]
    return sets


# ---------------------------------------------------------------- the scripted database
N_SCRIPT, N_PER = 70, 500
# keyframe: [(source keyframe, descriptors copied from the source's own fresh ones)]
SCRIPT = {
    4: [(0, 150), (1, 100)],           # i - gap == -1: an unrestricted query with results, yet -1
    8: [(1, 3)],                       # ret[0] at or below th
    10: [(2, 250)],                    # only ret[0] above th
    20: [(6, 150), (7, 150)],          # m >= 6: -1
    22: [(3, 150), (1, 100)],          # ret[0] = 3, then the lower id 1 takes over: 1
    25: [(4, 150), (7, 100), (2, 7)],  # ret[0] = 4; id 2 scores above th but not above 0.015: refused, 4
    30: [(0, 200), (9, 100)],          # 0
    35: [(12, 150), (5, 100)],         # ret[0] = 12, 5 takes over: 5
    40: [(2, 8), (3, 6)],              # one result above th, one below: only ret[0]
    45: [(13, 100), (14, 120)],        # m >= 6
    49: [(8, 40), (0, 30)],            # ret[0] = 8, 0 takes over: 0 (gap 50: the unrestricted query of i - gap == -1)
    60: [(22, 200), (3, 120), (1, 90)],  # ret[0] = 22, then 3, then 1 take over: 1
}
SCRIPT_EMPTY = 50      # a keyframe without descriptors
SCRIPT_WEIGHT0 = 55    # a keyframe whose words all weigh 0


@functools.lru_cache(maxsize=None)
def scripted_keyframes():
    """70 keyframes over the "script" vocabulary.  Fresh descriptors land on words no earlier
    keyframe uses (and of positive weight), so two keyframes share exactly the words one copied from
    the other."""
    voc = restated("script")
    rng = np.random.default_rng(2024)
    used = set()
    zero_pool = []

    def fresh(n):
        out = []
        while len(out) < n:
            cand = rng.integers(0, 256, (2 * (n - len(out)) + 16, 32), dtype=np.uint8)
            words, weights = voc.transform(cand)
            for d, wid, w in zip(cand, words.tolist(), weights.tolist()):
                if w == 0:
                    zero_pool.append(d)
                elif wid not in used and len(out) < n:
                    used.add(wid)
                    out.append(d)
        return np.array(out, np.uint8)

    own, cursor, frames = {}, {}, []
    for i in range(N_SCRIPT):
        if i == SCRIPT_EMPTY:
            frames.append(np.zeros((0, 32), np.uint8))
            continue
        if i == SCRIPT_WEIGHT0:
            frames.append(None)  # filled below, once the pool is known
            continue
        parts = []
        for src, cnt in SCRIPT.get(i, ()):
            c0 = cursor.get(src, 0)
            assert c0 + cnt <= own[src].shape[0]
            parts.append(own[src][c0:c0 + cnt])
            cursor[src] = c0 + cnt
        own[i] = fresh(N_PER - sum(p.shape[0] for p in parts))
        f = np.concatenate(parts + [own[i]])
        frames.append(f[rng.permutation(f.shape[0])])
    assert len(zero_pool) >= 20
    frames[SCRIPT_WEIGHT0] = np.array(zero_pool[:20], np.uint8)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def random_keyframes(n: int = 200, seed: int = 11):
    """Keyframes of 20..150 random descriptors (every 37th empty) for the k10L3 vocabulary: they all
    share words with one another."""
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (0 if k % 37 == 36 else int(rng.integers(20, 151)), 32), dtype=np.uint8)
                 for k in range(n))
