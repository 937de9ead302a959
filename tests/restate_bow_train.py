"""Restatement of DBoW3's vocabulary training in numpy / pure Python: ``Vocabulary::create`` after the
published library (rmsalinas/DBoW3 Vocabulary.cpp: HKmeansStep, initiateClustersKMpp, createWords,
setNodeWeights; DescManip::meanValue) for binary 32-byte descriptors and TF_IDF weights.  DBoW3 is on
no machine of this project: this text is unpinned against the library; the GPU (lislam_bow_train) is
pinned against this text, by equality of bytes.

Two forms:
  * ``train_recursive``: the literal depth-first HKmeansStep with a Python list of descriptor indices
    per node; node ids come out in DBoW3's order by construction;
  * ``train_levels``: what the kernels do.  All nodes of a level are seeded, then iterated together
    until no assignment of the level changes; ids are level order and are renumbered at the end.

Rules (the same text as lislam_bow.hip's training header):
  * a node's descriptors keep their original order (image, then row); every partition is stable;
  * <= k descriptors: each its own child, duplicates not merged; otherwise k-means++ seeding, then
    assign, then (means, assign) until an assignment equals the previous one or ``max_iterations``
    assignments were made (ours: DBoW3 has no limit);
  * assignment: the first centre with the smallest Hamming distance (strict <);
  * mean: bit b set iff at least n // 2 + n % 2 of the n members have it; an empty cluster keeps its
    centre (ours: DBoW3 is undefined there);
  * k-means++ on plain distances, integers throughout; S == 0 ends the seeding with fewer centres;
  * draws (ours: DBoW3 calls rand() in visiting order): counter-based, keyed by the node,
    key(root) = splitmix64(seed), key(child c) = splitmix64(key ^ (c + 1)),
    draw j = splitmix64(key + j * GOLDEN), reduced to [0, n) as ((x >> 32) * n) >> 32;
  * a child recurses if it holds more than one descriptor and its level is below L;
  * weight = log(N / Ni) for Ni > 0, else 0; N counts every image added, empty ones too.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

import restate_bow as RB

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB


def splitmix64(x: int) -> int:
    z = (x + GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    return z ^ (z >> 31)


def child_key(key: int, c: int) -> int:
    return splitmix64(key ^ (c + 1))


def draw(key: int, j: int) -> int:
    return splitmix64((key + j * GOLDEN) & MASK)


def reduce(x: int, n: int) -> int:
    return ((x >> 32) * n) >> 32


class Trained(NamedTuple):
    parent: np.ndarray      # (n_nodes,) int32
    descriptor: np.ndarray  # (n_nodes, 32) uint8, the root's zero
    weight: np.ndarray      # (n_nodes,) float64
    leaf_of: np.ndarray     # (n_descriptors,) the node training left each descriptor in
    stats: dict             # level_steps / level_clustered / level_iterations / level_capped: L ints each
    events: dict            # empty_cluster, s_zero: how often the two rules were met


def _stats(L):
    return {key: [0] * L for key in ("level_steps", "level_clustered", "level_iterations", "level_capped")}


def mean_value(rows: np.ndarray) -> np.ndarray:
    """DescManip::meanValue for ORB."""
    n = rows.shape[0]
    return np.packbits(np.unpackbits(rows, axis=1).sum(axis=0) >= n // 2 + n % 2)


def seed_kmpp(rows: np.ndarray, key: int, k: int, events: dict) -> np.ndarray:
    """initiateClustersKMpp -> (<= k, 32) centres."""
    n = rows.shape[0]
    centres = [rows[reduce(draw(key, 0), n)]]
    min_d = RB.hamming(rows, centres[0]).astype(np.int64)
    while len(centres) < k:
        d = RB.hamming(rows, centres[-1])
        upd = min_d > 0
        min_d[upd] = np.minimum(min_d[upd], d[upd])
        S = int(min_d.sum())
        if S == 0:
            events["s_zero"] += 1
            break
        r = 1 + reduce(draw(key, len(centres)), S)
        centres.append(rows[int(np.searchsorted(np.cumsum(min_d), r, side="left"))])  # first prefix >= r
    return np.array(centres, np.uint8)


def assign(rows: np.ndarray, centres: np.ndarray) -> np.ndarray:
    return np.argmin(RB.hamming(rows[:, None, :], centres[None, :, :]), axis=1)  # argmin: the first minimum


def means(rows: np.ndarray, slot: np.ndarray, centres: np.ndarray, events: dict) -> np.ndarray:
    out = centres.copy()
    for c in range(centres.shape[0]):
        members = rows[slot == c]
        if members.shape[0] == 0:
            events["empty_cluster"] += 1
        else:
            out[c] = mean_value(members)
    return out


def weights(parent, descriptor, desc, counts):
    """setNodeWeights(TF_IDF) over the finished tree."""
    n_nodes = len(parent)
    weight = np.zeros(n_nodes, np.float64)
    if n_nodes < 2:
        return weight
    voc = RB.Vocabulary(parent, descriptor, weight)
    words, _ = voc.transform(desc)
    ni = np.zeros(voc.leaf_node.shape[0], np.int64)
    at = 0
    for c in counts:
        ni[np.unique(words[at:at + c])] += 1
        at += c
    N = len(counts)
    for w, cnt in enumerate(ni.tolist()):
        if cnt > 0:
            weight[voc.leaf_node[w]] = math.log(N / cnt)
    return weight


def train_recursive(desc, counts, k: int, L: int, max_iterations: int = 100, seed: int = 0) -> Trained:
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    assert sum(counts) == desc.shape[0]
    parent, descriptor = [-1], [np.zeros(32, np.uint8)]
    leaf_of = np.zeros(desc.shape[0], np.int64)
    stats, events = _stats(L), dict(empty_cluster=0, s_zero=0)

    def step(parent_id, idxs, level, key):  # HKmeansStep(parent_id, descriptors, current_level)
        if not idxs:
            return
        rows = desc[idxs]
        stats["level_steps"][level - 1] += 1
        if len(idxs) <= k:
            centres, groups = rows, [[i] for i in idxs]
        else:
            stats["level_clustered"][level - 1] += 1
            centres = seed_kmpp(rows, key, k, events)
            slot = assign(rows, centres)
            it, capped = 1, True
            while it < max_iterations:
                centres = means(rows, slot, centres, events)
                new = assign(rows, centres)
                it += 1
                same = np.array_equal(new, slot)
                slot = new
                if same:
                    capped = False
                    break
            stats["level_iterations"][level - 1] = max(stats["level_iterations"][level - 1], it)
            stats["level_capped"][level - 1] += int(capped)
            groups = [[i for i, s in zip(idxs, slot.tolist()) if s == c] for c in range(centres.shape[0])]
        first = len(parent)
        for c in range(len(groups)):
            parent.append(parent_id)
            descriptor.append(centres[c].copy())
            leaf_of[groups[c]] = first + c
        if level < L:
            for c, g in enumerate(groups):
                if len(g) > 1:
                    step(first + c, g, level + 1, child_key(key, c))

    step(0, list(range(desc.shape[0])), 1, splitmix64(seed))
    parent, descriptor = np.array(parent, np.int32), np.array(descriptor, np.uint8)
    return Trained(parent, descriptor, weights(parent, descriptor, desc, counts), leaf_of, stats, events)


def train_levels(desc, counts, k: int, L: int, max_iterations: int = 100, seed: int = 0) -> Trained:
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    stats, events = _stats(L), dict(empty_cluster=0, s_zero=0)
    # level-order nodes: [parent (level-order id), descriptor, children (level-order ids)]
    nodes = [[-1, np.zeros(32, np.uint8), []]]
    where = np.zeros(desc.shape[0], np.int64)
    active = [(0, np.arange(desc.shape[0]), splitmix64(seed))] if desc.shape[0] else []
    for level in range(1, L + 1):
        if not active:
            break
        stats["level_steps"][level - 1] = len(active)
        centres, slots, last_changed = [], [], []
        for _, idxs, key in active:  # seeding and the first assignment
            rows = desc[idxs]
            if idxs.shape[0] <= k:
                centres.append(rows.copy())
                slots.append(np.arange(idxs.shape[0]))
                last_changed.append(0)
            else:
                centres.append(seed_kmpp(rows, key, k, events))
                slots.append(assign(rows, centres[-1]))
                last_changed.append(1)
        clustered = [a for a, (_, idxs, _) in enumerate(active) if idxs.shape[0] > k]
        it = 1
        while clustered and it < max_iterations:
            it += 1
            changed = 0
            for a in clustered:  # every node of the level, converged or not: a converged one is a fixed point
                rows = desc[active[a][1]]
                before = dict(events)
                centres[a] = means(rows, slots[a], centres[a], events)
                new = assign(rows, centres[a])
                if np.array_equal(new, slots[a]):
                    if last_changed[a] < it - 1:
                        events.update(before)  # the recursion had left this node: do not count it twice
                else:
                    last_changed[a] = it
                    changed += 1
                slots[a] = new
            if not changed:
                break
        for a in clustered:
            stats["level_iterations"][level - 1] = max(stats["level_iterations"][level - 1],
                                                       min(last_changed[a] + 1, max_iterations))
            stats["level_capped"][level - 1] += int(last_changed[a] == max_iterations)
        stats["level_clustered"][level - 1] = len(clustered)
        nxt = []
        for a, (node, idxs, key) in enumerate(active):
            for c in range(centres[a].shape[0]):
                g = idxs[slots[a] == c]  # boolean masks keep the order: a stable partition
                nodes.append([node, centres[a][c].copy(), []])
                nodes[node][2].append(len(nodes) - 1)
                where[g] = len(nodes) - 1
                if level < L and g.shape[0] > 1:
                    nxt.append((len(nodes) - 1, g, child_key(key, c)))
        active = nxt
    # DBoW3's ids: a step appends all its children, then recurses into child 0, child 1, ...
    new_id = {0: 0}
    parent, descriptor = [-1], [nodes[0][1]]

    def number(node):
        for ch in nodes[node][2]:
            new_id[ch] = len(parent)
            parent.append(new_id[node])
            descriptor.append(nodes[ch][1])
        for ch in nodes[node][2]:
            number(ch)

    number(0)
    parent, descriptor = np.array(parent, np.int32), np.array(descriptor, np.uint8)
    leaf_of = np.array([new_id[int(w)] for w in where], np.int64)
    return Trained(parent, descriptor, weights(parent, descriptor, desc, counts), leaf_of, stats, events)
