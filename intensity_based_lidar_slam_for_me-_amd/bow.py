"""ORB bag-of-words loop detection over the lislam C ABI: ``loopClosureHandler::detectLoop``
(``src/loop_closure_handler.cpp:127-188``, the ``USE_ORBLOOP`` detector that ``keyframeProcessor``
runs at ``:108-111``) with its DBoW3 database device-resident.

``BowDatabase.add_batch`` turns the ORB descriptors of a batch's scans into BoW vectors where they
lie on the device; ``detect`` replays ``detectLoop`` for a whole range of keyframes in one call.
``loop_id`` is what ``loop.loop_closure_icp`` takes as its history keyframe.  The vocabulary is
handed in as arrays (``parent``, ``descriptor``, ``weight`` per tree node); reading DBoW3's files is
the caller's work, or trained here: ``BowTrainer`` is ``DBoW3::Vocabulary::create`` (hierarchical
k-means++ and TF-IDF weights) over the descriptors this front end produces, on the device.  All
compute runs in ``liblislam.so`` on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import native as nat

BowConfig = nat.BowConfig
BowTrainConfig = nat.BowTrainConfig


class Detection(NamedTuple):
    loop_id: np.ndarray  # (n,) int32, -1 = no loop
    ids: list            # n arrays (n_ret,) int32: the query's results, best first
    scores: list         # n arrays (n_ret,) float64


def _rows(desc) -> np.ndarray:
    return np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)


class BowDatabase:
    """``DBoW3::Database`` (TF_IDF, L1_NORM, no direct index) + ``detectLoop``; ``config`` = the
    fields of ``BowConfig`` (defaults: the constants ``detectLoop`` compiles with)."""

    def __init__(self, ctx, parent, descriptor, weight, capacity: int, max_features: int = 1000, **config):
        self.ctx = ctx
        self.cfg = BowConfig(**config)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        des = _rows(descriptor)
        wgt = np.ascontiguousarray(weight, np.float64).reshape(-1)
        if des.shape[0] != par.shape[0] or wgt.shape[0] != par.shape[0]:
            raise ValueError("parent, descriptor and weight must hold one row per node")
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_bow_create(ctx.h, par.shape[0], nat.ptr(par), nat.ptr(des), nat.ptr(wgt), ctypes.byref(self.cfg),
                                            int(capacity), int(max_features), ctypes.byref(h)), ctx.h, "lislam_bow_create")
        self.h = h
        self.max_features = int(max_features)

    def close(self):
        if self.h:
            self.ctx.lib.lislam_bow_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_bow_size(self.h, ctypes.byref(n)), self.ctx.h, "lislam_bow_size")
        return n.value

    def add(self, images) -> None:
        """Database::add of each image's descriptors ((n, 32) uint8) of the list."""
        ds = [_rows(d) for d in images]
        if not ds:
            return
        counts = np.array([d.shape[0] for d in ds], np.int32)
        rows = np.ascontiguousarray(np.concatenate(ds))
        nat.check(self.ctx.lib.lislam_bow_add(self.h, nat.ptr(rows) if rows.size else None, nat.ptr(counts), len(ds)),
                  self.ctx.h, "lislam_bow_add")

    def add_batch(self, batch, first: int, n: int) -> None:
        """The same for the ORB descriptors of scans [first, first + n) of a batch whose
        intensity_odometry has run, on the device."""
        nat.check(self.ctx.lib.lislam_bow_add_batch(self.h, batch.h, int(first), int(n)), self.ctx.h, "lislam_bow_add_batch")

    def add_batch_scans(self, batch, scans) -> None:
        """The ORB descriptors of the listed scans of a batch whose intensity_odometry has run (any order,
        repeats allowed) in one set of launches: what ``add_batch(batch, s, 1)`` for every s would leave."""
        s = np.ascontiguousarray(np.atleast_1d(scans), np.int32).reshape(-1)
        nat.check(self.ctx.lib.lislam_bow_add_batch_scans(self.h, batch.h, nat.ptr(s) if s.size else None, s.shape[0]),
                  self.ctx.h, "lislam_bow_add_batch_scans")

    def detect(self, first: int | None = None, n: int | None = None) -> Detection:
        """detectLoop as it returned when keyframe k was the newest, k in [first, first + n)
        (default: every keyframe), with the results of the query behind it."""
        first = 0 if first is None else int(first)
        n = len(self) - first if n is None else int(n)
        m, R = max(n, 0), self.cfg.max_results
        loop_id, n_ret = np.zeros(m, np.int32), np.zeros(m, np.int32)
        ids, scores = np.zeros((m, R), np.int32), np.zeros((m, R), np.float64)
        nat.check(self.ctx.lib.lislam_bow_detect(self.h, first, n, nat.ptr(loop_id), nat.ptr(n_ret), nat.ptr(ids),
                                                 nat.ptr(scores)), self.ctx.h, "lislam_bow_detect")
        return Detection(loop_id, [ids[k, :n_ret[k]].copy() for k in range(m)], [scores[k, :n_ret[k]].copy() for k in range(m)])

    def detect_loop(self, descriptors) -> int:
        """detectLoop for one keyframe: query, add, decide -> loop id or -1."""
        self.add([descriptors])
        return int(self.detect(len(self) - 1, 1).loop_id[0])

    def score(self, a, b) -> np.ndarray:
        """L1Scoring::score(vector[a[k]], vector[b[k]]) -> (n,) float64 in [0, 1]."""
        ia = np.ascontiguousarray(np.atleast_1d(a), np.int32)
        ib = np.ascontiguousarray(np.atleast_1d(b), np.int32)
        if ia.shape != ib.shape:
            raise ValueError("a and b must hold the same number of indices")
        out = np.zeros(ia.shape[0], np.float64)
        nat.check(self.ctx.lib.lislam_bow_score(self.h, nat.ptr(ia), nat.ptr(ib), ia.shape[0], nat.ptr(out)), self.ctx.h,
                  "lislam_bow_score")
        return out

    def transform(self, descriptors):
        """Vocabulary::transform of each descriptor -> (word_id (n,) int32, weight (n,) float64)."""
        rows = _rows(descriptors)
        word, weight = np.zeros(rows.shape[0], np.int32), np.zeros(rows.shape[0], np.float64)
        nat.check(self.ctx.lib.lislam_bow_transform(self.h, nat.ptr(rows) if rows.size else None, rows.shape[0], nat.ptr(word),
                                                    nat.ptr(weight)), self.ctx.h, "lislam_bow_transform")
        return word, weight

    def _download(self, what, index, dtype):
        buf = np.zeros(self.max_features, dtype)
        n = ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_bow_download(self.h, what, int(index), nat.ptr(buf), buf.shape[0], ctypes.byref(n)),
                  self.ctx.h, "lislam_bow_download")
        return buf[:n.value].copy()

    def bow_vector(self, i: int):
        """Entry i's BoW vector -> (words (len,) int32 ascending, values (len,) float64)."""
        return self._download(nat.BOW_WORDS, i, np.int32), self._download(nat.BOW_VALUES, i, np.float64)


class Vocabulary(NamedTuple):
    parent: np.ndarray      # (n_nodes,) int32, -1 for the root; parent[i] < i, children consecutive
    descriptor: np.ndarray  # (n_nodes, 32) uint8
    weight: np.ndarray      # (n_nodes,) float64: log(N / Ni) for words, 0 for inner nodes


class TrainStats(NamedTuple):
    n_nodes: int
    n_words: int
    n_zero_words: int
    level_steps: list       # per level that ran: HKmeansStep calls
    level_clustered: list   # ... of which with more than k descriptors (k-means)
    level_iterations: list  # ... their largest iteration count
    level_capped: list      # ... how many stopped at max_iterations
    level_ms: list
    phase_ms: list          # per level {seed, assign, means, partition}; zeros unless train(profile=True)
    weights_ms: float
    total_ms: float         # the whole lislam_bow_train call on the host's clock


class BowTrainer:
    """``DBoW3::Vocabulary::create`` (k-means++ per node, TF_IDF) over the descriptors of up to
    ``cap_images`` images, device-resident.  The deviations from DBoW3 (keyed random draws, empty
    clusters, the iteration cap) are in ``include/lislam.h``."""

    def __init__(self, ctx, cap_images: int, cap_descriptors: int):
        self.ctx = ctx
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_bow_trainer_create(ctx.h, int(cap_images), int(cap_descriptors), ctypes.byref(h)), ctx.h,
                  "lislam_bow_trainer_create")
        self.h = h
        self.stats = None
        self.vocabulary = None

    def close(self):
        if self.h:
            self.ctx.lib.lislam_bow_trainer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """-> (images, descriptors) added so far."""
        ni, nd = ctypes.c_int32(), ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_bow_trainer_size(self.h, ctypes.byref(ni), ctypes.byref(nd)), self.ctx.h,
                  "lislam_bow_trainer_size")
        return ni.value, nd.value

    def add(self, images) -> None:
        """Each image's descriptors ((n, 32) uint8) of the list; an empty image counts towards N."""
        ds = [_rows(d) for d in images]
        if not ds:
            return
        counts = np.array([d.shape[0] for d in ds], np.int32)
        rows = np.ascontiguousarray(np.concatenate(ds))
        nat.check(self.ctx.lib.lislam_bow_trainer_add(self.h, nat.ptr(rows) if rows.size else None, nat.ptr(counts), len(ds)),
                  self.ctx.h, "lislam_bow_trainer_add")

    def add_batch(self, batch, first: int, n: int) -> None:
        """The ORB descriptors of scans [first, first + n) of a batch whose intensity_odometry has
        run, read where they lie on the device."""
        nat.check(self.ctx.lib.lislam_bow_trainer_add_batch(self.h, batch.h, int(first), int(n)), self.ctx.h,
                  "lislam_bow_trainer_add_batch")

    def train(self, k: int = 10, L: int = 5, max_iterations: int = 100, seed: int = 0, profile: bool = False) -> Vocabulary:
        """-> Vocabulary(parent, descriptor, weight), node ids in DBoW3's order; ``stats`` is filled.
        Without descriptors the tree is the root alone, which ``BowDatabase`` rejects."""
        cfg = BowTrainConfig(int(k), int(L), int(max_iterations), int(seed))
        st = nat.BowTrainStats()
        st.profile = int(bool(profile))
        n = ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_bow_train(self.h, ctypes.byref(cfg), ctypes.byref(n), ctypes.byref(st)), self.ctx.h,
                  "lislam_bow_train")
        parent, desc, weight = np.zeros(n.value, np.int32), np.zeros((n.value, 32), np.uint8), np.zeros(n.value, np.float64)
        nat.check(self.ctx.lib.lislam_bow_trainer_vocabulary(self.h, n.value, nat.ptr(parent), nat.ptr(desc), nat.ptr(weight)),
                  self.ctx.h, "lislam_bow_trainer_vocabulary")
        m = st.n_levels
        self.stats = TrainStats(st.n_nodes, st.n_words, st.n_zero_words, list(st.level_steps)[:m], list(st.level_clustered)[:m],
                                list(st.level_iterations)[:m], list(st.level_capped)[:m], list(st.level_ms)[:m],
                                [dict(zip(nat.BOW_PHASES, st.phase_ms[i])) for i in range(m)], st.weights_ms, st.total_ms)
        self.vocabulary = Vocabulary(parent, desc, weight)
        return self.vocabulary

    def database(self, capacity: int, max_features: int = 1000, **config) -> BowDatabase:
        """A ``BowDatabase`` over the vocabulary of the last ``train``."""
        if self.vocabulary is None:
            raise RuntimeError("BowTrainer.database: call train first")
        return BowDatabase(self.ctx, *self.vocabulary, capacity=capacity, max_features=max_features, **config)
