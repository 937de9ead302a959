"""CPU restatement of mapOptimization's ORB keyframe sliding window (src/mapOptimization.cpp:155-169,
:295-361, :481-493), stated literally: a brute-force L2 argmin, Python's stable ``sorted``, the
double-precision G, the 0.3 m gate, a deque.  The arithmetic that must match the oracle's mapopt step
bit for bit (pose composition, point transforms, the Ceres restatement over a mixed record list) is
tests/cpp/mapwin_restate.cpp, built by __graft_entry__.build() into
tests/cpp/build/libmapwin_restate.so.  A missing library raises: the tests that need it fail, they do
not skip."""
from __future__ import annotations

import ctypes
import os
from collections import deque
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "cpp", "build", "libmapwin_restate.so")

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built; run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp = ctypes.c_void_p
        L.mapwin_solve.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp]
        L.mapwin_compose.argtypes = [vp, vp, vp]
        L.mapwin_update.argtypes = [vp, vp, vp]
        L.mapwin_to_world.argtypes = [vp, vp, ctypes.c_int, vp]
        L.mapwin_point_world.argtypes = [vp, vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def solve(rec, kind, x0, max_iterations=10):
    """ceres::Solve over the records in list order: (x (7,), (iterations, termination))."""
    r = _f64(rec).reshape(-1, 9)
    k = np.ascontiguousarray(kind, np.int32)
    x = np.array(x0, np.float64)
    s = np.zeros(2, np.int32)
    lib().mapwin_solve(_p(r), _p(k), r.shape[0], _p(x), max_iterations, _p(s))
    return x, s


def compose(state, odom):
    x = np.zeros(7)
    lib().mapwin_compose(_p(_f64(state)), _p(_f64(odom)), _p(x))
    return x


def update(x, odom):
    st = np.zeros(7)
    lib().mapwin_update(_p(_f64(x)), _p(_f64(odom)), _p(st))
    return st


def to_world(x, pts):
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    w = np.zeros_like(p)
    lib().mapwin_to_world(_p(_f64(x)), _p(p), p.shape[0], _p(w))
    return w


def point_world(x, p):
    w = np.zeros(3)
    lib().mapwin_point_world(_p(_f64(x)), _p(np.ascontiguousarray(p[:3], np.float32)), _p(w))
    return w


# ------------------------------------------------------------------ step 1: the features' zero filter
def keeps_point(track):
    """extractPointsAndFilterZeroValue, mapOptimization's variant (:620): a keypoint is dropped only
    when |x| < 0.01 && |y| < 0.01 && |z| < 0.01 of its cloud_track point (abs(float) compared with the
    double 0.01).  Returns the keep flag of every point of `track`."""
    t = np.asarray(track, np.float32).reshape(-1, 4).astype(np.float64)
    return ~((np.abs(t[:, 0]) < 0.01) & (np.abs(t[:, 1]) < 0.01) & (np.abs(t[:, 2]) < 0.01))


# ------------------------------------------------------------------ step 2: the window loop
def l2_match(qdesc, tdesc):
    """cv::BFMatcher() (NORM_L2, no cross-check) .match(query, train): per query the train row of
    the smallest sum of squared byte differences, the first in train order among equals.
    Returns (train index (nq,), integer sum (nq,)); an empty list when either side is empty."""
    q = np.asarray(qdesc, np.uint8).reshape(-1, 32).astype(np.int64)
    t = np.asarray(tdesc, np.uint8).reshape(-1, 32).astype(np.int64)
    if len(q) == 0 or len(t) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    idx = np.zeros(len(q), np.int64)
    best = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        s = ((t - q[i]) ** 2).sum(1)
        j = 0
        for k in range(1, len(s)):  # strict <: the first minimum wins
            if s[k] < s[j]:
                j = k
        idx[i], best[i] = j, s[j]
    return idx, best


def l2_match_fast(qdesc, tdesc):
    """The same result through numpy (argmin returns the first minimum); test_mapwin_cpu checks it
    against l2_match."""
    q = np.asarray(qdesc, np.uint8).reshape(-1, 32).astype(np.int64)
    t = np.asarray(tdesc, np.uint8).reshape(-1, 32).astype(np.int64)
    if len(q) == 0 or len(t) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    s = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    idx = s.argmin(1)
    return idx, s[np.arange(len(q)), idx]


def good_count(M: int) -> int:
    """for (size_t i = 0; i < matches.size() * 0.2; ++i) (:314): the comparison is in double."""
    i = 0
    while float(i) < float(M) * 0.2:
        i += 1
    return i


@dataclass
class Keyframe:
    desc: np.ndarray  # (n, 32) uint8
    p3d: np.ndarray   # (n, 4) float32, sensor frame
    pose: np.ndarray  # (7,) q_map_cur_tk, t_map_cur_tk


def window_records(window, desc, p3d, pose, match=l2_match_fast):
    """:295-361 for the current keyframe (desc, p3d) at `pose` against `window` (oldest first).
    Blocks in the fixed order: window keyframes newest to oldest, matches in sorted order.
    Returns (rec (n, 9), info (len(window), 6), pairs (n, 3), gate distances (list, every candidate))."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    p3d = np.asarray(p3d, np.float32).reshape(-1, 4)
    rec, info, pairs, dists = [], [], [], []
    for w, kf in enumerate(reversed(window)):  # rbegin .. rend
        nt, nq = len(kf.desc), len(desc)
        idx, ssum = match(desc, kf.desc)
        M = len(idx)
        row = [nt, M, good_count(M), 0, 0, len(rec)]
        if M > 100:  # :309
            dist = np.sqrt(ssum.astype(np.float32))  # DMatch::distance
            order = sorted(range(M), key=lambda i: dist[i])  # std::sort, equal distances in query order
            G = row[2]
            if G > 50 and G != M and nt != nq:  # :327
                row[3] = 1
                for i in order[:G]:
                    prev_w = point_world(kf.pose, kf.p3d[idx[i]])
                    cur_w = point_world(pose, p3d[i])
                    d = float(np.sqrt(((prev_w - cur_w) ** 2).sum()))
                    dists.append(d)
                    if d > 0.3:
                        continue
                    rec.append(np.concatenate([p3d[i, :3].astype(np.float64), prev_w, np.zeros(3)]))
                    pairs.append((w, i, int(idx[i])))
                    row[4] += 1
        info.append(row)
    return (np.array(rec, np.float64).reshape(-1, 9), np.array(info, np.int32).reshape(-1, 6),
            np.array(pairs, np.int32).reshape(-1, 3), dists)


# ------------------------------------------------------------------ steps 1-4: the whole callback
@dataclass
class MapOptimization:
    """mapOptimizationCallback over the oracle's ikd-Tree restatement (oracle.IkdMap,
    oracle.voxel_grid): the ground planes and the window's FeatureMatchingResiduals in one problem."""
    oracle: object
    sliding_window_size: int = 0
    downsample: float = 0.4
    corner_downsample: float = 0.8
    state: np.ndarray = field(default_factory=lambda: np.array([0, 0, 0, 1, 0, 0, 0], np.float64))

    def __post_init__(self):
        self.map = self.oracle.IkdMap(self.downsample)
        self.corner_map = self.oracle.IkdMap(self.corner_downsample)
        self.window = deque()
        self.last_records = None

    def callback(self, ground, odom, corner=None, features=None):
        """Returns (pose (7,), summary (5,) = planes, iterations, termination (-1: built), feature
        blocks, window keyframes used)."""
        O = self.oracle
        g = np.ascontiguousarray(ground, np.float32).reshape(-1, 4)
        c = np.ascontiguousarray(corner if corner is not None else np.zeros((0, 4)), np.float32).reshape(-1, 4)
        desc, p3d = features if features is not None else (np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.float32))
        x = compose(self.state, odom)  # transformAssociateToMap (:112)
        x0 = x.copy()
        new = Keyframe(np.array(desc, np.uint8).reshape(-1, 32), np.array(p3d, np.float32).reshape(-1, 4), x0.copy())
        if self.map.size() == 0:  # :173-196: Build, nothing is pushed (:218, :561)
            self.map.build(to_world(x, g))
            if len(c):
                self.corner_map.build(to_world(x, c))
            return x, np.array([0, 0, -1, 0, 0], np.int32)
        frec, info, pairs, _ = window_records(list(self.window), new.desc, new.p3d, x0)
        self.last_records = (frec, info, pairs)
        g4 = g.copy()
        g4[:, 3] = 0
        vox = O.voxel_grid(g4, 0.8)
        prec, pkind = self.map.associate(1, vox, x)
        keep = pkind >= 0
        rec = np.concatenate([frec, prec[keep]])
        kind = np.concatenate([np.full(len(frec), 3, np.int32), pkind[keep].astype(np.int32)])
        x, s = solve(rec, kind, x, 10)
        conv = s[1] == 1
        if conv:
            self.state = update(x, odom)  # transformUpdate (:448-450)
        key = x if conv else x0
        self.map.add_points(to_world(key, vox), True)
        if len(c):
            self.corner_map.add_points(to_world(key, c), True)
        new.pose = np.array(key, np.float64)  # :481-485
        self.window.append(new)
        if len(self.window) > self.sliding_window_size:
            self.window.popleft()
        return x, np.array([int(keep.sum()), s[0], s[1], len(frec), int(info[:, 3].sum()) if len(info) else 0], np.int32)
