"""Restatement (numpy / pure Python) of the reference's Scan Context place recognition
(include/Scancontext.h, src/Scancontext.cpp), the checker of the GPU place database
(lislam_place_*).  Test infrastructure only.

Every reference expression carries its float32 / float64 type explicitly.  ``SCManager`` is
stateful as the reference's is: it keeps ``tree_making_period_conter`` and the snapshot of ring
keys its "tree" was last built over, so the closed-form prefix the kernels use
(``tree_prefix``) is checked against the real call sequence.

Orders the reference leaves to Eigen / nanoflann are fixed here exactly as in the kernels:
dot products and norms run sequentially in the ring index, the sums over columns sequentially in
the sector index, all in plain double without FMA; the k-nearest search is exact, in nanoflann's
float accumulation (L2_Adaptor::evalMetric, nanoflann.hpp:383-408), equal distances by lower index.
"""
from __future__ import annotations

import math

import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN = -(2 ** 31)
NO_POINT = -1000.0

DEFAULTS = dict(lidar_height=2.0, num_ring=20, num_sector=60, max_radius=80.0, num_exclude_recent=50,
                num_candidates=10, search_ratio=0.1, dist_thres=0.13, tree_making_period=50)


def _atan64(v):
    """libm's double atan, element by element (numpy's vectorized arctan may be another routine)."""
    return np.fromiter(map(math.atan, np.asarray(v, f64).tolist()), f64, count=len(v))


def xy2theta(x, y):
    """xy2theta (:25-42) of float32 arrays -> (float32 angle, defined mask).  The four branches in the
    source's order (-0.0 counts as >= 0); the quotient is float, atan and the scaling by 180 / M_PI
    double, the result narrows to float on return.  A NaN x or y takes no branch: the reference
    falls off the function's end there (undefined); ``defined`` is False and the point is skipped."""
    x = np.asarray(x, f32)
    y = np.asarray(y, f32)
    K = f64(180.0) / f64(math.pi)
    out = np.full(x.shape, np.nan, f64)
    b1 = (x >= 0) & (y >= 0)
    b2 = (x < 0) & (y >= 0)
    b3 = (x < 0) & (y < 0)
    b4 = (x >= 0) & (y < 0)
    with np.errstate(all="ignore"):
        out[b1] = K * _atan64((y[b1] / x[b1]).astype(f32))
        out[b2] = 180.0 - K * _atan64((y[b2] / (-x[b2])).astype(f32))
        out[b3] = 180.0 + K * _atan64((y[b3] / x[b3]).astype(f32))
        out[b4] = 360.0 - K * _atan64(((-y[b4]) / x[b4]).astype(f32))
    return out.astype(f32), b1 | b2 | b3 | b4


def _int_ceil(v):
    """int(ceil(double)) as the reference's x86-64 build converts it (cvttsd2si): NaN and values
    out of int range give INT_MIN."""
    c = np.ceil(v)
    bad = ~np.isfinite(c) | (c >= 2.0 ** 31) | (c < -(2.0 ** 31))
    return np.where(bad, f64(INT_MIN), np.where(bad, 0.0, c)).astype(np.int64)


def bins(points, cfg=DEFAULTS):
    """Per point of (n, 4) float32: (keep mask, ring index 0-based, sector index 0-based, float32 height)."""
    p = np.asarray(points, f32).reshape(-1, 4)
    R, S = int(cfg["num_ring"]), int(cfg["num_sector"])
    max_radius = f64(cfg["max_radius"])
    x, y = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        z = (p[:, 2].astype(f64) + f64(cfg["lidar_height"])).astype(f32)
        rng = np.sqrt(x * x + y * y)  # float products, float sum, float sqrt
        ang, defined = xy2theta(x, y)
        keep = defined & ~(rng.astype(f64) > max_radius)
        ring = np.maximum(np.minimum(R, _int_ceil(rng.astype(f64) / max_radius * f64(R))), 1)
        sector = np.maximum(np.minimum(S, _int_ceil(ang.astype(f64) / 360.0 * f64(S))), 1)
    return keep, ring - 1, sector - 1, z


def make_scancontext(points, cfg=DEFAULTS):
    """makeScancontext (:160-204): (R, S) float64 holding float32 values."""
    R, S = int(cfg["num_ring"]), int(cfg["num_sector"])
    keep, ring, sector, z = bins(points, cfg)
    desc = np.full(R * S, NO_POINT, f64)
    m = keep & ~np.isnan(z)  # `desc < pt.z` is false for a NaN height: it never wins
    np.maximum.at(desc, ring[m] * S + sector[m], z[m].astype(f64))
    desc[desc == NO_POINT] = 0.0
    return desc.reshape(R, S)


def ring_key(desc):
    """makeRingkeyFromScancontext (:206-219) narrowed to float as eig2stdvec does."""
    return (_seq_sum(desc.T) / f64(desc.shape[1])).astype(f32)


def _seq_sum(m):
    """Sum of the rows of m, one after the other."""
    acc = np.zeros(m.shape[1], f64)
    for r in range(m.shape[0]):
        acc = acc + m[r]
    return acc


def sector_key(desc):
    """makeSectorkeyFromScancontext (:222-235): column means in double."""
    return _seq_sum(desc) / f64(desc.shape[0])


def column_norms(desc):
    acc = np.zeros(desc.shape[1], f64)
    for r in range(desc.shape[0]):
        acc = acc + desc[r] * desc[r]
    return np.sqrt(acc)


def fast_align(vkey1, vkey2):
    """fastAlignUsingVkey (:104-124): strict <, so the lowest shift wins ties."""
    S = vkey1.shape[0]
    j = np.arange(S)
    sh = np.arange(S)[:, None]
    D = vkey1[None, :] - vkey2[(j[None, :] - sh) % S]  # circshift: shifted[(c + s) % S] = v[c]
    acc = np.zeros(S, f64)
    for c in range(S):
        acc = acc + D[:, c] * D[:, c]
    norms = np.sqrt(acc)
    best, arg = 10000000.0, 0
    for s in range(S):
        if norms[s] < best:
            best, arg = norms[s], s
    return arg


def shift_set(argmin, S, search_ratio):
    radius = int(math.floor(0.5 * search_ratio * S + 0.5))  # round() of a non-negative double
    out = [argmin]
    for ii in range(1, radius + 1):
        out.append((argmin + ii + S) % S)
        out.append((argmin - ii + S) % S)
    return sorted(out)


def dist_direct(sc1, n1, sc2, n2, shift):
    """distDirectSC (:79-101) of sc1 against circshift(sc2, shift)."""
    R, S = sc1.shape
    src = (np.arange(S) - shift) % S
    b = sc2[:, src]
    nb = n2[src]
    dot = np.zeros(S, f64)
    for r in range(R):
        dot = dot + sc1[r] * b[r]
    total, cols = 0.0, 0
    with np.errstate(all="ignore"):
        sim = dot / (n1 * nb)
    for c in range(S):
        if n1[c] == 0 or nb[c] == 0:
            continue
        total = total + float(sim[c])
        cols += 1
    if cols == 0:
        return float("nan")
    return 1.0 - total / cols


def distance_btn_scancontext(sc1, sc2, cfg=DEFAULTS):
    """distanceBtnScanContext (:126-157) -> (distance, shift)."""
    S = sc1.shape[1]
    a = fast_align(sector_key(sc1), sector_key(sc2))
    n1, n2 = column_norms(sc1), column_norms(sc2)
    best, arg = 10000000.0, 0
    for s in shift_set(a, S, float(cfg["search_ratio"])):
        d = dist_direct(sc1, n1, sc2, n2, s)
        if d < best:
            best, arg = d, s
    return best, arg


def knn(keys, query, k):
    """The k nearest rows of float32 ``keys`` to ``query`` in nanoflann's L2_Adaptor metric, exact,
    ordered by (distance, index)."""
    keys = np.asarray(keys, f32)
    d = query[None, :].astype(f32) - keys
    sq = d * d
    res = np.zeros(keys.shape[0], f32)
    R = keys.shape[1]
    g = 0
    while g + 3 < R:
        res = res + (((sq[:, g] + sq[:, g + 1]) + sq[:, g + 2]) + sq[:, g + 3])
        g += 4
    while g < R:
        res = res + sq[:, g]
        g += 1
    order = np.argsort(res, kind="stable")[:k]
    return order, res[order]


def tree_prefix(i, E, P):
    """Number of ring keys the tree in use holds when keyframe i (0-based) is the newest and one
    detect call was made per keyframe; 0 = not eligible yet."""
    if i < E:
        return 0
    return 1 + P * ((i - E) // P)


def yaw_of(nn_align, S):
    deg = f32(f64(nn_align) * (f64(360.0) / f64(S)))  # deg2rad takes a float
    return f32(f64(deg) * f64(math.pi) / f64(180.0))


class SCManager:
    """The reference's SCManager: makeAndSaveScancontextAndKeys + detectLoopClosureID, stateful."""

    def __init__(self, **cfg):
        self.cfg = dict(DEFAULTS)
        self.cfg.update(cfg)
        self.polarcontexts = []
        self.invkeys = []
        self.vkeys = []
        self.tree_keys = None  # polarcontext_invkeys_to_search_
        self.counter = 0       # tree_making_period_conter
        self.last = None       # details of the last detect call

    def make_and_save(self, cloud):
        self.save(make_scancontext(cloud, self.cfg))

    def save(self, sc):
        """The saving half of makeAndSaveScancontextAndKeys, for a descriptor made before."""
        self.polarcontexts.append(sc)
        self.invkeys.append(ring_key(sc))
        self.vkeys.append(sector_key(sc))

    def detect(self, search=True):
        """-> (loop_id, yaw float32); self.last holds min_dist, nn_idx, nn_align, the candidates.
        search=False only advances the state (eligibility, tree rebuild, counter) and returns None:
        a long sequence of which only some calls are compared."""
        c = self.cfg
        E, P, K = int(c["num_exclude_recent"]), int(c["tree_making_period"]), int(c["num_candidates"])
        S = int(c["num_sector"])
        self.last = dict(min_dist=10000000.0, nn_idx=0, nn_align=0, cands=[], prefix=0)
        if len(self.invkeys) < E + 1:
            return -1, f32(0.0)
        if self.counter % P == 0:
            self.tree_keys = np.stack(self.invkeys[:len(self.invkeys) - E]) if len(self.invkeys) > E else np.zeros((0, 1), f32)
        self.counter += 1
        if not search:
            self.last = None
            return None
        cur_key, cur_desc = self.invkeys[-1], self.polarcontexts[-1]
        idx, _ = knn(self.tree_keys, cur_key, K)
        min_dist, nn_align, nn_idx = 10000000.0, 0, 0
        cands = []
        for j in idx:
            d, a = distance_btn_scancontext(cur_desc, self.polarcontexts[int(j)], c)
            cands.append((int(j), d, a))
            if d < min_dist:
                min_dist, nn_align, nn_idx = d, a, int(j)
        loop_id = nn_idx if min_dist < float(c["dist_thres"]) else -1
        self.last = dict(min_dist=min_dist, nn_idx=nn_idx, nn_align=nn_align, cands=cands, prefix=self.tree_keys.shape[0])
        return loop_id, yaw_of(nn_align, S)
