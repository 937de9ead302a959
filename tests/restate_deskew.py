"""ctypes wrapper of tests/cpp/deskew_restate.cpp (built by __graft_entry__.build() into
tests/cpp/build/libdeskew_restate.so): the CPU restatement of the scan-to-scan odometry with the
reference's DISTORTION switch, modes 0 / 1 / 2 = lislam_set_distortion's OFF / QUERIES / TO_END.
A missing library raises: the tests that need it fail, they do not skip."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "cpp", "build", "libdeskew_restate.so")
OFF, QUERIES, TO_END = 0, 1, 2
SCAN_PERIOD = 0.1

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built; run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        vp = ctypes.c_void_p
        L.deskew_odometry_chain.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 17
        L.deskew_odometry_chain.restype = ctypes.c_int
        _LIB = L
    return _LIB


@dataclass
class Chain:
    pose: np.ndarray   # (n, 7) q_w_curr, t_w_curr
    para: np.ndarray   # (n, 7) q_last_curr, t_last_curr
    stats: np.ndarray  # (n, 6) corners / planes of pass 0, pass 1, LM iterations of pass 0, 1
    corner_last: list  # mode 2: per frame, the less-sharp cloud at the scan's end (else the inputs)
    surf_last: list
    full_end: list


def _pack(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([c.shape[0] for c in clouds])
    data = np.zeros((max(int(off[-1]), 1), 4), np.float32)
    if off[-1]:
        data[: off[-1]] = np.concatenate([np.asarray(c, np.float32).reshape(-1, 4) for c in clouds])
    return data, off


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _split(data, off):
    return [data[off[k]: off[k + 1]].copy() for k in range(len(off) - 1)]


def odometry_chain(feats, mode: int, use_aloam=None) -> Chain:
    """A fresh laserOdometry node over `feats` (objects with sharp, less_sharp, flat, less_flat and
    laser_cloud arrays (n, 4)) in one distortion mode."""
    n = len(feats)
    s, so = _pack([f.sharp for f in feats])
    ls, lso = _pack([f.less_sharp for f in feats])
    fl, flo = _pack([f.flat for f in feats])
    lf, lfo = _pack([f.less_flat for f in feats])
    fu, fuo = _pack([f.laser_cloud for f in feats])
    pose = np.zeros((n, 7))
    rel = np.zeros((n, 7))
    st = np.zeros((n, 6), np.int32)
    u = None if use_aloam is None else np.ascontiguousarray(np.asarray(use_aloam).reshape(-1)[:n], np.int32)
    ocl, osl, ofe = ls.copy(), lf.copy(), fu.copy()
    rc = lib().deskew_odometry_chain(int(mode), n, _p(s), _p(so), _p(ls), _p(lso), _p(fl), _p(flo), _p(lf), _p(lfo),
                                     _p(fu), _p(fuo), _p(u), _p(pose), _p(rel), _p(st), _p(ocl), _p(osl), _p(ofe))
    if rc != 0:
        raise RuntimeError(f"deskew_odometry_chain failed ({rc})")
    return Chain(pose, rel, st, _split(ocl, lso), _split(osl, lfo), _split(ofe, fuo))


def batch_chains(feats, mode: int, chain_len: int, use_aloam=None) -> Chain:
    """What Batch.odometry(n, chain_len) computes: chain c is a fresh node over scans
    [c L, min(c L + L, n - 1)].  A boundary scan's para / pose / stats and to-end clouds are what the
    chain that solved it left; scan 0 keeps its first-frame (identity) version."""
    n = len(feats)
    out = None
    c0 = 0
    while c0 < n - 1 or out is None:
        c1 = min(c0 + chain_len, n - 1)
        ch = odometry_chain(feats[c0: c1 + 1], mode, None if use_aloam is None else list(use_aloam[c0: c1 + 1]))
        if out is None:
            out = Chain(np.zeros((n, 7)), np.zeros((n, 7)), np.zeros((n, 6), np.int32), [None] * n, [None] * n, [None] * n)
            lo = 0
        else:
            lo = 1
        for j in range(lo, c1 - c0 + 1):
            k = c0 + j
            out.pose[k], out.para[k], out.stats[k] = ch.pose[j], ch.para[j], ch.stats[j]
            out.corner_last[k], out.surf_last[k], out.full_end[k] = ch.corner_last[j], ch.surf_last[j], ch.full_end[j]
        if c1 >= n - 1:
            break
        c0 = c1
    return out


def rel_s(cloud: np.ndarray) -> np.ndarray:
    """s of every point as laserOdometry.cpp:153 computes it: float subtraction of int(intensity),
    then a double division by SCAN_PERIOD."""
    i = np.asarray(cloud, np.float32)[:, 3]
    return (i - np.trunc(i).astype(np.float32)).astype(np.float64) / SCAN_PERIOD
