#!/usr/bin/env python3
"""Times the batched loop verification (lislam_loop_verify from a device keyframe pool) against
the same candidates verified one by one through lislam_loop_icp with device-resident inputs, in
one process on the GPU.

Workload: bench.py --workload icp -- eight loop closures of a 64x1024 keyframe against its
3-keyframe submap, the same drifts.  The pool holds the four keyframes of every case; a sweep of L
candidates cycles through the eight cases.  For every L the two paths alternate ``--reps`` times
(host clock around calls that end in a device synchronise, kernel timing off); then one more pass
of each with the library's timing scopes on gives the per-kernel times.  The rows of the two paths
are compared for equality.  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_loop_verify.py [--sweep 1,8,32,64] [--reps 7] [--out profiles/loop_verify_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "intensity_based_lidar_slam_for_me-_amd"
H, W = 64, 1024
NCASE = 8


def loop_case(synth, k: int):
    """bench.py's _loop_case: keyframe k under a drifted pose, keyframes k-3..k-1 under the ground truth."""
    def pose_T(p):
        c, s = math.cos(p.yaw), math.sin(p.yaw)
        T = np.eye(4)
        T[:2, :2] = [[c, -s], [s, c]]
        T[0, 3], T[1, 3] = p.x, p.y
        return T
    yaw = math.radians(2.0 + 0.5 * (k % 5))
    D = np.eye(4)
    D[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    D[:3, 3] = (0.3, -0.2, 0.05)
    ids = (k - 3, k - 2, k - 1, k)
    clouds = [synth.make_scan(j, H, W).reshape(-1, 4) for j in ids]
    T = [pose_T(synth.ground_truth_pose(j)) for j in ids]
    T[3] = D @ T[3]
    return clouds, T


def kernel_times(pkg, ctx, calls: int) -> dict:
    ms = (ctypes.c_float * 32)()
    la = (ctypes.c_int32 * 32)()
    ctx.lib.lislam_map_kernel_times(ctx.h, ms, la)
    names = pkg.native.MAP_KERNELS
    return {names[i]: {"ms_per_call": round(ms[i] / calls, 4), "launches_per_call": round(la[i] / calls, 2)}
            for i in range(len(names)) if la[i]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweep", default="1,8,32,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sweep = [int(v) for v in args.sweep.split(",")]

    import torch

    pkg = importlib.import_module(PKG)
    nat = pkg.native
    cases = [loop_case(pkg.synth, 40 + 7 * i) for i in range(NCASE)]
    ctx = pkg.Context(n_scans=H, width=W)
    lib = ctx.lib
    cfg = pkg.loop.IcpConfig()
    # the pool: case i = keyframes 4i .. 4i + 3, candidate (4i + 3, 4i + 1) with the window 1
    pool = pkg.KeyframePool(ctx, capacity=4 * NCASE, point_capacity=4 * NCASE * H * W)
    pool.add_clouds([c for clouds, _ in cases for c in clouds])
    T_kf = np.ascontiguousarray(np.stack([t for _, T in cases for t in T]).reshape(-1, 16))
    # the sequential path's inputs, resident in HBM as bench.py stages them
    staged = []
    for clouds, T in cases:
        dc = torch.from_numpy(clouds[3]).cuda()
        dh = torch.from_numpy(np.concatenate(clouds[:3])).cuda()
        staged.append((dc, np.ascontiguousarray(T[3].reshape(16)), dh, np.full(3, H * W, np.int32),
                       np.ascontiguousarray(np.stack(T[:3]).reshape(-1, 16))))
    torch.cuda.synchronize()

    def batch(L):
        cur = np.array([4 * (k % NCASE) + 3 for k in range(L)], np.int32)
        out = (np.zeros((L, 16)), np.zeros((L, 16)), np.zeros(L), np.zeros((L, 8), np.int32))
        nat.check(lib.lislam_loop_verify(pool.h, ctypes.byref(cfg), 1, nat.ptr(cur), nat.ptr(cur - 2), L, nat.ptr(T_kf),
                                         *(nat.ptr(o) for o in out)), ctx.h, "lislam_loop_verify")
        return out

    def sequential(L):
        out = (np.zeros((L, 16)), np.zeros((L, 16)), np.zeros(L), np.zeros((L, 8), np.int32))
        for k in range(L):
            dc, Tc, dh, counts, Th = staged[k % NCASE]
            nat.check(lib.lislam_loop_icp(ctx.h, ctypes.byref(cfg), ctypes.c_void_p(dc.data_ptr()), dc.shape[0], nat.ptr(Tc),
                                          ctypes.c_void_p(dh.data_ptr()), nat.ptr(counts), 3, nat.ptr(Th), nat.ptr(out[0][k]),
                                          nat.ptr(out[1][k]), nat.ptr(out[2][k:]), nat.ptr(out[3][k])), ctx.h, "lislam_loop_icp")
        return out

    def wall(fn, L):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn(L)  # both paths return after their last device synchronise
        return (time.perf_counter() - t0) * 1e3

    rows = []
    for L in sweep:
        for _ in range(args.warmup):
            b, s = batch(L), sequential(L)
        same = all(np.array_equal(x, y) for x, y in zip(b, s))
        tb, ts = [], []
        for _ in range(args.reps):  # alternating
            tb.append(wall(batch, L))
            ts.append(wall(sequential, L))
        kern = {}
        for name, fn in (("batch", batch), ("sequential", sequential)):
            lib.lislam_map_set_timing(ctx.h, 1)
            lib.lislam_map_kernel_times(ctx.h, (ctypes.c_float * 32)(), None)
            fn(L)
            ctx.synchronize()
            kern[name] = kernel_times(pkg, ctx, 1)
            lib.lislam_map_set_timing(ctx.h, 0)
        mb, ms = float(np.median(tb)), float(np.median(ts))
        rows.append({"L": L, "rows_equal": bool(same), "iterations": [int(v) for v in b[3][:NCASE, 3]],
                     "batch_ms": round(mb, 4), "batch_ms_min": round(min(tb), 4), "batch_ms_max": round(max(tb), 4),
                     "sequential_ms": round(ms, 4), "sequential_ms_min": round(min(ts), 4),
                     "sequential_ms_max": round(max(ts), 4), "batch_ms_per_candidate": round(mb / L, 4),
                     "sequential_ms_per_candidate": round(ms / L, 4), "sequential_over_batch": round(ms / mb, 3),
                     "kernels_per_call": kern})
    text = json.dumps({"bench": "loop_verify", "shape": [H, W], "cases": NCASE, "submap_keyframes": 3, "reps": args.reps,
                       "what": "lislam_loop_verify of L candidates from a device pool vs. the same candidates one by one through "
                               "lislam_loop_icp with device-resident inputs; wall ms per call, median of alternating repetitions",
                       "staged_bytes_per_candidate": {"sequential": 4 * H * W * 16, "batch": 0},
                       "sweep": rows})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    pool.close()
    ctx.close()
    return 0 if all(r["rows_equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
