#!/usr/bin/env python3
"""Times mapOptimization's ORB keyframe sliding window on the GPU, in one process: the window loop
alone (lislam_mapwin_records) and the whole mapOptimization step (lislam_mapopt_step_window) at
sliding_window_size W = 0, 5, 10, with the CPU restatement of the same work on one host core beside
them.

Workload: ``--frames`` synthetic 64 x 1024 scans (synth.make_sequence from scan 40), their ground +
less-flat clouds and less-sharp clouds downloaded from a batch, cv::ORB::create(2000, ...) features
of each scan with mapOptimization's zero filter (orb_detect(map_filter=True)), drifting odometry
(perturb_pose 0.02 m / 0.2 deg).  Inputs are host arrays, as MapOptimization.callback takes them: a
timed call includes their upload and ends in the step's own device synchronise (host clock).
  records  a window of W keyframes (scans 0..W-1 at their optimised poses), the current keyframe
           = scan W: wall ms per call, median of ``--reps``
  step     a fresh map per repetition, every frame through callback; wall ms of the frames whose
           window is full (index > W), median over frames and repetitions, the W's alternating
  kernels  one more pass per W with the library's timing scopes on: ms per step of every kernel
  cpu      tests/restate_mapwin.py over the same frames (numpy + the oracle's ikd-Tree and Ceres
           restatements, one core): a restatement written for checking, not an optimised port
Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_mapwin.py [--frames 14] [--reps 5] [--out profiles/mapwin_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
PKG = "intensity_based_lidar_slam_for_me-_amd"
H, W_IMG, NF, START = 64, 1024, 2000, 40
WINDOWS = (0, 5, 10)


def kernel_times(pkg, ctx, calls: int) -> dict:
    ms = (ctypes.c_float * 32)()
    la = (ctypes.c_int32 * 32)()
    ctx.lib.lislam_map_kernel_times(ctx.h, ms, la)
    names = pkg.native.MAP_KERNELS
    return {names[i]: {"ms_per_call": round(ms[i] / calls, 4), "launches_per_call": round(la[i] / calls, 2)}
            for i in range(len(names)) if la[i]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=14, help="frames of the CPU restatement (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    S = args.frames
    if S <= max(WINDOWS) + 1:
        ap.error("--frames must exceed the largest window by 2")

    pkg = importlib.import_module(PKG)
    nat = pkg.native
    synth = pkg.synth
    ctx = pkg.Context(n_scans=H, width=W_IMG)
    scans = synth.make_sequence(S, start=START)
    b = pkg.Batch(ctx, S)
    b.upload(scans)
    b.extract(S)
    b.ground(S)
    frames = []
    for k in range(S):
        f = b.features(k)
        ground = np.concatenate([b.ground_result(k)[0], f.less_flat]).astype(np.float32)
        img = b.download(nat.OUT_IMAGE_INTENSITY, k).reshape(H, W_IMG)
        _, de, p3 = pkg.intensity.orb_detect(ctx, img, b.download(nat.OUT_CLOUD_TRACK, k), NF, None, map_filter=True)
        q, t = synth.ground_truth_pose(START + k).as_qt()
        frames.append((ground, f.less_sharp, synth.perturb_pose(q, t, 0.02, 0.2, seed=60 + k), (de, p3)))
    b.close()

    def drive(Wn, timed=None):
        mo = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, corner=True, sliding_window_size=Wn)
        out = []
        for k, (g, c, od, f) in enumerate(frames):
            ctx.synchronize()
            t0 = time.perf_counter()
            pose, summ = mo.callback(g, od, c, features=f)
            dt = (time.perf_counter() - t0) * 1e3
            if timed is not None and k > Wn:
                timed.append(dt)
            out.append((pose, summ))
        mo.close()
        return out

    rows = {}
    ref = {Wn: drive(Wn) for Wn in WINDOWS}  # warm-up of every shape, and the poses of each W
    times = {Wn: [] for Wn in WINDOWS}
    for _ in range(args.reps):  # the windows alternate
        for Wn in WINDOWS:
            drive(Wn, times[Wn])
    for Wn in WINDOWS:
        ctx.lib.lislam_map_set_timing(ctx.h, 1)
        ctx.lib.lislam_map_kernel_times(ctx.h, (ctypes.c_float * 32)(), None)
        drive(Wn)
        ctx.synchronize()
        kern = kernel_times(pkg, ctx, S)
        ctx.lib.lislam_map_set_timing(ctx.h, 0)
        t = np.array(times[Wn])
        full = [s for k, (_, s) in enumerate(ref[Wn]) if k > Wn]
        rows[str(Wn)] = {"step_ms": round(float(np.median(t)), 4), "step_ms_min": round(float(t.min()), 4),
                         "step_ms_max": round(float(t.max()), 4), "timed_steps": len(t),
                         "feature_blocks_per_step": round(float(np.mean([s[3] if len(s) > 3 else 0 for s in full])), 1),
                         "keyframes_used_per_step": round(float(np.mean([s[4] if len(s) > 4 else 0 for s in full])), 2),
                         "plane_blocks_per_step": round(float(np.mean([s[0] for s in full])), 1),
                         "kernels_ms_per_step_all_frames": kern}

    # the window loop alone
    rec_rows = {}
    for Wn in WINDOWS[1:]:
        win = pkg.mapping.SlidingWindow(ctx, Wn, 4096)
        for k in range(Wn):
            win.push(frames[k][3][0], frames[k][3][1], ref[Wn][k][0])
        cur = (frames[Wn][3][0], frames[Wn][3][1], ref[Wn][Wn][0])
        for _ in range(2):
            rec, info, pairs = win.records(*cur)
        t = []
        for _ in range(max(args.reps, 5) * 4):
            ctx.synchronize()
            t0 = time.perf_counter()
            win.records(*cur)
            t.append((time.perf_counter() - t0) * 1e3)
        ctx.lib.lislam_map_set_timing(ctx.h, 1)
        ctx.lib.lislam_map_kernel_times(ctx.h, (ctypes.c_float * 32)(), None)
        for _ in range(10):
            win.records(*cur)
        kern = kernel_times(pkg, ctx, 10)
        ctx.lib.lislam_map_set_timing(ctx.h, 0)
        rec_rows[str(Wn)] = {"records_ms": round(float(np.median(t)), 4), "records_ms_min": round(min(t), 4),
                             "records_ms_max": round(max(t), 4), "calls": len(t), "queries": int(len(cur[0])),
                             "trains": [int(v) for v in info[:, 0]], "records": int(len(rec)),
                             "keyframes_used": int(info[:, 3].sum()), "kernels_ms_per_call": kern}
        win.close()

    cpu = None
    if args.cpu_frames > 0:
        import oracle as O
        import restate_mapwin as R

        O.lib()
        n = min(args.cpu_frames, S)
        cpu = {"cores": 1, "kind": "restatement (numpy + the oracle's C++ ikd-Tree and Ceres restatements), not an optimised port"}
        for Wn in WINDOWS:
            ro = R.MapOptimization(O, Wn)
            ts, agree = [], 0.0
            for k, (g, c, od, f) in enumerate(frames[:n]):
                t0 = time.perf_counter()
                p, s = ro.callback(g, od, c, f)
                dt = (time.perf_counter() - t0) * 1e3
                if k > Wn:
                    ts.append(dt)
                agree = max(agree, float(np.max(np.abs(p - ref[Wn][k][0]))))
            cpu[str(Wn)] = {"step_ms": round(float(np.median(ts)), 3) if ts else None, "timed_steps": len(ts),
                            "max_pose_difference_to_gpu": agree}
        for Wn in WINDOWS[1:]:
            kfs = [R.Keyframe(frames[k][3][0], frames[k][3][1], ref[Wn][k][0]) for k in range(Wn)]
            cur = (frames[Wn][3][0], frames[Wn][3][1], ref[Wn][Wn][0])
            t0 = time.perf_counter()
            R.window_records(kfs, *cur)
            cpu[str(Wn)]["records_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

    text = json.dumps({"bench": "mapwin", "shape": [H, W_IMG], "nfeatures": NF, "frames": S, "reps": args.reps,
                       "what": "mapOptimization step with the ORB keyframe sliding window (lislam_mapopt_step_window, host inputs, "
                               "wall ms per step with a full window, median) and the window loop alone (lislam_mapwin_records, "
                               "wall ms per call incl. feature upload and result download); W = sliding_window_size",
                       "step": rows, "records": rec_rows, "cpu_restatement": cpu})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
