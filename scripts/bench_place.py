#!/usr/bin/env python3
"""Times the Scan Context place database (lislam_place_*) on the GPU:

  a  add_batch   300 extracted 64x1024 scans described from the batch's device cloud_track
                 (k_sc_describe + k_sc_finish)
  b  detect      300 queries against a 3,000-entry database in one k_sc_detect launch (with the
                 copy of its five result arrays to the host)
  c  add_clouds  the same 300 clouds from host memory (upload + describe + finish)

Each step runs in a child process of its own under ``timeout``; a step warms up, then times
``--reps`` repetitions with HIP events recorded on the context's stream.  Beside each time stand
the algorithmic bytes (what the step must read and write once) and their share of the HBM peak, as
bench.py's roofline does it.  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_place.py [--scans 300] [--db 3000] [--reps 20] [--out profiles/place_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "intensity_based_lidar_slam_for_me-_amd"
HBM_PEAK_GBS = 8000.0  # HBM3E peak, the figure bench.py's roofline uses
H, W = 64, 1024
R, S = 20, 60
STEP_TIMEOUT_S = 240


def _gen(job):
    start, n = job
    return importlib.import_module(PKG + ".synth").make_sequence(n, H, W, start=start)


def generate(n: int, workers: int = 8) -> np.ndarray:
    """The seeded synthetic stream [0, n), made by a spawn pool before any GPU use."""
    import multiprocessing as mp

    chunk = (n + workers - 1) // workers
    jobs = [(i, min(chunk, n - i)) for i in range(0, n, chunk)]
    with mp.get_context("spawn").Pool(len(jobs)) as pool:
        return np.concatenate(pool.map(_gen, jobs))


def entry_bytes() -> int:
    """What k_sc_finish reads and writes per entry: the integer grid, the double grid, both keys
    and the column norms."""
    return R * S * 4 + R * S * 8 + R * 4 + S * 8 + S * 8


def run_step(step: str, n: int, db: int, reps: int, warmup: int) -> dict:
    scans = generate(n)
    import torch

    pkg = importlib.import_module(PKG)
    nat = pkg.native
    ctx = pkg.Context(n_scans=H, width=W)
    raw = ctypes.c_void_p()
    nat.check(ctx.lib.lislam_get_stream(ctx.h, ctypes.byref(raw)), ctx.h, "lislam_get_stream")
    stream = torch.cuda.ExternalStream(raw.value) if raw.value else torch.cuda.default_stream()
    batch = pkg.Batch(ctx, n)
    batch.upload(scans)
    batch.extract(n)
    ctx.synchronize()
    N = H * W

    def timed(fn, before=None):
        ms = []
        for k in range(warmup + reps):
            if before:
                before()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    state = {}

    def fresh():
        if state.get("sc"):
            state["sc"].close()
        state["sc"] = pkg.ScanContext(ctx, capacity=n)

    if step == "a":
        ms = timed(lambda: state["sc"].add_batch(batch, 0, n), fresh)
        nbytes = n * N * 16 + n * entry_bytes()
        what = f"add_batch of {n} extracted {H}x{W} scans"
    elif step == "c":
        tracks = np.ascontiguousarray(np.stack([batch.download(nat.OUT_CLOUD_TRACK, k) for k in range(n)]))
        counts = np.full(n, N, np.int32)

        def add_clouds():
            nat.check(ctx.lib.lislam_place_add_clouds(state["sc"].h, nat.ptr(tracks), nat.ptr(counts), n), ctx.h,
                      "lislam_place_add_clouds")

        ms = timed(add_clouds, fresh)
        nbytes = 2 * n * N * 16 + n * entry_bytes()  # the staging copy lands in HBM and is read back once
        what = f"add_clouds of the same {n} clouds from host memory (upload included)"
    else:
        sc = pkg.ScanContext(ctx, capacity=db)
        for _ in range(db // n):
            sc.add_batch(batch, 0, n)
        if db % n:
            sc.add_batch(batch, 0, db % n)
        first = db - n
        res = {}
        ms = timed(lambda: res.__setitem__("d", sc.detect(first, n)))
        d = res["d"]
        cfg = pkg.native.PlaceConfig()
        E, P, K = cfg.num_exclude_recent, cfg.tree_making_period, cfg.num_candidates
        prefixes = [1 + P * ((i - E) // P) for i in range(first, db)]
        shifts = 2 * int(round(0.5 * cfg.search_ratio * S)) + 1
        # ring keys of each query's prefix once, and both descriptors, sector keys and column norms of
        # every (query, candidate) pair once; the per-shift re-reads are served on chip
        nbytes = sum(p * R * 4 for p in prefixes) + n * K * 2 * (R * S * 8 + 2 * S * 8)
        what = f"detect of {n} queries against a {db}-entry database ({K} candidates x {shifts} shifts)"
        state["extra"] = {"loops_found": int(np.count_nonzero(d.loop_id >= 0)), "mean_prefix": float(np.mean(prefixes))}
        sc.close()
    if state.get("sc"):
        state["sc"].close()
    batch.close()
    ctx.close()
    med = float(np.median(ms))
    gbs = nbytes / (med * 1e-3) / 1e9
    out = {"step": step, "what": what, "reps": reps, "ms_median": round(med, 4), "ms_min": round(float(np.min(ms)), 4),
           "ms_max": round(float(np.max(ms)), 4), "algorithmic_bytes": int(nbytes), "achieved_GBs": round(gbs, 2),
           "hbm_peak_GBs": HBM_PEAK_GBS, "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 5)}
    out.update(state.get("extra", {}))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--db", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["a", "b", "c"], default=None, help="run one step in this process (the children's mode)")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(run_step(args.step, args.scans, args.db, args.reps, args.warmup)), flush=True)
        return 0
    steps = []
    for step in ("a", "b", "c"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step,
               "--scans", str(args.scans), "--db", str(args.db), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(json.dumps({"error": f"step {step} ended with status {p.returncode}", "steps": steps}))
            return 1  # nothing more is started on the GPU after a failed step
        steps.append(json.loads(line[-1][len("RESULT "):]))
    text = json.dumps({"bench": "place", "shape": [H, W], "ring_sector": [R, S], "steps": steps})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
