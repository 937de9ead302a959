#!/usr/bin/env python3
"""Times keyframe selection and the back end's list feeds on the GPU, on one 300-scan 64x1024 batch of
the synthetic drive (extracted, odometry and ORB front end run) at the reference's thresholds
(0.3 s, 0.3 m; config/spot.yaml:35-36), scans 0.1 s apart:

  select    KeyframeSelector.step_batch over the whole batch, alone (k_keysel and the copies back)
  feeds     each add_batch_scans over the selected scans against the same scans fed by single-scan range
            calls add_batch(b, s, 1), the only way to feed a list before the list forms existed: the
            keyframe pool, Scan Context, the bag of words, the pose graph
  backend   one LoopBackend.step over the batch against the every-scan-is-a-keyframe feed of the same
            objects (add_batch over all 300 scans, detect, close_loops, optimize)

Every timing is a host clock around work that ends in a device synchronise, on fresh objects made
outside the window; the two sides of a comparison alternate inside one process.  Prints one JSON line and
writes it to ``--out``.

    python scripts/bench_backend.py [--scans 300] [--reps 10] [--out profiles/backend_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "intensity_based_lidar_slam_for_me-_amd"
H, W = 64, 1024
NFEATURES = 1000
K, L = 10, 4  # the bag-of-words vocabulary: random descriptors, 10,000 words
INTERVALS = (0.3, 0.3)


def vocabulary(seed: int = 1):
    n = (K ** (L + 1) - 1) // (K - 1)
    rng = np.random.default_rng(seed)
    parent = ((np.arange(n, dtype=np.int64) - 1) // K).astype(np.int32)
    parent[0] = -1
    return parent, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.uniform(0.5, 3.0, n)


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


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4),
            "ms_max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--backend-reps", type=int, default=3, help="repetitions of the backend comparison (one warm-up)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backend_bench.json"))
    args = ap.parse_args()
    n = args.scans
    scans = generate(n)
    pkg = importlib.import_module(PKG)
    ctx = pkg.Context(n_scans=H, width=W)
    b = pkg.Batch(ctx, n)
    b.upload(scans)
    b.extract(n)
    b.odometry(n, n - 1)
    b.intensity_odometry(n, NFEATURES)
    ctx.synchronize()
    times = 100.0 + 0.1 * np.arange(n) + np.random.default_rng(5).uniform(-0.004, 0.004, n)
    voc = vocabulary()
    N = H * W

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def compare(make, a, c, warmup=args.warmup, reps=args.reps):
        """Wall times of a(obj) and c(obj) on fresh objects, alternating."""
        ta, tc = [], []
        for k in range(warmup + reps):
            for fn, acc in ((a, ta), (c, tc)):
                obj = make()
                ctx.synchronize()
                ms, _ = timed(lambda: fn(obj))
                if k >= warmup:
                    acc.append(ms)
                for o in obj if isinstance(obj, tuple) else (obj,):
                    o.close()
        return ta, tc

    # select
    ms, ids = [], None
    for k in range(args.warmup + args.reps):
        sel = pkg.KeyframeSelector(ctx, *INTERVALS)
        t, (ids, _, _) = timed(lambda: sel.step_batch(b, 0, n, times))
        sel.close()
        if k >= args.warmup:
            ms.append(t)
    sel_scans = np.flatnonzero(ids >= 0).astype(np.int32)
    m = int(sel_scans.shape[0])
    out = {"bench": "backend", "shape": [H, W], "scans": n, "intervals": list(INTERVALS), "keyframes": m,
           "good_frames": int(sum(int(b.download(pkg.native.OUT_ORB_STATS, k)[0]) == 1 for k in range(n))),
           "select": dict(stats(ms), what=f"KeyframeSelector.step_batch over {n} scans, results on the host")}

    def loop_of(name):
        def run(obj):
            f = getattr(obj, name)
            for s in sel_scans:
                f(b, int(s), 1)
        return run

    feeds = {}
    makers = {
        "keyframes": lambda: pkg.KeyframePool(ctx, m, m * N),
        "place": lambda: pkg.ScanContext(ctx, capacity=m),
        "bow": lambda: pkg.BowDatabase(ctx, *voc, capacity=m, max_features=NFEATURES),
        "pgo": lambda: pkg.PoseGraph(ctx, node_capacity=m, edge_capacity=m),
    }
    for name, make in makers.items():
        tl, ts = compare(make, lambda o: o.add_batch_scans(b, sel_scans), loop_of("add_batch"))
        feeds[name] = {"list": stats(tl), "single_scan_calls": stats(ts),
                       "speedup": round(float(np.median(ts) / np.median(tl)), 3)}
    out["feeds"] = dict(feeds, what=f"add_batch_scans of the {m} selected scans vs {m} calls add_batch(b, s, 1)")

    # backend: selected keyframes vs every scan a keyframe
    def objects():
        return (pkg.KeyframeSelector(ctx, *INTERVALS), pkg.KeyframePool(ctx, n, n * N),
                pkg.BowDatabase(ctx, *voc, capacity=n, max_features=NFEATURES),
                pkg.PoseGraph(ctx, node_capacity=n, edge_capacity=4 * n))

    found = {}

    def backend(o):
        s = pkg.LoopBackend(ctx, *o).step(b, 0, n, times)
        found["backend"] = (int(np.count_nonzero(s.detection.loop_id >= 0)), int(np.count_nonzero(s.info[:, 0] == 1)))

    def every_scan(o):
        _, pool, db, g = o
        pool.add_batch(b, 0, n)
        db.add_batch(b, 0, n)
        g.add_batch(b, 0, n)
        g.set_prior(0, g.poses(0, 1)[0])
        det = db.detect(0, n)
        v = pkg.close_loops(pool, g, np.arange(n, dtype=np.int32), det.loop_id)
        if np.any(v[3][:, 0] == 1):
            g.optimize()
        found["every_scan"] = (int(np.count_nonzero(det.loop_id >= 0)), int(np.count_nonzero(v[3][:, 0] == 1)))

    tb, te = compare(objects, backend, every_scan, 1, args.backend_reps)
    out["backend"] = {"selected": dict(stats(tb), keyframes=m, candidates=found["backend"][0], accepted=found["backend"][1]),
                      "every_scan": dict(stats(te), keyframes=n, candidates=found["every_scan"][0],
                                         accepted=found["every_scan"][1]),
                      "speedup": round(float(np.median(te) / np.median(tb)), 3),
                      "what": "LoopBackend.step (bag-of-words detector, default thresholds) vs add_batch of every scan, "
                              "detect, close_loops, optimize"}
    b.close()
    ctx.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
