#!/usr/bin/env python3
"""Times the ORB bag-of-words loop detector (lislam_bow_*) on the GPU, over a synthetic k = 10,
L = 6 vocabulary (1,000,000 words) of random descriptors:

  a  add_batch   the ORB descriptors (nfeatures 1,000) of 300 extracted 64x1024 scans, read where
                 lislam_batch_intensity_odometry left them on the device (k_bow_words + k_bow_vector)
  b  detect      300 keyframes against a 3,000-entry database of 1,000 random descriptors per entry
                 (k_bow_query + k_bow_select, with the copy of the results to the host)

Each step runs in a child process of its own under ``timeout``; a step warms up, then times
``--reps`` repetitions with HIP events recorded on the context's stream.  A second pass runs each step
under ``rocprofv3 --kernel-trace`` (fewer repetitions, the profiler slows the host) and reads the
per-kernel times from its trace.  Beside them stands the time of the numpy / Python restatement
(tests/restate_bow.py) on the host for the same work.  Prints one JSON line; ``--out`` also writes it.
``--no-host --work DIR`` first and ``--host-only --work DIR --out FILE`` afterwards time the host's
part apart from the GPU's.

    python scripts/bench_bow.py [--scans 300] [--db 3000] [--reps 20] [--out profiles/bow_bench.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "intensity_based_lidar_slam_for_me-_amd"
H, W = 64, 1024
K, L = 10, 6
NFEATURES = 1000
STEP_TIMEOUT_S = 420
KERNELS = ("k_bow_words", "k_bow_vector", "k_bow_query", "k_bow_select")


def vocabulary(seed: int = 1):
    """The full k-ary tree in breadth-first ids: parent[i] = (i - 1) // K."""
    n = (K ** (L + 1) - 1) // (K - 1)
    rng = np.random.default_rng(seed)
    parent = ((np.arange(n, dtype=np.int64) - 1) // K).astype(np.int32)
    parent[0] = -1
    return parent, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.uniform(0.5, 3.0, n)


def database_images(db: int, seed: int = 2):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (db, NFEATURES, 32), dtype=np.uint8)


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


def run_step(step: str, n: int, db: int, reps: int, warmup: int, dump: str) -> dict:
    scans = generate(n) if step == "a" else None
    import ctypes

    import torch

    pkg = importlib.import_module(PKG)
    nat = pkg.native
    ctx = pkg.Context(n_scans=H, width=W)
    raw = ctypes.c_void_p()
    nat.check(ctx.lib.lislam_get_stream(ctx.h, ctypes.byref(raw)), ctx.h, "lislam_get_stream")
    stream = torch.cuda.ExternalStream(raw.value) if raw.value else torch.cuda.default_stream()
    voc = vocabulary()

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

    extra = {}
    if step == "a":
        batch = pkg.Batch(ctx, n)
        batch.upload(scans)
        batch.extract(n)
        batch.intensity_odometry(n, NFEATURES)
        ctx.synchronize()
        bow = pkg.BowDatabase(ctx, *voc, capacity=n * (warmup + reps), max_features=NFEATURES)
        ms = timed(lambda: bow.add_batch(batch, 0, n))
        counts = [batch.count(nat.OUT_ORB_DESCRIPTORS, k) for k in range(n)]
        extra = {"descriptors": int(np.sum(counts)), "mean_words_per_entry": float(np.mean([bow.bow_vector(k)[0].shape[0]
                                                                                           for k in range(0, n, 10)]))}
        what = f"add_batch of the ORB descriptors of {n} extracted {H}x{W} scans"
        if dump:
            np.save(dump, np.concatenate([batch.download(nat.OUT_ORB_DESCRIPTORS, k) for k in range(n)]))
            np.save(dump + ".counts.npy", np.array(counts, np.int32))
        batch.close()
    else:
        images = database_images(db)
        bow = pkg.BowDatabase(ctx, *voc, capacity=db, max_features=NFEATURES)
        for i in range(0, db, 500):
            bow.add(list(images[i:i + 500]))
        first = db - n
        res = {}
        ms = timed(lambda: res.__setitem__("d", bow.detect(first, n)))
        d = res["d"]
        extra = {"results": int(sum(len(x) for x in d.ids)), "loops_found": int(np.count_nonzero(d.loop_id >= 0)),
                 "mean_words_per_entry": float(np.mean([bow.bow_vector(k)[0].shape[0] for k in range(0, db, 100)]))}
        what = f"detect of {n} keyframes against a {db}-entry database ({NFEATURES} descriptors per entry, results copied to the host)"
    bow.close()
    ctx.close()
    out = {"step": step, "what": what, "reps": reps, "ms_median": round(float(np.median(ms)), 4),
           "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}
    out.update(extra)
    return out


def kernel_times(trace_dir: str, calls: int, kernels) -> dict:
    """Per kernel: launches and total ms per call of the step, from a rocprofv3 kernel trace."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {"error": "no kernel trace written"}
    agg = {}
    for r in csv.DictReader(open(files[0])):
        name = r.get("Kernel_Name", "")
        for k in kernels:
            if k in name:
                a = agg.setdefault(k, [0.0, 0])
                a[0] += (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) * 1e-6
                a[1] += 1
    return {k: {"ms_per_call": round(v[0] / calls, 4), "launches_per_call": v[1] / calls} for k, v in agg.items()}


def host_restatement(n: int, db: int, desc_path: str) -> dict:
    """The same work through tests/restate_bow.py on the host, once."""
    import restate_bow as RB

    voc = RB.Vocabulary(*vocabulary())
    out = {}
    if os.path.exists(desc_path):
        rows, counts = np.load(desc_path), np.load(desc_path + ".counts.npy")
        offs = np.concatenate([[0], np.cumsum(counts)])
        t0 = time.perf_counter()
        for k in range(n):
            RB.bow_vector(voc, rows[offs[k]:offs[k + 1]])
        out["add_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    images = database_images(db)
    base = RB.Database(voc)
    vectors = [RB.bow_vector(voc, im) for im in images]
    for v in vectors[:db - n]:
        base.add_vector(v)
    cfg = RB.DEFAULTS
    t0 = time.perf_counter()
    for k in range(db - n, db):
        ret = base.query_vector(vectors[k], cfg["max_results"], k - cfg["min_loop_search_gap"])
        base.add_vector(vectors[k])
        RB.decide(ret, k, cfg)
    out["detect_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["what"] = ("tests/restate_bow.py on one core: add = transform + bow_vector of the same descriptors (numpy descent), "
                   "detect = the inverted-file query, add and decision per keyframe (Python)")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--db", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the restatement's time on the host")
    ap.add_argument("--host-only", action="store_true", help="add the restatement's time to the JSON that --out names (no GPU)")
    ap.add_argument("--work", default="", help="keep the intermediate files (step a's ORB descriptors) in this directory")
    ap.add_argument("--step", choices=["a", "b"], default=None, help="run one step in this process (the children's mode)")
    ap.add_argument("--dump", default="", help="step a: save the ORB descriptors here (for the host restatement)")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(run_step(args.step, args.scans, args.db, args.reps, args.warmup, args.dump)), flush=True)
        return 0
    tmp = args.work or tempfile.mkdtemp(prefix="bow_bench_")
    os.makedirs(tmp, exist_ok=True)
    desc_path = os.path.join(tmp, "orb_desc.npy")
    if args.host_only:
        out = json.load(open(args.out))
        out["host_restatement"] = host_restatement(args.scans, args.db, desc_path)
        text = json.dumps(out)
        print(text)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        return 0
    steps, failed = [], None
    prof_reps, prof_warm = 3, 1
    for step in ("a", "b"):
        base = [sys.executable, os.path.abspath(__file__), "--step", step, "--scans", str(args.scans), "--db", str(args.db)]
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), *base, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        if step == "a":
            cmd += ["--dump", desc_path]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            failed = f"step {step} ended with status {p.returncode}"
            break  # nothing more is started on the GPU after a failed step
        res = json.loads(line[-1][len("RESULT "):])
        trace = os.path.join(tmp, "trace_" + step)
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace,
               "-o", "bow", "--", *base, "--reps", str(prof_reps), "--warmup", str(prof_warm)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            failed = f"the profiled pass of step {step} ended with status {p.returncode}"
            steps.append(res)
            break
        res["kernels"] = kernel_times(trace, prof_reps + prof_warm, KERNELS[:2] if step == "a" else KERNELS[2:])
        steps.append(res)
    out = {"bench": "bow", "shape": [H, W], "vocabulary": {"k": K, "L": L, "words": K ** L}, "nfeatures": NFEATURES, "steps": steps}
    if failed:
        out["error"] = failed
    elif not args.no_host:
        out["host_restatement"] = host_restatement(args.scans, args.db, desc_path)
    if not args.work:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
