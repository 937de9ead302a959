#!/usr/bin/env python3
"""Times the vocabulary training (lislam_bow_train) on the GPU over the ORB descriptors (nfeatures
1,000) of 300 extracted synthetic 64x1024 scans, fed through ``BowTrainer.add_batch`` where
lislam_batch_intensity_odometry left them on the device, at k = 10 and L in {3, 5}:

  train     ms per training (host wall clock around ``BowTrainer.train``, median of ``--reps``; beside it
            the lislam_bow_train call alone, without the copy of the arrays to numpy), ms per level, the
            iterations per level, and from one more run with ``profile`` (a device wait after every
            phase) the ms per level and phase (seed, assign, means, partition) and of the weighting
  subset    the same on the first ``--host-scans`` scans alone
  host      the restatement (tests/restate_bow_train.py, the literal recursion, one core) on the subset
            and on all 300 scans (about a minute; ``--host-subset-only`` skips the full set), with its
            node and iteration counts, which must be the GPU's
  database  ``BowDatabase`` over the trained tree: add_batch of the 300 scans and detect of the last
            300 of 3,000 entries (the 300 scans added ten times), HIP events on the context's stream;
            beside them the figures of the random tree from profiles/bow_bench.json (there the 3,000
            entries hold random descriptors)

A second child runs three trainings at L = 5 under ``rocprofv3 --kernel-trace`` for the per-kernel
times.  Each child runs under ``timeout``; nothing is started after one that failed.  ``--no-host --work DIR`` first and
``--host-only --work DIR --out FILE`` afterwards time the host's part apart from the GPU's.

    python scripts/bench_bow_train.py [--scans 300] [--reps 5] [--out profiles/bow_train_bench.json]
"""
from __future__ import annotations

import argparse
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "intensity_based_lidar_slam_for_me-_amd"
H, W = 64, 1024
K, LEVELS = 10, (3, 5)
NFEATURES = 1000
DB_REPEATS = 10
STEP_TIMEOUT_S = 540
KERNELS = ("k_bowt_seed", "k_bowt_assign", "k_bowt_means", "k_bowt_majority", "k_bowt_tilecount", "k_bowt_offsets",
           "k_bowt_scatter", "k_bowt_locate", "k_bowt_ni", "k_bowt_ingest", "k_bow_words")


def _stats(tr) -> dict:
    s = tr.stats
    return {"nodes": s.n_nodes, "words": s.n_words, "zero_weight_words": s.n_zero_words, "level_steps": s.level_steps,
            "level_clustered": s.level_clustered, "level_iterations": s.level_iterations, "level_capped": s.level_capped,
            "level_ms": [round(x, 3) for x in s.level_ms], "weights_ms": round(s.weights_ms, 3),
            "phase_ms": [{k: round(v, 3) for k, v in p.items()} for p in s.phase_ms]}


def _train(tr, L: int, reps: int) -> dict:
    tr.train(K, L)  # warm-up: the trainer's buffers grow here
    wall, levels, call = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        tr.train(K, L)
        wall.append((time.perf_counter() - t0) * 1e3)
        levels.append(tr.stats.level_ms)
        call.append(tr.stats.total_ms)
    out = {"k": K, "L": L, "reps": reps, "ms_median": round(float(np.median(wall)), 3), "ms_min": round(float(np.min(wall)), 3),
           "ms_max": round(float(np.max(wall)), 3), "ms_all": [round(x, 3) for x in wall],
           "abi_call_ms_median": round(float(np.median(call)), 3), "level_ms_median": [round(float(x), 3) for x in np.median(levels, axis=0)]}
    tr.train(K, L, profile=True)
    out["profiled"] = _stats(tr)
    return out


def run_gpu(n: int, host_scans: int, reps: int, dump: str) -> dict:
    import bench_bow

    scans = bench_bow.generate(n)
    import ctypes

    import torch

    pkg = importlib.import_module(PKG)
    nat = pkg.native
    ctx = pkg.Context(n_scans=H, width=W)
    raw = ctypes.c_void_p()
    nat.check(ctx.lib.lislam_get_stream(ctx.h, ctypes.byref(raw)), ctx.h, "lislam_get_stream")
    stream = torch.cuda.ExternalStream(raw.value) if raw.value else torch.cuda.default_stream()

    def timed(fn, before=None):
        ms = []
        for k in range(1 + reps):
            if before:
                before()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if k >= 1:
                ms.append(e0.elapsed_time(e1))
        return round(float(np.median(ms)), 4)

    batch = pkg.Batch(ctx, n)
    batch.upload(scans)
    batch.extract(n)
    batch.intensity_odometry(n, NFEATURES)
    ctx.synchronize()
    counts = [batch.count(nat.OUT_ORB_DESCRIPTORS, k) for k in range(n)]
    total = int(np.sum(counts))
    if dump:
        np.save(dump, np.concatenate([batch.download(nat.OUT_ORB_DESCRIPTORS, k) for k in range(n)]))
        np.save(dump + ".counts.npy", np.array(counts, np.int32))
    full, sub = pkg.BowTrainer(ctx, n, n * NFEATURES), pkg.BowTrainer(ctx, host_scans, host_scans * NFEATURES)
    t0 = time.perf_counter()
    full.add_batch(batch, 0, n)
    add_ms = (time.perf_counter() - t0) * 1e3
    sub.add_batch(batch, 0, host_scans)
    out = {"scans": n, "descriptors": total, "trainer_add_batch_ms": round(add_ms, 3), "train": [], "database": [],
           "subset": {"scans": host_scans, "descriptors": int(np.sum(counts[:host_scans])), "train": []}}
    for L in LEVELS:
        out["train"].append(_train(full, L, reps))
        # the database over this tree (the last training above was the profiled one: the same tree)
        db = full.database(n * (reps + 1), max_features=NFEATURES)
        res = {"L": L, "words": full.stats.n_words}
        res["add_batch_ms"] = timed(lambda: db.add_batch(batch, 0, n))
        db.close()
        db = full.database(n * DB_REPEATS, max_features=NFEATURES)
        for _ in range(DB_REPEATS):
            db.add_batch(batch, 0, n)
        found = {}
        res["detect_ms"] = timed(lambda: found.__setitem__("d", db.detect(n * (DB_REPEATS - 1), n)))
        res["loops_found"] = int(np.count_nonzero(found["d"].loop_id >= 0))
        res["mean_words_per_entry"] = float(np.mean([db.bow_vector(k)[0].shape[0] for k in range(0, n, 10)]))
        db.close()
        out["database"].append(res)
        out["subset"]["train"].append(_train(sub, L, reps))
    for o in (full, sub, batch, ctx):
        o.close()
    return out


def run_trace(n: int, L: int, reps: int) -> dict:
    """The child under rocprofv3: ``reps`` identical trainings at (K, L) and nothing else after the
    descriptors are in the trainer, so the trace's k_bowt_* (and k_bow_words) rows are theirs."""
    import bench_bow

    scans = bench_bow.generate(n)
    pkg = importlib.import_module(PKG)
    ctx = pkg.Context(n_scans=H, width=W)
    batch = pkg.Batch(ctx, n)
    batch.upload(scans)
    batch.extract(n)
    batch.intensity_odometry(n, NFEATURES)
    tr = pkg.BowTrainer(ctx, n, n * NFEATURES)
    tr.add_batch(batch, 0, n)
    for _ in range(reps):
        tr.train(K, L)
    for o in (tr, batch, ctx):
        o.close()
    return {"L": L, "trainings": reps}


def host_restatement(desc_path: str, host_scans: int, full: bool) -> dict:
    """tests/restate_bow_train.py (the literal recursion, numpy distances, one core) on the first
    ``host_scans`` scans' descriptors and, with ``full``, on all of them."""
    import restate_bow_train as RT

    rows, counts = np.load(desc_path), np.load(desc_path + ".counts.npy").tolist()
    out = {"what": "tests/restate_bow_train.py train_recursive on one core over the same descriptors", "runs": []}
    for scans in [host_scans] + ([len(counts)] if full and len(counts) > host_scans else []):
        sub = rows[:sum(counts[:scans])]
        run = {"scans": scans, "descriptors": int(sub.shape[0]), "train": []}
        for L in LEVELS:
            t0 = time.perf_counter()
            r = RT.train_recursive(sub, counts[:scans], K, L)
            run["train"].append({"k": K, "L": L, "ms": round((time.perf_counter() - t0) * 1e3, 1), "nodes": int(r.parent.shape[0]),
                                 "level_iterations": r.stats["level_iterations"]})
        out["runs"].append(run)
    return out


def random_tree_figures() -> dict:
    path = os.path.join(ROOT, "profiles", "bow_bench.json")
    if not os.path.exists(path):
        return {}
    ref = json.load(open(path))
    return {"source": "profiles/bow_bench.json", "vocabulary": ref.get("vocabulary"),
            "steps": [{"what": s["what"], "ms_median": s["ms_median"]} for s in ref.get("steps", [])]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--host-scans", type=int, default=30, help="the restatement (and the GPU's subset run) use the first so many scans")
    ap.add_argument("--host-subset-only", action="store_true", help="the restatement skips the full set (about a minute)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the restatement's time on the host")
    ap.add_argument("--host-only", action="store_true", help="add the restatement's time to the JSON that --out names (no GPU)")
    ap.add_argument("--work", default="", help="keep the intermediate files (the ORB descriptors) in this directory")
    ap.add_argument("--gpu", action="store_true", help="run the GPU part in this process (the child's mode)")
    ap.add_argument("--dump", default="")
    ap.add_argument("--trace-L", type=int, default=0, help="run only trainings at this L in this process (the traced child's mode)")
    args = ap.parse_args()
    if args.trace_L:
        print("RESULT " + json.dumps(run_trace(args.scans, args.trace_L, args.reps)), flush=True)
        return 0
    if args.gpu:
        print("RESULT " + json.dumps(run_gpu(args.scans, args.host_scans, args.reps, args.dump)), flush=True)
        return 0
    tmp = args.work or tempfile.mkdtemp(prefix="bow_train_bench_")
    os.makedirs(tmp, exist_ok=True)
    desc_path = os.path.join(tmp, "orb_desc.npy")
    if args.host_only:
        out = json.load(open(args.out))
        out["host_restatement"] = host_restatement(desc_path, args.host_scans, not args.host_subset_only)
    else:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--gpu", "--scans",
               str(args.scans), "--host-scans", str(args.host_scans), "--reps", str(args.reps), "--dump", desc_path]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        out = {"bench": "bow_train", "shape": [H, W], "nfeatures": NFEATURES}
        if p.returncode != 0 or not line:
            out["error"] = f"the GPU part ended with status {p.returncode}"
        else:
            out.update(json.loads(line[-1][len("RESULT "):]))
            # per-kernel times of one training at the deepest L, from a traced run of its own
            trace, calls = os.path.join(tmp, "trace"), 3
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace,
                   "-o", "bow_train", "--", sys.executable, os.path.abspath(__file__), "--trace-L", str(LEVELS[-1]), "--scans",
                   str(args.scans), "--reps", str(calls)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                out["error"] = f"the traced pass ended with status {p.returncode}"
            else:
                import bench_bow

                out["kernels"] = {"what": f"rocprofv3 --kernel-trace, per training at k = {K}, L = {LEVELS[-1]} (mean of {calls})",
                                  "per_training": bench_bow.kernel_times(trace, calls, KERNELS)}
            out["random_tree"] = random_tree_figures()
            if not args.no_host and "error" not in out:
                out["host_restatement"] = host_restatement(desc_path, args.host_scans, not args.host_subset_only)
    if not args.work:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
