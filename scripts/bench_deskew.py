"""What lislam_set_distortion costs (GPU box): one continuous odometry chain over a synthetic 300-scan
64 x 1024 batch (bench.py's config-2 shape) on the per-round schedule, modes 0 / 1 / 2 alternating
within one session so that clocks and neighbours are shared.  Per mode: scans/s (median and spread over
the repetitions) and lislam_batch_kernel_times (ms and launches per call; k_odom_to_end and
k_target_index_round are mode 2's TransformToEnd and per-round index builds).  The figure to compare
against is mode 0 on the same schedule in the same run, not bench.py's headline (the chain engine).
usage: python scripts/bench_deskew.py [--scans S] [--reps R] [--out profiles/deskew_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import __graft_entry__ as g  # noqa: E402

MODES = ("off", "queries", "to_end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(_R, "profiles", "deskew_bench.json"))
    args = ap.parse_args()
    pkg = g.package()
    S = args.scans
    scans = pkg.synth.make_sequence(S, args.lines, args.width)
    times = {m: [] for m in MODES}
    kernels = {}
    with pkg.Context(n_scans=args.lines, width=args.width) as ctx:
        b = pkg.Batch(ctx, S)
        b.upload(scans)
        b.extract(S)
        ctx.set_odometry_schedule(ctx.ENGINE_OFF)
        for mode in range(3):  # warm-up: first launches, mode 1 / 2 allocations
            ctx.set_distortion(mode)
            b.odometry(S, S - 1)
        ctx.synchronize()
        for _ in range(args.reps):
            for mode, name in enumerate(MODES):
                ctx.set_distortion(mode)
                t = time.perf_counter()
                b.odometry(S, S - 1)
                ctx.synchronize()
                times[name].append(time.perf_counter() - t)
        b.set_timing(True)  # a separate pass: the events add host work to every launch
        for mode, name in enumerate(MODES):
            ctx.set_distortion(mode)
            b.odometry(S, S - 1)
            ms, launches, _ = b.kernel_times()
            kernels[name] = {k: {"ms": round(float(m), 4), "launches": int(n)}
                             for k, m, n in zip(pkg.native.KERNELS, ms, launches) if n}
        b.set_timing(False)
        stats = np.array([b.download(pkg.native.OUT_STATS, k) for k in range(S)])
        b.close()
    res = {"shape": {"scans": S, "lines": args.lines, "width": args.width, "chains": 1, "schedule": "per-round launches"},
           "reps": args.reps, "solved_pairs_last_mode": int(np.count_nonzero(stats[:, 0] + stats[:, 1])), "modes": {}}
    base = float(np.median(times["off"]))
    for name in MODES:
        t = np.array(times[name])
        med = float(np.median(t))
        res["modes"][name] = {"ms_per_chain_median": round(med * 1e3, 3), "ms_per_chain_min": round(float(t.min()) * 1e3, 3),
                              "ms_per_chain_max": round(float(t.max()) * 1e3, 3), "scans_per_s": round(S / med, 1),
                              "relative_to_off": round(med / base, 3), "kernels": kernels[name]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
