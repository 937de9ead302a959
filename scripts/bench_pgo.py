#!/usr/bin/env python3
"""Times the pose-graph optimization (lislam_pgo_optimize) on the GPU on a 3,000-node there-and-back
graph with 30 loop edges (tests/pgo_cases.py's generator: 0.5 m steps, odometry noise 2e-3 rad /
2e-2 m, the reference's odometry variances, loop variance 0.05, every second loop robust).

``optimize`` is timed on a fresh copy of the graph each time (wall clock around the call: it returns
once the result is on the host), ``--reps`` runs after ``--warmup``.  Beside it stands a CPU figure: the
numpy restatement of the same problem and outer loop (tests/restate_pgo.py) with
scipy.sparse.linalg.spsolve as the linear solver, run once; its factors are evaluated in Python, so the
time of the sparse solves alone is given too.  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_pgo.py [--nodes 3000] [--loops 30] [--reps 20] [--out profiles/pgo_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "intensity_based_lidar_slam_for_me-_amd"
TRIDIAGONAL_SOLVE = "one-wave block Thomas sweep (block LDL' by 36 lanes, sweeps by 6 lanes); cyclic reduction is not built"


def cpu_sparse(case, PG, C):
    """restate_pgo.Graph.optimize with the dense solve replaced by scipy's sparse one."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve

    g = C.restatement(case)
    N, E = g.x.shape[0], len(g.frm)
    cfg = PG.DEFAULTS

    def normal_equations(x):
        r, Jf, Jt, w, cost = g.linearize(x)
        rows, cols, vals = [], [], []
        grad = np.zeros(6 * N)
        k6 = np.arange(6)
        for e in range(E + 1):
            blocks = [(g.prior[0], Jt[e])] if e == E else [(g.frm[e], Jf[e]), (g.to[e], Jt[e])]
            for a, Ja in blocks:
                grad[6 * a:6 * a + 6] += w[e] * (Ja.T @ r[e])
                for b, Jb in blocks:
                    rows.append(np.repeat(6 * a + k6, 6))
                    cols.append(np.tile(6 * b + k6, 6))
                    vals.append((w[e] * (Ja.T @ Jb)).ravel())
        H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * N, 6 * N))
        return H, grad, cost

    t_solve = 0.0
    t0 = time.perf_counter()
    lam = cfg["lambda_init"]
    H, grad, cost = normal_equations(g.x)
    out = {"initial_cost": cost, "iterations": 0, "accepted": 0}
    while out["iterations"] < cfg["max_iterations"]:
        out["iterations"] += 1
        d = np.clip(H.diagonal(), PG.DIAG_MIN, PG.DIAG_MAX)
        t1 = time.perf_counter()
        delta = spsolve((H + sp.diags(lam * d)).tocsc(), -grad).reshape(N, 6)
        t_solve += time.perf_counter() - t1
        trial = np.array([PG.retract(g.x[k], delta[k]) for k in range(N)])
        c_new = g.cost(trial)
        if c_new < cost:
            rel = (cost - c_new) / cost
            g.x = trial
            out["accepted"] += 1
            lam = max(lam / 10.0, PG.LAMBDA_MIN)
            H, grad, cost = normal_equations(g.x)
            if rel < cfg["rel_cost_tol"]:
                break
        else:
            lam *= 10.0
            if lam > PG.LAMBDA_MAX:
                break
    out.update(final_cost=cost, total_s=round(time.perf_counter() - t0, 3), spsolve_s=round(t_solve, 4),
               spsolve_ms_per_solve=round(1e3 * t_solve / out["iterations"], 3))
    return out, g.x


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=3000)
    ap.add_argument("--loops", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy figure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pgo_cases as C
    import restate_pgo as PG

    N, L = args.nodes, args.loops
    case = C.drive(N, L)
    cpu, cpu_x = (None, None) if args.no_cpu else cpu_sparse(case, PG, C)

    pkg = importlib.import_module(PKG)
    ctx = pkg.Context(n_scans=16, width=256)
    frm = np.array([e[0] for e in case.loops], np.int32)
    to = np.array([e[1] for e in case.loops], np.int32)
    meas = np.array([e[2] for e in case.loops]).reshape(-1, 7)
    var = np.array([e[3] for e in case.loops]).reshape(-1, 6)
    robust = np.array([e[4] for e in case.loops], np.int32)

    def fresh():
        g = pkg.PoseGraph(ctx, node_capacity=N, edge_capacity=N - 1 + L)
        g.add_nodes(case.nodes)
        g.set_prior(0, case.prior)
        g.add_odometry(0, case.odom)
        if L:
            g.add_edges(frm, to, meas, var, robust)
        return g

    ms, s, x = [], None, None
    for k in range(args.warmup + args.reps):
        g = fresh()
        ctx.synchronize()
        t0 = time.perf_counter()
        s = g.optimize()
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            ms.append(1e3 * dt)
        x = g.poses()
        g.close()
    ctx.close()
    out = {"bench": "pgo", "nodes": N, "edges": N - 1 + L, "loop_edges": L, "reps": args.reps,
           "optimize_ms_median": round(float(np.median(ms)), 3), "optimize_ms_min": round(float(np.min(ms)), 3),
           "optimize_ms_max": round(float(np.max(ms)), 3), "status": pkg.posegraph.STATUS[s.status],
           "lm_iterations": s.iterations, "accepted_steps": s.accepted, "cg_iterations_total": s.cg_iterations,
           "cg_iterations_most": s.cg_most, "ms_per_lm_iteration": round(float(np.median(ms)) / max(s.iterations, 1), 3),
           "initial_cost": s.initial_cost, "final_cost": s.final_cost, "cg_last_relres": s.cg_relres,
           "tridiagonal_solve": TRIDIAGONAL_SOLVE}
    if cpu is not None:
        dt, dr = C.pose_gap(x, cpu_x)
        out["cpu_scipy_spsolve"] = dict(cpu, pose_gap_m=dt, pose_gap_rad=dr)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
