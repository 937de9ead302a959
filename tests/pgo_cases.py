"""Pose graphs shared by the lislam_pgo tests: a there-and-back drive of N keyframes (0.5 m steps, a
turn of pi over five steps at the midpoint) whose odometry edges are the true steps times Exp(noise)
and whose loop edges tie keyframe N-1-3m of the way back to keyframe 3m of the way out."""
import math
from typing import NamedTuple

import numpy as np

import restate_pgo as PG

STEP = 0.5
SIGMA_ROT, SIGMA_TRANS = 2e-3, 2e-2
LOOP_VARIANCE = 0.05
SEED = 20240917
# N -> loop edges of the optimisation cases.  N = 2 and 3 get one (for N = 2 it doubles the chain pair, as
# (1, 0)): prior plus chain alone is exactly determined, its cost at the dead-reckoned start is rounding
# noise and so would be the count of steps that "decrease" it.  N = 1 starts at cost 0 exactly.
LOOPS = {1: 0, 2: 1, 3: 1, 12: 1, 40: 2, 120: 4, 257: 6, 300: 8}


class Case(NamedTuple):
    truth: np.ndarray      # (N, 7)
    nodes: np.ndarray      # (N, 7) initial estimate: the prior pose and the odometry composed
    odom: np.ndarray       # (N-1, 7) measurement of edge (k, k+1)
    prior: np.ndarray      # (7,) the true first pose
    loops: list            # (from, to, meas (7,), var (6,), robust)


def true_step(k, N):
    """Step from keyframe k-1 to k: 0.5 m ahead, and pi / 5 of yaw in the five steps around the midpoint."""
    mid = N // 2
    yaw = math.pi / 5 if mid - 2 <= k <= mid + 2 else 0.0
    return np.array([0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw), STEP, 0.0, 0.0])


def drive(N, L=None, seed=SEED):
    L = LOOPS[N] if L is None else L
    rng = np.random.default_rng(seed)
    first = PG.normalized([0.02, -0.01, 0.3, 0.95, 1.0, -2.0, 0.5])
    truth = [first]
    for k in range(1, N):
        truth.append(PG.normalized(PG.compose(truth[-1], true_step(k, N))))
    noise = rng.normal(size=(max(N - 1, 0), 6)) * ([SIGMA_ROT] * 3 + [SIGMA_TRANS] * 3)
    odom = [PG.normalized(PG.compose(true_step(k, N), PG.se3_exp(noise[k - 1]))) for k in range(1, N)]
    nodes = [first]
    for z in odom:
        nodes.append(PG.normalized(PG.compose(nodes[-1], z)))
    loops = []
    for m in range(L):
        i, j = N - 1 - 3 * m, 3 * m
        assert i > j, "no room for loop %d in %d keyframes" % (m, N)
        loops.append((i, j, PG.between(truth[i], truth[j]), np.full(6, LOOP_VARIANCE), m % 2 == 1))
    return Case(np.array(truth), np.array(nodes), np.array(odom).reshape(-1, 7), first, loops)


def restatement(case, extra=()):
    """The case as a restate_pgo.Graph (prior and odometry with the reference's variances)."""
    g = PG.Graph(case.nodes, prior=(0, case.prior, np.array(PG.ODOMETRY_VARIANCES)))
    for k in range(case.odom.shape[0]):
        g.add_edge(k, k + 1, case.odom[k], PG.ODOMETRY_VARIANCES)
    for e in list(case.loops) + list(extra):
        g.add_edge(*e)
    return g


def pose_gap(a, b):
    """(largest translation difference [m], largest rotation angle between [rad]) of two (n, 7) pose arrays."""
    a, b = np.asarray(a).reshape(-1, 7), np.asarray(b).reshape(-1, 7)
    dt = float(np.max(np.linalg.norm(a[:, 4:] - b[:, 4:], axis=1))) if a.size else 0.0
    dr = max([float(np.linalg.norm(PG.q_log(PG.q_mul(PG.q_conj(PG.normalized(p)[:4]), PG.normalized(q)[:4]))))
              for p, q in zip(a, b)] or [0.0])
    return dt, dr
