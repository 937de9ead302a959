"""GPU checks of the pose graph (lislam_pgo_*: k_pgo_linearize, k_pgo_assemble, k_pgo_sum, k_pgo_factor,
k_pgo_cg, k_pgo_retract, k_pgo_add_batch, k_pgo_pose6d) against the dense numpy restatement
(tests/restate_pgo.py) on the there-and-back graphs of tests/pgo_cases.py.

Tolerances.  Linearisation: both sides are fp64 with the same formulas, rtol 1e-9 / atol 1e-12.  Poses
after optimisation: the project's 1e-4 m / 1e-4 rad (BASELINE.json).  Final cost: relative 1e-8, a
hundred times rel_cost_tol (1e-10), the relative decrease below which either side stops."""
import ctypes
import math

import numpy as np
import pytest

import pgo_cases as C
import place_cases as PC
import restate_pgo as PG
from loop_cases import pose_T

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
COST_RTOL = 1e-8
VAR = np.array(PG.ODOMETRY_VARIANCES)


@pytest.fixture(scope="module")
def ctx16(pkg):
    c = pkg.Context(n_scans=16, width=256)
    yield c
    c.close()


def build(pkg, ctx, case, extra=(), **config):
    N = case.nodes.shape[0]
    g = pkg.PoseGraph(ctx, node_capacity=N, edge_capacity=N + len(case.loops) + len(extra) + 1, **config)
    g.add_nodes(case.nodes)
    g.set_prior(0, case.prior)
    if N > 1:
        g.add_odometry(0, case.odom)
    for i, j, z, var, robust in list(case.loops) + list(extra):
        g.add_edges([i], [j], z[None], var, [robust])
    return g


_REFERENCE = {}


def reference(N):
    """The restatement's optimum of drive(N), computed once."""
    if N not in _REFERENCE:
        r = C.restatement(C.drive(N))
        out = r.optimize()
        _REFERENCE[N] = (out, r.x.copy())
    return _REFERENCE[N]


def assert_same_optimum(g, s, ref_out, ref_x, loops):
    print("iterations %d accepted %d (restatement %d) cost %.17g (restatement %.17g) cg most %d total %d" %
          (s.iterations, s.accepted, ref_out["accepted"], s.final_cost, ref_out["final_cost"], s.cg_most, s.cg_iterations))
    dt, dr = C.pose_gap(g.poses(), ref_x)
    print("pose gap %.3e m %.3e rad" % (dt, dr))
    assert s.iterations < g.cfg.max_iterations
    assert s.accepted == ref_out["accepted"]
    assert abs(s.final_cost - ref_out["final_cost"]) <= COST_RTOL * abs(ref_out["final_cost"])
    assert dt < POSE_TOL and dr < POSE_TOL
    assert s.cg_most <= 6 * loops + 1


def compare_linearization(g, r, x):
    got = g.linearize()
    ref = r.linearize(x)
    for name, a, b in zip(("residual", "J_from", "J_to", "weight", "cost"), got, ref):
        a, b = np.asarray(a), np.asarray(b)
        err = np.abs(a - b)
        rel = (err / np.maximum(np.abs(b), 1e-300))[np.abs(b) > 1e-6]
        print("%s: max abs %.3e, max rel %.3e" % (name, err.max(initial=0.0), rel.max(initial=0.0)))
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("N", [12, 40])
def test_linearization(pkg, ctx16, N):
    """Residuals, both Jacobians, weights and cost at the initial estimate and after one step."""
    case = C.drive(N)
    assert [e[4] for e in case.loops] == ([False] if N == 12 else [False, True])
    g = build(pkg, ctx16, case, max_iterations=1)
    r = C.restatement(case)
    compare_linearization(g, r, r.x)
    s = g.optimize()
    assert s.iterations == 1 and s.accepted == 1
    x1 = g.poses()
    assert C.pose_gap(x1, case.nodes)[0] > 1e-6  # the step moved the estimate: the second comparison is at another point
    compare_linearization(g, r, np.array([PG.normalized(p) for p in x1]))
    g.close()


@pytest.mark.parametrize("N", [1, 2, 3, 40, 257])
def test_optimize(pkg, ctx16, N):
    """257 nodes exceed a 256-thread workgroup (and would add a ninth level to a cyclic reduction)."""
    case = C.drive(N)
    ref_out, ref_x = reference(N)
    g = build(pkg, ctx16, case)
    s = g.optimize()
    assert (s.nodes, s.edges) == (N, N - 1 + len(case.loops))
    assert s.initial_cost == pytest.approx(ref_out["initial_cost"], rel=1e-9, abs=1e-300)
    assert_same_optimum(g, s, ref_out, ref_x, sum(abs(e[0] - e[1]) != 1 for e in case.loops))
    g.close()


def _exact_chain(N):
    c = C.drive(N, L=0)
    odom = np.array([PG.between(c.truth[k], c.truth[k + 1]) for k in range(N - 1)])
    return C.Case(c.truth, c.truth.copy(), odom, c.prior, [])


def test_exact_chain_stays_put(pkg, ctx16):
    """Residuals of about 1e-16 go through the small-angle branches: no NaN, nothing moves."""
    case = _exact_chain(40)
    g = build(pkg, ctx16, case)
    lin = g.linearize()
    assert all(np.isfinite(a).all() for a in lin[:4]) and math.isfinite(lin.cost)
    s = g.optimize()
    x = g.poses()
    print("cost %.3e -> %.3e, iterations %d, accepted %d" % (s.initial_cost, s.final_cost, s.iterations, s.accepted))
    assert np.isfinite(x).all() and np.isfinite(s.stats).all()
    dt, dr = C.pose_gap(x, case.nodes)
    assert dt < 1e-12 and dr < 1e-12
    assert s.final_cost <= s.initial_cost
    g.close()


def test_noisy_chain_without_loops_is_already_optimal(pkg, ctx16):
    """Prior plus chain is exactly determined: the dead-reckoned estimate is the optimum.  Whatever a
    rounding-level step moves is far below 1e-10 (coordinates of tens of metres at 1e-16)."""
    case = C.drive(40, L=0)
    g = build(pkg, ctx16, case)
    s = g.optimize()
    dt, dr = C.pose_gap(g.poses(), case.nodes)
    print("cost %.3e -> %.3e, moved %.3e m %.3e rad, cg most %d" % (s.initial_cost, s.final_cost, dt, dr, s.cg_most))
    assert dt < 1e-10 and dr < 1e-10 and s.final_cost <= s.initial_cost and s.final_cost < 1e-12
    assert s.cg_most <= 1  # the preconditioner is the whole matrix
    g.close()


def _extra(case, i, j, robust=False):
    return (i, j, PG.between(case.truth[i], case.truth[j]), np.full(6, C.LOOP_VARIANCE), robust)


@pytest.mark.parametrize("shape", ["duplicates_chain_pair", "forward_edge", "shared_node"])
def test_edge_shapes(pkg, ctx16, shape):
    case = C.drive(40)  # its two loops are (39, 0) and (36, 3): from > to
    extra = {"duplicates_chain_pair": [_extra(case, 10, 11)],
             "forward_edge": [_extra(case, 5, 25)],
             "shared_node": [_extra(case, 30, 3), _extra(case, 33, 3, True)]}[shape]
    r = C.restatement(case, extra)
    ref_out = r.optimize()
    g = build(pkg, ctx16, case, extra)
    s = g.optimize()
    off = sum(abs(e[0] - e[1]) != 1 for e in list(case.loops) + extra)
    assert off == {"duplicates_chain_pair": 2, "forward_edge": 3, "shared_node": 4}[shape]
    assert_same_optimum(g, s, ref_out, r.x, off)
    g.close()


def test_determinism(pkg, ctx16):
    case = C.drive(257)
    out = []
    for _ in range(2):
        g = build(pkg, ctx16, case)
        s = g.optimize()
        out.append((g.poses().tobytes(), s.stats.tobytes(), s[:7]))
        g.close()
    assert out[0] == out[1]


def test_incremental_use(pkg, ctx16):
    """mapOdomHandle's pattern: a node, its odometry edge, optimize; loop edges when their newer node arrives."""
    N = 40
    case = C.drive(N)
    _, ref_x = reference(N)
    batch = build(pkg, ctx16, case)
    batch.optimize()
    g = pkg.PoseGraph(ctx16, node_capacity=N, edge_capacity=N + 2)
    g.add_nodes(case.nodes[:1])
    g.set_prior(0, case.prior)
    capped = 0
    for k in range(1, N):
        last = PG.normalized(g.poses(k - 1, 1)[0])
        g.add_nodes(PG.compose(last, case.odom[k - 1])[None])
        g.add_odometry(k - 1, case.odom[k - 1:k])
        for i, j, z, var, robust in case.loops:
            if i == k:
                g.add_edges([i], [j], z[None], var, [robust])
        s = g.optimize()
        capped += s.iterations >= g.cfg.max_iterations
    assert capped == 0 and g.size() == batch.size()
    for other in (batch.poses(), ref_x):
        dt, dr = C.pose_gap(g.poses(), other)
        print("gap %.3e m %.3e rad" % (dt, dr))
        assert dt < POSE_TOL and dr < POSE_TOL
    g.close()
    batch.close()


def test_add_batch(pkg, synth, ctx16):
    n = 8
    b = pkg.Batch(ctx16, n)
    b.upload(synth.make_sequence(n, 16, 256))
    b.extract(n)
    b.odometry(n, n - 1)
    pose = np.array([b.download(pkg.native.OUT_POSE, k) for k in range(n)]).reshape(n, 7)
    g = pkg.PoseGraph(ctx16, node_capacity=n, edge_capacity=n)
    g.add_batch(b, 0, 5)
    g.add_batch(b, 5, 3)  # continues the chain from scan 4
    assert g.size() == (n, n - 1)
    assert g.poses().tobytes() == pose.tobytes()
    i, j, z, var, robust = g.edges()
    assert list(i) == list(range(n - 1)) and list(j) == list(range(1, n)) and not robust.any()
    assert np.allclose(var, VAR, rtol=1e-14, atol=0)
    assert np.abs(pose[1:, 4:] - pose[:-1, 4:]).max() > 1e-3  # the odometry moved
    for k in range(n - 1):
        ref = PG.between(PG.normalized(pose[k]), PG.normalized(pose[k + 1]))
        assert np.abs(z[k] - ref).max() < 1e-12, k
    g.set_prior(0, pose[0])
    s = g.optimize()
    assert s.final_cost <= s.initial_cost and C.pose_gap(g.poses(), pose)[0] < 1e-9
    g.close()
    b.close()


def test_hand_off_from_detection_and_icp(pkg, synth, ctx16):
    """detect -> loop_closure_icp -> add_loop -> optimize on the drive of test_gpu_place's hand-off test."""
    n = 2 * PC.N_OUT
    b = pkg.Batch(ctx16, n)
    b.upload(PC.there_and_back(synth))
    b.extract(n)
    tracks = {k: b.download(pkg.native.OUT_CLOUD_TRACK, k) for k in (0, n - 1)}
    sc = pkg.ScanContext(ctx16, capacity=n)
    sc.add_batch(b, 0, n)
    d = sc.detect(n - 1, 1)
    sc.close()
    b.close()
    loop_id, yaw = int(d.loop_id[0]), float(d.yaw[0])
    assert loop_id == 0
    # keyframe poses: the drive's, with an odometry drift of 2 mm and 0.2 mrad per step
    truth = np.array([PG.matrix_pose(pose_T(PC.drive_pose(synth, k))) for k in range(n)])
    rng = np.random.default_rng(3)
    odom = np.array([PG.compose(PG.between(truth[k], truth[k + 1]), PG.se3_exp(rng.normal(size=6) * ([2e-4] * 3 + [2e-3] * 3)))
                     for k in range(n - 1)])
    nodes = [truth[0]]
    for z in odom:
        nodes.append(PG.normalized(PG.compose(nodes[-1], z)))
    g = pkg.PoseGraph(ctx16, node_capacity=n, edge_capacity=n)
    g.add_nodes(np.array(nodes))
    g.set_prior(0, truth[0])
    g.add_odometry(0, odom)
    c, s = math.cos(-yaw), math.sin(-yaw)
    Rz = np.eye(4)
    Rz[:2, :2] = [[c, -s], [s, c]]
    T_hist = pkg.loop.get_transform_matrix(*g.key_poses_6d(loop_id, 1)[0])
    T_cur = T_hist @ Rz
    T_icp, T_cur2map, fitness, info = pkg.loop.loop_closure_icp(ctx16, tracks[n - 1], T_cur, [tracks[loop_id]], [T_hist])
    assert info[0] == pkg.loop.ACCEPTED and fitness > 0
    g.add_loop(n - 1, loop_id, T_cur2map, T_hist, fitness)
    before = float(np.linalg.norm(g.linearize().residual[n - 1]))
    s = g.optimize()
    after = float(np.linalg.norm(g.linearize().residual[n - 1]))
    print("loop residual %.4f -> %.4f, cost %.4f -> %.4f, %d iterations" % (before, after, s.initial_cost, s.final_cost, s.iterations))
    assert s.iterations < g.cfg.max_iterations and after < before and s.final_cost < s.initial_cost
    x = g.poses()
    for k, p6 in enumerate(g.key_poses_6d()):
        assert np.allclose(pkg.loop.get_transform_matrix(*p6), PG.pose_matrix(x[k]), rtol=0, atol=2e-5), k
    g.close()


def test_argument_errors_leave_the_graph_unchanged(pkg, ctx16):
    n = pkg.native
    lib = ctx16.lib
    case = C.drive(12)
    g = pkg.PoseGraph(ctx16, node_capacity=12, edge_capacity=13)
    g.add_nodes(case.nodes)
    g.set_prior(0, case.prior)
    g.add_odometry(0, case.odom)
    before = (g.size(), g.poses().tobytes(), [a.tobytes() for a in g.edges()])

    def err():
        return lib.lislam_last_error(ctx16.h).decode()

    def add(i, j, var=0.05, count=1):
        f, t = np.array(i, np.int32), np.array(j, np.int32)
        z = np.tile(case.odom[0], (count, 1))
        v = np.full((count, 6), var)
        return lib.lislam_pgo_add_edges(g.h, n.ptr(f), n.ptr(t), n.ptr(z), n.ptr(v), None, count)

    assert add([12], [0]) == n.ERR_ARG and "invalid" in err()
    assert add([-1], [0]) == n.ERR_ARG
    assert add([3], [3]) == n.ERR_ARG
    assert add([3], [7], var=0.0) == n.ERR_ARG and "positive" in err()
    assert add([3], [7], var=-1.0) == n.ERR_ARG
    assert add([3, 3], [7, 3], count=2) == n.ERR_ARG  # the valid first edge of a bad call is not kept
    assert add([3, 4, 5], [7, 8, 9], count=3) == n.ERR_CAPACITY and "capacity" in err()
    assert lib.lislam_pgo_add_nodes(g.h, n.ptr(case.nodes), 1) == n.ERR_CAPACITY
    assert lib.lislam_pgo_set_prior(g.h, 12, n.ptr(case.prior), n.ptr(VAR)) == n.ERR_ARG
    assert lib.lislam_pgo_set_prior(g.h, 0, n.ptr(case.prior), n.ptr(np.zeros(6))) == n.ERR_ARG
    assert lib.lislam_pgo_poses(g.h, 5, 8, None, None) == n.ERR_ARG and "range" in err()
    assert (g.size(), g.poses().tobytes(), [a.tobytes() for a in g.edges()]) == before
    h = ctypes.c_void_p()
    bad = n.PgoConfig(lambda_init=0.0)
    assert lib.lislam_pgo_create(ctx16.h, ctypes.byref(bad), 4, 4, ctypes.byref(h)) == n.ERR_ARG
    assert lib.lislam_pgo_create(ctx16.h, None, 0, 4, ctypes.byref(h)) == n.ERR_ARG
    empty = pkg.PoseGraph(ctx16, node_capacity=2, edge_capacity=1)
    empty.add_nodes(case.nodes[:2])
    assert lib.lislam_pgo_optimize(empty.h, None, None) == n.ERR_STATE and "prior" in err()
    empty.close()
    assert add([11], [0]) == n.OK and g.size() == (12, 12)  # and a valid call still works
    g.close()
