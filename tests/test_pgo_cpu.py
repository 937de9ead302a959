"""CPU checks of the pose graph (lislam_pgo_*): the header declares the ABI and the library exports it,
the config struct's layout and defaults, kernel names, null arguments, and self-checks of the
restatement (tests/restate_pgo.py).  No compute call without a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pgo_cases as C
import restate_pgo as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lislam.h")
PGO_FUNCTIONS = ["lislam_pgo_add_batch", "lislam_pgo_add_edges", "lislam_pgo_add_nodes", "lislam_pgo_create",
                 "lislam_pgo_destroy", "lislam_pgo_edges", "lislam_pgo_linearize", "lislam_pgo_optimize", "lislam_pgo_poses",
                 "lislam_pgo_set_prior", "lislam_pgo_size"]


def test_header_declares_and_library_exports_pgo_api(pkg):
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"^\s*int\s+(lislam_pgo_\w+)\s*\(", text, re.M)))
    assert declared == PGO_FUNCTIONS
    lib = pkg.native.load()
    assert all(hasattr(lib, f) for f in PGO_FUNCTIONS)
    assert set(PGO_FUNCTIONS) <= set(pkg.native.EXPORTED_SYMBOLS)
    for name, value in (("LISLAM_PGO_CONVERGED", pkg.native.PGO_CONVERGED), ("LISLAM_PGO_LAMBDA_LIMIT", pkg.native.PGO_LAMBDA_LIMIT),
                        ("LISLAM_PGO_MAX_ITERATIONS", pkg.native.PGO_MAX_ITERATIONS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value
    assert "pi - 0.1" in text  # the domain of Log is stated


def test_pgo_config_layout_and_defaults(pkg):
    n = pkg.native
    assert ctypes.sizeof(n.PgoConfig) == 32
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} lislam_pgo_config;", text).group(1)
    fields = re.findall(r"(int32_t|double)\s+(\w+);\s*/\*.*\(([-0-9.e]+)\) \*/", body)
    assert [f[1] for f in fields] == [k for k, _ in n.PgoConfig._fields_]
    c = n.PgoConfig()
    got = {k: getattr(c, k) for k, _ in n.PgoConfig._fields_}
    assert got == {f[1]: (int(f[2]) if f[0] == "int32_t" else float(f[2])) for f in fields}
    assert got == PG.DEFAULTS
    assert pkg.PoseGraph is pkg.posegraph.PoseGraph
    assert pkg.posegraph.ODOMETRY_VARIANCES == PG.ODOMETRY_VARIANCES


def test_pgo_kernels_are_in_the_library(pkg):
    data = open(pkg.native.LIB_PATH, "rb").read()
    for k in pkg.native.PGO_KERNELS:
        assert k.encode() in data, k


def test_pgo_null_arguments(pkg):
    lib, E = pkg.native.load(), pkg.native.ERR_ARG
    h = ctypes.c_void_p()
    assert lib.lislam_pgo_create(None, None, 4, 4, ctypes.byref(h)) == E
    assert lib.lislam_pgo_destroy(None) == E
    assert lib.lislam_pgo_size(None, None, None) == E
    assert lib.lislam_pgo_add_nodes(None, None, 0) == E
    assert lib.lislam_pgo_set_prior(None, 0, None, None) == E
    assert lib.lislam_pgo_add_edges(None, None, None, None, None, None, 0) == E
    assert lib.lislam_pgo_add_batch(None, None, 0, 0, None) == E
    assert lib.lislam_pgo_edges(None, 0, 0, None, None, None, None, None) == E
    assert lib.lislam_pgo_linearize(None, None, None, None, None, None) == E
    assert lib.lislam_pgo_optimize(None, None, None) == E
    assert lib.lislam_pgo_poses(None, 0, 0, None, None) == E


def _random_pose(rng, rot=0.8, trans=2.0):
    return PG.se3_exp(rng.normal(size=6) * ([rot] * 3 + [trans] * 3))


def _central(f, T, h=1e-6):
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        J[:, k] = (f(PG.retract(T, d)) - f(PG.retract(T, -d))) / (2 * h)
    return J


@pytest.mark.parametrize("angle", [None, 2e-3, 5e-4, 0.0])
def test_restatement_jacobians_against_central_differences(angle):
    """angle: the rotation of Z^-1 h (None: whatever random poses give); 5e-4 and 0 take the series branches."""
    rng = np.random.default_rng(11)
    var = np.array([1e-2, 2e-2, 3e-2, 1e-1, 2e-1, 3e-1])
    Ti, Tj, Z = _random_pose(rng), _random_pose(rng), _random_pose(rng)
    if angle is not None:
        xi = rng.normal(size=6)
        xi[:3] *= angle / np.linalg.norm(xi[:3])
        xi[3:] *= angle
        Z = PG.compose(PG.between(Ti, Tj), PG.se3_exp(-xi))
    e, Jf, Jt = PG.between_factor(Ti, Tj, Z, var)
    if angle is not None:
        assert abs(np.linalg.norm(e[:3] * np.sqrt(var[:3])) - angle) < 1e-12
    assert np.abs(_central(lambda T: PG.between_factor(T, Tj, Z, var)[0], Ti) - Jf).max() < 1e-7
    assert np.abs(_central(lambda T: PG.between_factor(Ti, T, Z, var)[0], Tj) - Jt).max() < 1e-7
    P = Z if angle is None else PG.compose(Tj, PG.se3_exp(-xi))
    Jp = PG.prior_factor(Tj, P, var)[1]
    assert np.abs(_central(lambda T: PG.prior_factor(T, P, var)[0], Tj) - Jp).max() < 1e-7


def test_restatement_exp_log_round_trip():
    rng = np.random.default_rng(5)
    for scale in (1.0, 1.1e-2, 0.9e-2, 1e-3, 1e-5, 1e-8, 1e-9, 0.0):
        xi = rng.normal(size=6) * scale
        T = PG.se3_exp(xi)
        assert np.abs(PG.se3_log(T) - xi).max() <= 1e-14 * max(1.0, scale) + 1e-12 * scale
        assert np.abs(PG.se3_exp(PG.se3_log(T)) - T).max() < 1e-14
    big = np.array([0, 0, math.pi - 0.1, 1.0, -2.0, 0.5])  # the edge of the stated domain
    assert np.abs(PG.se3_log(PG.se3_exp(big)) - big).max() < 1e-12
    assert np.abs(PG.dlog(np.zeros(6)) - np.eye(6)).max() == 0.0
    assert np.abs(PG.se3_log(np.array([0, 0, 0, 1.0, 0, 0, 0]))).max() == 0.0


def test_restatement_small_angle_branches_are_continuous():
    """Each coefficient function, and D and Exp built from them, on either side of the switch.  The series
    are exact to 1e-16 there.  The closed forms carry the absolute rounding of 1 - gamma (about eps) divided
    by a power of the angle, and the term they scale multiplies that power back: a coefficient may jump by
    1e-13 / angle^p, p = the power of the angle in its term (a4 ad^4: 3, with one factor from v)."""
    lo, hi = PG.SMALL * (1 - 1e-9), PG.SMALL * (1 + 1e-9)
    for f, powers in ((PG.half_cot, (0, 2)), (PG.exp_coeffs, (1, 1, 2)), (PG.dlog_coeffs, (1, 3))):
        for a, b, p in zip(f(lo), f(hi), powers):
            assert abs(a - b) * PG.SMALL ** p <= 1e-13, f.__name__
    u = np.array([0.6, -0.48, 0.64, 0, 0, 0])
    v = np.array([0, 0, 0, 0.3, -0.2, 0.1])
    assert np.abs(PG.dlog(lo * u + v) - PG.dlog(hi * u + v)).max() < 1e-11  # d D / d angle * 2e-11
    assert np.abs(PG.se3_exp(lo * u + v) - PG.se3_exp(hi * u + v)).max() < 1e-11
    for n in (PG.TINY * (1 - 1e-9), PG.TINY * (1 + 1e-9)):
        q = np.concatenate([n * u[:3], [math.sqrt(1 - n * n)]])
        assert abs(np.linalg.norm(PG.q_log(q)) - 2 * math.asin(n)) < 1e-22


def test_restatement_minimum_has_no_gradient():
    g = C.restatement(C.drive(12))
    out = g.optimize()
    assert out["iterations"] < PG.DEFAULTS["max_iterations"] and out["accepted"] >= 2
    assert out["final_cost"] < out["initial_cost"]
    assert out["gradient"] < 1e-6 * out["gradient0"]


def test_cases_do_not_stop_at_the_iteration_cap():
    for N in (40, 120):
        out = C.restatement(C.drive(N)).optimize()
        assert out["iterations"] < PG.DEFAULTS["max_iterations"], N


def test_key_pose_6d_round_trip(pkg):
    """get_transform_matrix(*key_pose_6d(T)) == T for |pitch| < pi / 2 - 0.1."""
    rng = np.random.default_rng(9)
    for _ in range(200):
        roll, yaw = rng.uniform(-math.pi, math.pi, 2)
        pitch = rng.uniform(-(math.pi / 2 - 0.1), math.pi / 2 - 0.1)
        T = pkg.loop.get_transform_matrix(*rng.uniform(-50, 50, 3), roll, pitch, yaw)
        for helper in (pkg.posegraph.key_pose_6d, PG.key_pose_6d):
            assert np.abs(pkg.loop.get_transform_matrix(*helper(T)) - T).max() < 1e-12
        assert np.abs(PG.pose_matrix(pkg.posegraph.matrix_to_pose(T)) - T).max() < 1e-12
        assert np.abs(pkg.posegraph.matrix_to_pose(T) - PG.matrix_pose(T)).max() < 1e-15
