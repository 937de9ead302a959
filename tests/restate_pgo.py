"""Dense numpy restatement of the pose-graph problem of lislam_pgo_* (include/lislam.h): the factors of
feature_tracker::mapOdomHandle / loopClosureThread (src/intensity_feature_tracker.cpp:395-583,
:314-381) as one least-squares problem, its Jacobians and the Levenberg-Marquardt outer loop, with
np.linalg.solve as the linear solver.  Checker only: nothing here runs on the GPU.

Poses are 7 doubles qx qy qz qw tx ty tz; tangent vectors are [omega(3), v(3)] (GTSAM's Pose3 order);
Exp / Log are the full SE(3) maps and the retraction is T <- T Exp(delta).

The residual path (normalisation, between, Log) spells its sums and products out left to right in
Python floats, without BLAS and so without fused multiply-adds: a dead-reckoned estimate leaves residuals
that are nothing but rounding (about 1e-16 / sigma), and only a fixed evaluation order makes those
comparable between two implementations.
"""
import math

import numpy as np

SMALL = 1e-2          # below this angle the coefficient functions use their series (truncation below 1e-16
                      # relative there; the closed forms cancel to about 60 eps / angle^2 = 1e-10 at worst)
TINY = 1e-8           # below this |vec q| the quaternion logarithm's atan2(n, w) / n is replaced by its limit
DEFAULTS = {"max_iterations": 50, "cg_max_iterations": 0, "lambda_init": 1e-4, "rel_cost_tol": 1e-10, "cg_rel_tol": 1e-12}
ODOMETRY_VARIANCES = (1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6)   # odometryNoise_ / priorNoise_ (:41-44)
LAMBDA_MIN, LAMBDA_MAX, DIAG_MIN, DIAG_MAX = 1e-12, 1e10, 1e-6, 1e32


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def matvec3(R, d):
    return np.array([R[r][0] * d[0] + R[r][1] * d[1] + R[r][2] * d[2] for r in range(3)])


def norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


# ---------------------------------------------------------------------------- quaternions, poses
def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def normalized(p):
    p = np.array(p, np.float64)
    p[:4] /= math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3])
    return p


def compose(a, b):
    """a * b of two (normalized) poses."""
    return np.concatenate([q_mul(a[:4], b[:4]), a[4:] + q_rot(a[:4]) @ b[4:]])


def between(a, b):
    """a^-1 * b."""
    qi = q_conj(a[:4])
    return np.concatenate([q_mul(qi, b[:4]), matvec3(q_rot(qi), b[4:] - a[4:])])


def pose_matrix(p):
    p = normalized(p)
    T = np.eye(4)
    T[:3, :3] = q_rot(p[:4])
    T[:3, 3] = p[4:]
    return T


def matrix_pose(T):
    """4x4 -> pose7 (Shepperd's method)."""
    R = np.asarray(T, np.float64)[:3, :3]
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    return normalized(np.concatenate([q, np.asarray(T, np.float64)[:3, 3]]))


# ---------------------------------------------------------------------------- coefficient functions
def half_cot(th):
    """gamma = (th / 2) cot(th / 2) and (1 - gamma) / th^2."""
    if th < SMALL:
        t2 = th * th
        return 1.0 - t2 / 12.0 - t2 * t2 / 720.0, 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0
    g = 0.5 * th * math.cos(0.5 * th) / math.sin(0.5 * th)
    return g, (1.0 - g) / (th * th)


def exp_coeffs(th):
    """sin(th/2)/th, (1 - cos th)/th^2, (th - sin th)/th^3."""
    t2 = th * th
    if th < SMALL:
        return 0.5 - t2 / 48.0 + t2 * t2 / 3840.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0
    return math.sin(0.5 * th) / th, (1.0 - math.cos(th)) / t2, (th - math.sin(th)) / (t2 * th)


def dlog_coeffs(th):
    """a2, a4 of Jr^-1(xi) = I + ad/2 + a2 ad^2 + a4 ad^4 (ad's minimal polynomial is x (x^2 + th^2)^2)."""
    t2 = th * th
    if th < SMALL:
        return 1.0 / 12.0 - t2 * t2 / 30240.0, -1.0 / 720.0 - t2 / 15120.0
    s, c = math.sin(0.5 * th), math.cos(0.5 * th)
    g = 0.5 * th * c / s
    dg = 0.5 * c / s - 0.25 * th / (s * s)   # d gamma / d th
    return (2.0 * (1.0 - g) + 0.5 * th * dg) / t2, (1.0 - g + 0.5 * th * dg) / (t2 * t2)


# ---------------------------------------------------------------------------- Exp, Log, D, Ad
def q_log(q):
    """Rotation vector of a unit quaternion (angle below pi)."""
    v = np.array(q[:3], np.float64)
    w = q[3]
    if w < 0:
        v, w = -v, -w
    n = norm3(v)
    if n < TINY:
        k = 2.0 / w * (1.0 - n * n / (3.0 * w * w))
    else:
        k = 2.0 * math.atan2(n, w) / n
    return k * v


def se3_log(p):
    """[omega, v] of a (normalized) pose."""
    w = q_log(p[:4])
    _, c = half_cot(norm3(w))
    t = p[4:]
    wt = cross(w, t)
    return np.concatenate([w, t - 0.5 * wt + c * cross(w, wt)])


def se3_exp(xi):
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = math.sqrt(float(w @ w))
    a, b, c = exp_coeffs(th)
    W = skew(w)
    q = np.concatenate([a * w, [math.cos(0.5 * th)]])
    return np.concatenate([q, v + b * (W @ v) + c * (W @ (W @ v))])


def ad(xi):
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = skew(xi[:3])
    A[3:, :3] = skew(xi[3:])
    return A


def dlog(xi):
    """D: the inverse right Jacobian of SE(3) at xi."""
    th = math.sqrt(float(xi[:3] @ xi[:3]))
    a2, a4 = dlog_coeffs(th)
    A = ad(xi)
    A2 = A @ A
    return np.eye(6) + 0.5 * A + a2 * A2 + a4 * (A2 @ A2)


def adjoint(p):
    R = q_rot(p[:4])
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = R
    A[3:, :3] = skew(p[4:]) @ R
    return A


def inverse(p):
    qi = q_conj(p[:4])
    return np.concatenate([qi, -(q_rot(qi) @ p[4:])])


def retract(p, d):
    return normalized(compose(normalized(p), se3_exp(d)))


# ---------------------------------------------------------------------------- factors
def between_factor(Ti, Tj, Z, var):
    """Whitened residual, J_from, J_to of a BetweenFactor<Pose3>."""
    sig = np.sqrt(np.asarray(var, np.float64))
    h = between(normalized(Ti), normalized(Tj))
    xi = se3_log(between(normalized(Z), h))
    D = dlog(xi)
    return xi / sig, -(D @ adjoint(inverse(h))) / sig[:, None], D / sig[:, None]


def prior_factor(T, P, var):
    sig = np.sqrt(np.asarray(var, np.float64))
    xi = se3_log(between(normalized(P), normalized(T)))
    return xi / sig, dlog(xi) / sig[:, None]


class Graph:
    """nodes (N, 7); edges = lists from, to, meas (E, 7), var (E, 6), robust (E,); one prior."""

    def __init__(self, nodes, prior=None):
        self.x = np.array([normalized(p) for p in np.asarray(nodes, np.float64).reshape(-1, 7)]).reshape(-1, 7)
        self.frm, self.to, self.meas, self.var, self.robust = [], [], [], [], []
        self.prior = prior   # (node, pose7, var6)

    def add_edge(self, i, j, Z, var, robust=False):
        self.frm.append(int(i)); self.to.append(int(j)); self.meas.append(normalized(Z))
        self.var.append(np.asarray(var, np.float64)); self.robust.append(bool(robust))

    def linearize(self, x=None):
        """residual (E+1, 6), J_from (E, 6, 6), J_to (E+1, 6, 6), weight (E+1,), cost; the prior last."""
        x = self.x if x is None else x
        E = len(self.frm)
        r = np.zeros((E + 1, 6)); Jf = np.zeros((E, 6, 6)); Jt = np.zeros((E + 1, 6, 6)); w = np.ones(E + 1)
        cost = 0.0
        for e in range(E):
            r[e], Jf[e], Jt[e] = between_factor(x[self.frm[e]], x[self.to[e]], self.meas[e], self.var[e])
            s = float(r[e] @ r[e])
            if self.robust[e]:
                w[e] = 1.0 / (1.0 + s)
                cost += 0.5 * math.log1p(s)
            else:
                cost += 0.5 * s
        node, P, var = self.prior
        r[E], Jt[E] = prior_factor(x[node], P, var)
        cost += 0.5 * float(r[E] @ r[E])
        return r, Jf, Jt, w, cost

    def cost(self, x):
        return self.linearize(x)[4]

    def normal_equations(self, x=None):
        N, E = self.x.shape[0], len(self.frm)
        r, Jf, Jt, w, cost = self.linearize(x)
        H = np.zeros((6 * N, 6 * N)); g = np.zeros(6 * N)
        for e in range(E + 1):
            cols = [(self.prior[0], Jt[e])] if e == E else [(self.frm[e], Jf[e]), (self.to[e], Jt[e])]
            for a, Ja in cols:
                g[6 * a:6 * a + 6] += w[e] * (Ja.T @ r[e])
                for b, Jb in cols:
                    H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += w[e] * (Ja.T @ Jb)
        return H, g, cost

    def optimize(self, **config):
        """The outer loop of lislam_pgo_optimize -> dict(iterations, accepted, initial_cost, final_cost,
        lam, gradient0, gradient).  self.x holds the result."""
        cfg = dict(DEFAULTS, **config)
        N = self.x.shape[0]
        lam = cfg["lambda_init"]
        H, g, cost = self.normal_equations()
        out = {"initial_cost": cost, "gradient0": float(np.max(np.abs(g))) if N else 0.0, "iterations": 0, "accepted": 0}
        while N and out["iterations"] < cfg["max_iterations"]:
            out["iterations"] += 1
            d = np.clip(np.diag(H), DIAG_MIN, DIAG_MAX)
            delta = np.linalg.solve(H + lam * np.diag(d), -g).reshape(N, 6)
            trial = np.array([retract(self.x[k], delta[k]) for k in range(N)])
            c_new = self.cost(trial)
            if c_new < cost:
                rel = (cost - c_new) / cost
                self.x = trial
                out["accepted"] += 1
                lam = max(lam / 10.0, LAMBDA_MIN)
                H, g, cost = self.normal_equations()
                if rel < cfg["rel_cost_tol"]:
                    break
            else:
                lam *= 10.0
                if lam > LAMBDA_MAX:
                    break
        out.update(final_cost=cost, lam=lam, gradient=float(np.max(np.abs(g))) if N else 0.0)
        return out


# ---------------------------------------------------------------------------- PointTypePose helper
def key_pose_6d(T):
    """(x, y, z, roll, pitch, yaw) with get_transform_matrix(x, y, z, roll, pitch, yaw) == T:
    getTransformMatrix (:152-165) builds Rz(roll) Ry(pitch) Rx(yaw) from the stored angles."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    return (T[0, 3], T[1, 3], T[2, 3], math.atan2(R[1, 0], R[0, 0]), math.asin(max(-1.0, min(1.0, -R[2, 0]))),
            math.atan2(R[2, 1], R[2, 2]))
