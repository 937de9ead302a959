"""Pose-graph optimization over the lislam C ABI (``lislam_pgo_*``): the factor graph that
``feature_tracker::mapOdomHandle`` and ``loopClosureThread`` keep
(``src/intensity_feature_tracker.cpp:395-583``, ``:314-381``) -- a prior on the first keyframe, a
``BetweenFactor<Pose3>`` per consecutive keyframe pair and one per accepted ICP loop -- held on the
device and solved in batch, and ``updatePoses`` (``:110-145``), which writes the corrected keyframe
poses back for ``getTransformMatrix``.

The optimizer is Levenberg-Marquardt on the whole graph: it replaces iSAM2's incremental update with
the batch optimum of the same factors.  Poses are 7 doubles ``qx qy qz qw tx ty tz``; variances are
GTSAM's ``Variances(Vector6)``: rad^2 x 3, then m^2 x 3.  All compute runs in ``liblislam.so`` on the
GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np

from . import native as nat

PgoConfig = nat.PgoConfig
ODOMETRY_VARIANCES = (1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6)  # odometryNoise_ and priorNoise_ (:41-44)
STATUS = ("converged", "lambda_limit", "max_iterations")


class Linearization(NamedTuple):
    residual: np.ndarray  # (E + 1, 6) whitened, the prior last
    J_from: np.ndarray    # (E, 6, 6)
    J_to: np.ndarray      # (E + 1, 6, 6)
    weight: np.ndarray    # (E + 1,)
    cost: float


class Summary(NamedTuple):
    status: int
    iterations: int
    accepted: int
    cg_iterations: int
    cg_most: int
    nodes: int
    edges: int
    initial_cost: float
    final_cost: float
    lam: float
    cg_relres: float
    stats: np.ndarray  # the four doubles as the library wrote them


def matrix_to_pose(T) -> np.ndarray:
    """Row-major 4x4 -> qx qy qz qw tx ty tz (Shepperd's method)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3]
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
    q = np.array(q)
    return np.concatenate([q / np.linalg.norm(q), T[:3, 3]])


def key_pose_6d(T):
    """(x, y, z, roll, pitch, yaw) of a 4x4 pose such that ``loop.get_transform_matrix`` of it is the
    pose again: getTransformMatrix (:152-165) builds RzRyRx(yaw, pitch, roll) = Rz(roll) Ry(pitch)
    Rx(yaw) from a PointTypePose, so roll is the angle about z and yaw the one about x.  The
    reference's own eulerAngles(2, 1, 0) insertion (:433-462) is not replayed.  |pitch| < pi / 2."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3]
    return (float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), math.atan2(R[1, 0], R[0, 0]),
            math.asin(max(-1.0, min(1.0, -R[2, 0]))), math.atan2(R[2, 1], R[2, 2]))


class PoseGraph:
    """The keyframe pose graph on the device; ``config`` = the fields of ``PgoConfig``."""

    def __init__(self, ctx, node_capacity: int = 4096, edge_capacity: int = 8192, **config):
        self.ctx = ctx
        self.cfg = PgoConfig(**config)
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_pgo_create(ctx.h, ctypes.byref(self.cfg), int(node_capacity), int(edge_capacity),
                                            ctypes.byref(h)), ctx.h, "lislam_pgo_create")
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:  # the graph holds its context's stream: once the context is closed it can only be dropped
                self.ctx.lib.lislam_pgo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """(nodes, edges)."""
        n, e = ctypes.c_int32(), ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_pgo_size(self.h, ctypes.byref(n), ctypes.byref(e)), self.ctx.h, "lislam_pgo_size")
        return n.value, e.value

    def __len__(self) -> int:
        return self.size()[0]

    def add_nodes(self, poses) -> None:
        """Nodes with consecutive ids; poses (n, 7) = their initial estimates."""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        nat.check(self.ctx.lib.lislam_pgo_add_nodes(self.h, nat.ptr(p), p.shape[0]), self.ctx.h, "lislam_pgo_add_nodes")

    def set_prior(self, node: int, pose, variances=ODOMETRY_VARIANCES) -> None:
        """PriorFactor<Pose3> (:444-455); the default variances are priorNoise_."""
        p = np.ascontiguousarray(pose, np.float64).reshape(7)
        v = np.ascontiguousarray(variances, np.float64).reshape(6)
        nat.check(self.ctx.lib.lislam_pgo_set_prior(self.h, int(node), nat.ptr(p), nat.ptr(v)), self.ctx.h,
                  "lislam_pgo_set_prior")

    def add_edges(self, frm, to, meas, variances, robust=None) -> None:
        """n between factors: ids (n,), meas (n, 7), variances (n, 6) or (6,), robust (n,) bool."""
        i = np.ascontiguousarray(np.atleast_1d(frm), np.int32)
        j = np.ascontiguousarray(np.atleast_1d(to), np.int32)
        z = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(variances, np.float64), (i.shape[0], 6)))
        r = np.zeros(i.shape[0], np.int32) if robust is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(robust), i.shape).astype(np.int32))
        if not (i.shape == j.shape and z.shape[0] == i.shape[0]):
            raise ValueError("from, to and meas must hold the same number of edges")
        nat.check(self.ctx.lib.lislam_pgo_add_edges(self.h, nat.ptr(i), nat.ptr(j), nat.ptr(z), nat.ptr(v), nat.ptr(r),
                                                    i.shape[0]), self.ctx.h, "lislam_pgo_add_edges")

    def add_odometry(self, first: int, meas, variances=ODOMETRY_VARIANCES) -> None:
        """mapOdomHandle's BetweenFactor (:492-497) for the consecutive pairs (first + k, first + k + 1):
        meas (n, 7) = pose_from.between(pose_to); the default variances are odometryNoise_."""
        z = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
        ids = np.arange(int(first), int(first) + z.shape[0], dtype=np.int32)
        self.add_edges(ids, ids + 1, z, variances)

    def add_loop(self, cur: int, loop: int, T_cur2map, T_loop2map, fitness: float, robust: bool = False) -> None:
        """The loop factor of loopClosureThread (:316-360): pose_from = T_cur2map (loop_closure_icp's
        output), pose_to = the history keyframe's pose, measurement pose_from.between(pose_to), every
        variance = the ICP fitness score; robust wraps it in Cauchy(1) (:350-353)."""
        z = np.linalg.inv(np.asarray(T_cur2map, np.float64).reshape(4, 4)) @ np.asarray(T_loop2map, np.float64).reshape(4, 4)
        self.add_edges([cur], [loop], matrix_to_pose(z)[None], np.full(6, float(fitness)), [robust])

    def add_batch(self, batch, first: int, n: int, variances=None) -> None:
        """Nodes and odometry edges from the OUT_POSE rows of scans [first, first + n) of a batch, on the device."""
        v = None if variances is None else np.ascontiguousarray(variances, np.float64).reshape(6)
        nat.check(self.ctx.lib.lislam_pgo_add_batch(self.h, batch.h, int(first), int(n), None if v is None else nat.ptr(v)),
                  self.ctx.h, "lislam_pgo_add_batch")

    def add_keyframes(self, poses, index, variances=None) -> None:
        """mapOdomHandle (:395-514) for the keyframes ``index`` (strictly increasing) of one trajectory
        ``poses`` (n_poses, 7), a numpy array or a float64 torch device tensor: node k = poses[index[k]], edge
        (k - 1, k) = poses[index[k-1]]^-1 poses[index[k]].  On a graph that is not empty the first keyframe gets
        an edge from the last node, measured from the pose that node was added with."""
        idx = np.ascontiguousarray(np.atleast_1d(index), np.int32).reshape(-1)
        v = None if variances is None else np.ascontiguousarray(variances, np.float64).reshape(6)
        if hasattr(poses, "data_ptr"):
            if str(poses.dtype) != "torch.float64" or not poses.is_contiguous() or poses.numel() % 7:
                raise ValueError("poses must be a contiguous float64 tensor of (n_poses, 7)")
            keep, n_poses, pp = poses, poses.numel() // 7, ctypes.c_void_p(poses.data_ptr())
        else:
            keep = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
            n_poses, pp = keep.shape[0], nat.ptr(keep)
        nat.check(self.ctx.lib.lislam_pgo_add_keyframes(self.h, pp if n_poses else None, n_poses,
                                                        nat.ptr(idx) if idx.size else None, idx.shape[0],
                                                        None if v is None else nat.ptr(v)), self.ctx.h, "lislam_pgo_add_keyframes")

    def add_batch_scans(self, batch, scans, variances=None) -> None:
        """``add_keyframes`` with poses = the batch's OUT_POSE rows, read on the device.  OUT_POSE starts again
        at the identity with every batch: a stream over several batches goes through ``add_keyframes``."""
        s = np.ascontiguousarray(np.atleast_1d(scans), np.int32).reshape(-1)
        v = None if variances is None else np.ascontiguousarray(variances, np.float64).reshape(6)
        nat.check(self.ctx.lib.lislam_pgo_add_batch_scans(self.h, batch.h, nat.ptr(s) if s.size else None, s.shape[0],
                                                          None if v is None else nat.ptr(v)), self.ctx.h, "lislam_pgo_add_batch_scans")

    def edges(self, first: int = 0, n: int | None = None):
        """(from, to, meas (n, 7), variances (n, 6), robust) of edges [first, first + n)."""
        n = self.size()[1] - first if n is None else int(n)
        i, j, r = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        z, v = np.zeros((n, 7)), np.zeros((n, 6))
        nat.check(self.ctx.lib.lislam_pgo_edges(self.h, int(first), n, nat.ptr(i), nat.ptr(j), nat.ptr(z), nat.ptr(v),
                                                nat.ptr(r)), self.ctx.h, "lislam_pgo_edges")
        return i, j, z, v, r

    def linearize(self) -> Linearization:
        E = self.size()[1]
        r, Jf, Jt, w = np.zeros((E + 1, 6)), np.zeros((E, 6, 6)), np.zeros((E + 1, 6, 6)), np.zeros(E + 1)
        cost = np.zeros(1)
        nat.check(self.ctx.lib.lislam_pgo_linearize(self.h, nat.ptr(r), nat.ptr(Jf) if E else None, nat.ptr(Jt), nat.ptr(w),
                                                    nat.ptr(cost)), self.ctx.h, "lislam_pgo_linearize")
        return Linearization(r, Jf, Jt, w, float(cost[0]))

    def optimize(self) -> Summary:
        info = np.zeros(8, np.int32)
        stats = np.zeros(4)
        nat.check(self.ctx.lib.lislam_pgo_optimize(self.h, nat.ptr(info), nat.ptr(stats)), self.ctx.h, "lislam_pgo_optimize")
        return Summary(*(int(v) for v in info[:7]), *(float(v) for v in stats), stats)

    def poses(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """(n, 7) current estimates: updatePoses' isamCurrentEstimate_."""
        n = len(self) - first if n is None else int(n)
        out = np.zeros((n, 7))
        nat.check(self.ctx.lib.lislam_pgo_poses(self.h, int(first), n, nat.ptr(out), None), self.ctx.h, "lislam_pgo_poses")
        return out

    def key_poses_6d(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """(n, 6) float32 x, y, z, roll, pitch, yaw: cloudKeyPoses6D_ as ``loop.get_transform_matrix`` reads it."""
        n = len(self) - first if n is None else int(n)
        out = np.zeros((n, 6), np.float32)
        nat.check(self.ctx.lib.lislam_pgo_poses(self.h, int(first), n, None, nat.ptr(out)), self.ctx.h, "lislam_pgo_poses")
        return out
