"""The loop-closure back end over a stream of scans: ``feature_tracker::loopClosureThread`` and
``factorGraphThread`` (``src/intensity_feature_tracker.cpp:196-392``, ``:395-583``) driven from
``getKeyframe``'s selection (``:741-815``), every stage one call into ``liblislam.so``.

``LoopBackend.step`` runs, for scans [first, first + n) of a batch: select the keyframes
(``KeyframeSelector.step_batch``), feed the keyframe pool, the loop detector and the pose graph from
the selected scans only (the ``add_batch_scans`` list feeds), detect loops for the new keyframes,
verify the candidates (``keyframes.close_loops``) and optimise the graph when a loop factor was
accepted.  All compute runs on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .keyframes import close_loops
from .loop import ACCEPTED, IcpConfig


class BackendStep(NamedTuple):
    keyframe_id: np.ndarray  # (n,) int32, -1 = not a keyframe
    T_s2m: np.ndarray        # (n, 4, 4)
    nodes: np.ndarray        # (k, 26) FactorGraphNode rows of the k selected scans
    scans: np.ndarray        # (k,) int32 the selected scans of the batch
    detection: object        # the detector's Detection for the k new keyframes (None when k == 0)
    T_icp: np.ndarray        # (k, 4, 4) close_loops' outputs, one row per new keyframe
    T_cur2map: np.ndarray    # (k, 4, 4)
    fitness: np.ndarray      # (k,)
    info: np.ndarray         # (k, 8)
    summary: object          # posegraph.Summary, None when the optimiser did not run


class LoopBackend:
    """``selector``: a ``KeyframeSelector``; ``pool``: a ``KeyframePool``; ``detector``: a ``BowDatabase`` or a
    ``ScanContext`` (anything with ``add_batch_scans``, ``detect(first, n).loop_id`` and ``len``);
    ``pose_graph``: a ``PoseGraph``.  The three containers must hold the same keyframes: entry i of each is
    keyframe i.

    One deviation from the reference: the candidates of one step are all verified at the poses the
    graph held when the step began, and the graph is optimised once, after the step's loop factors are
    in.  The reference verifies and updates per keyframe; steps of one keyframe give its order."""

    def __init__(self, ctx, selector, pool, detector, pose_graph, icp_cfg: IcpConfig | None = None, robust: bool = False):
        self.ctx = ctx
        self.selector, self.pool, self.detector, self.pose_graph = selector, pool, detector, pose_graph
        self.icp_cfg = icp_cfg
        self.robust = bool(robust)

    def _sizes(self):
        return len(self.pool), len(self.detector), len(self.pose_graph)

    def step(self, batch, first: int, n: int, times, poses=None) -> BackendStep:
        """Scans [first, first + n) of ``batch`` (extracted, odometry and intensity_odometry run), ``times`` (n,)
        their stamps.  ``poses`` (scans of the batch, 7), numpy or a float64 torch device tensor: the trajectory
        the pose graph takes its nodes and odometry edges from, row s = scan s of the batch; None = the batch's
        OUT_POSE rows (which start at the identity with every batch: a stream over several batches passes a
        continuous trajectory)."""
        k0 = len(self.pool)
        assert self._sizes() == (k0, k0, k0), f"pool, detector and graph hold {self._sizes()} keyframes"
        ids, T_s2m, nodes = self.selector.step_batch(batch, first, n, times)
        scans = (int(first) + np.flatnonzero(ids >= 0)).astype(np.int32)
        k = scans.shape[0]
        if k == 0:
            return BackendStep(ids, T_s2m, nodes, scans, None, np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), np.zeros(0),
                               np.zeros((0, 8), np.int32), None)
        self.pool.add_batch_scans(batch, scans)
        self.detector.add_batch_scans(batch, scans)
        if poses is None:
            self.pose_graph.add_batch_scans(batch, scans)
        else:
            self.pose_graph.add_keyframes(poses, scans)
        if k0 == 0:  # the prior on the first keyframe ever (:444-455)
            self.pose_graph.set_prior(0, self.pose_graph.poses(0, 1)[0])
        assert self._sizes() == (k0 + k,) * 3, f"pool, detector and graph hold {self._sizes()} keyframes"
        det = self.detector.detect(k0, k)
        cur = np.arange(k0, k0 + k, dtype=np.int32)
        T_icp, T_c2m, fit, info = close_loops(self.pool, self.pose_graph, cur, det.loop_id, self.icp_cfg, self.robust)
        summary = self.pose_graph.optimize() if np.any(info[:, 0] == ACCEPTED) else None
        return BackendStep(ids, T_s2m, nodes, scans, det, T_icp, T_c2m, fit, info, summary)
