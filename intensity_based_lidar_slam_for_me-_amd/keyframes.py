"""The keyframe clouds of the loop-closure back end on the device, and the ``USE_ICP`` block of
``feature_tracker::loopClosureThread`` (``src/intensity_feature_tracker.cpp:217-366``) for a whole
batch of loop candidates, over the lislam C ABI.

``KeyframePool`` is ``loopClosureProcessor_.keyframe_pool_[i].cloud_track_`` in HBM: keyframe ids
are consecutive from 0 in the order added.  ``KeyframePool.verify_loops`` verifies L candidates
``(cur, loop)`` -- e.g. the ``loop_id`` array of ``ScanContext.detect`` / ``BowDatabase.detect`` as it
comes, -1 entries included -- with one set of launches; every row equals what
``loop.loop_closure_icp`` returns for that candidate alone, bit for bit.  ``close_loops`` is the
block ``:216-363`` in one call: poses from the pose graph, verification, one loop factor per
accepted candidate.  All compute runs in ``liblislam.so`` on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as nat
from .loop import ACCEPTED, IcpConfig, get_transform_matrix

NO_CANDIDATE = -3  # info[0] of a candidate whose loop_id is negative


def submap_ids(cur: int, loop: int, window: int = 1) -> list[int]:
    """getSubmapOfhistory (:174-193) as it ran when keyframe ``cur`` was the newest."""
    return [i for i in range(max(0, loop - window), loop + window + 1) if i <= cur]


class KeyframePool:
    """Up to ``capacity`` keyframe clouds of ``point_capacity`` points in all, device resident."""

    def __init__(self, ctx, capacity: int = 4096, point_capacity: int = 1 << 24):
        self.ctx = ctx
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_keyframes_create(ctx.h, int(capacity), int(point_capacity), ctypes.byref(h)), ctx.h,
                  "lislam_keyframes_create")
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:
                self.ctx.lib.lislam_keyframes_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """(keyframes, points)."""
        n, p = ctypes.c_int32(), ctypes.c_int64()
        nat.check(self.ctx.lib.lislam_keyframes_size(self.h, ctypes.byref(n), ctypes.byref(p)), self.ctx.h,
                  "lislam_keyframes_size")
        return n.value, p.value

    def __len__(self) -> int:
        return self.size()[0]

    def add_clouds(self, clouds, counts=None) -> None:
        """``clouds``: a list of (n, 4) float32 host arrays (x, y, z, intensity), one keyframe each; or,
        with ``counts``, one array or torch device tensor holding ``sum(counts)`` points, cut into
        ``len(counts)`` keyframes (read where it lies)."""
        if counts is None:
            cs = [np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in clouds]
            if not cs:
                return
            cnt = np.array([c.shape[0] for c in cs], np.int32)
            pts = np.ascontiguousarray(np.concatenate(cs))
            p = nat.ptr(pts) if pts.size else None
        else:
            cnt = np.ascontiguousarray(counts, np.int32).reshape(-1)
            if hasattr(clouds, "data_ptr"):
                if str(clouds.dtype) != "torch.float32" or not clouds.is_contiguous() or clouds.numel() != 4 * int(cnt.sum()):
                    raise ValueError("clouds must be a contiguous float32 tensor of sum(counts) x 4")
                pts = clouds
                p = ctypes.c_void_p(clouds.data_ptr()) if clouds.numel() else None
            else:
                pts = np.ascontiguousarray(clouds, np.float32).reshape(-1, 4)
                if pts.shape[0] != int(cnt.sum()):
                    raise ValueError("clouds must hold sum(counts) points")
                p = nat.ptr(pts) if pts.size else None
        nat.check(self.ctx.lib.lislam_keyframes_add_clouds(self.h, p, nat.ptr(cnt), cnt.shape[0]), self.ctx.h,
                  "lislam_keyframes_add_clouds")

    def add_batch(self, batch, first: int, n: int) -> None:
        """cloud_track of scans [first, first + n) of an extracted batch, copied device to device."""
        nat.check(self.ctx.lib.lislam_keyframes_add_batch(self.h, batch.h, int(first), int(n)), self.ctx.h,
                  "lislam_keyframes_add_batch")

    def add_batch_scans(self, batch, scans) -> None:
        """cloud_track of the listed scans of an extracted batch (any order, repeats allowed), one gather
        launch: what ``add_batch(batch, s, 1)`` for every s in ``scans`` would leave."""
        s = np.ascontiguousarray(np.atleast_1d(scans), np.int32).reshape(-1)
        nat.check(self.ctx.lib.lislam_keyframes_add_batch_scans(self.h, batch.h, nat.ptr(s) if s.size else None, s.shape[0]),
                  self.ctx.h, "lislam_keyframes_add_batch_scans")

    def cloud(self, i: int) -> np.ndarray:
        """Keyframe i as (n, 4) float32."""
        n = ctypes.c_int32()
        rc = self.ctx.lib.lislam_keyframes_download(self.h, int(i), None, 0, ctypes.byref(n))
        if rc not in (nat.OK, nat.ERR_CAPACITY):
            nat.check(rc, self.ctx.h, "lislam_keyframes_download")
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            nat.check(self.ctx.lib.lislam_keyframes_download(self.h, int(i), nat.ptr(out), n.value, ctypes.byref(n)), self.ctx.h,
                      "lislam_keyframes_download")
        return out

    def verify_loops(self, cur_ids, loop_ids, T_kf, cfg: IcpConfig | None = None, submap_window: int = 1):
        """The USE_ICP block for the candidates ``(cur_ids[k], loop_ids[k])``; ``T_kf`` (pool size, 4, 4)
        = getTransformMatrix of every keyframe (a numpy array or a float64 torch device tensor).

        Returns ``(T_icp (L, 4, 4), T_cur2map (L, 4, 4), fitness (L,), info (L, 8))``, row k as
        ``loop.loop_closure_icp`` of candidate k on its submap ``submap_ids(cur, loop, submap_window)``;
        ``info[k, 0] == NO_CANDIDATE`` where ``loop_ids[k] < 0``."""
        cfg = cfg or IcpConfig()
        cur = np.ascontiguousarray(np.atleast_1d(cur_ids), np.int32)
        loop = np.ascontiguousarray(np.atleast_1d(loop_ids), np.int32)
        if cur.shape != loop.shape or cur.ndim != 1:
            raise ValueError("cur_ids and loop_ids must hold the same number of candidates")
        nk = len(self)
        if hasattr(T_kf, "data_ptr"):
            if str(T_kf.dtype) != "torch.float64" or not T_kf.is_contiguous() or T_kf.numel() != 16 * nk:
                raise ValueError("T_kf must be a contiguous float64 tensor of (pool size, 4, 4)")
            T, pT = T_kf, ctypes.c_void_p(T_kf.data_ptr())
        else:
            T = np.ascontiguousarray(T_kf, np.float64).reshape(-1, 16)
            if T.shape[0] != nk:
                raise ValueError("T_kf must hold one 4x4 pose per keyframe of the pool")
            pT = nat.ptr(T)
        L = cur.shape[0]
        T_icp, T_c2m = np.zeros((L, 4, 4)), np.zeros((L, 4, 4))
        fit, info = np.zeros(L), np.zeros((L, 8), np.int32)
        nat.check(self.ctx.lib.lislam_loop_verify(self.h, ctypes.byref(cfg), int(submap_window), nat.ptr(cur), nat.ptr(loop), L,
                                                  pT, nat.ptr(T_icp), nat.ptr(T_c2m), nat.ptr(fit), nat.ptr(info)),
                  self.ctx.h, "lislam_loop_verify")
        return T_icp, T_c2m, fit, info


class KeyframeSelector:
    """``feature_tracker::getKeyframe`` (``src/intensity_feature_tracker.cpp:741-815``) behind tfBroadcast's
    ``T_s2m = T_s2m * T_s2s`` (``:819``), its state on the device (``lislam_keysel_*``).  The reference's
    first branch (``cloudKeyPoses3D_->points.empty()``, filled by another thread) is taken exactly once
    here, by the first good frame.  Each step returns ``(keyframe_id (n,) int32 with -1 = not a keyframe,
    T_s2m (n, 4, 4), nodes (n_selected, 26))``; a node row is time, id, cur_position[3], prev_position[3],
    cur_rotation[9], prev_rotation[9] (``FactorGraphNode``, ``src/keyframe.h:115-121``)."""

    def __init__(self, ctx, time_interval: float = 0.3, distance_interval: float = 0.3):
        self.ctx = ctx
        self.cfg = nat.KeyselConfig(float(time_interval), float(distance_interval))
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_keysel_create(ctx.h, ctypes.byref(self.cfg), ctypes.byref(h)), ctx.h, "lislam_keysel_create")
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:
                self.ctx.lib.lislam_keysel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _out(n):
        return np.full(n, -1, np.int32), ctypes.c_int32(), np.zeros((n, 4, 4)), np.zeros((n, 26))

    def step(self, T_s2s, good, times):
        """n frames in stream order: ``T_s2s`` (n, 7) q x,y,z,w, t and ``good`` (n,) int32, each a numpy array
        or a contiguous torch device tensor (float64 / int32); ``times`` (n,) on the host."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        n = t.shape[0]
        if hasattr(T_s2s, "data_ptr"):
            if str(T_s2s.dtype) != "torch.float64" or not T_s2s.is_contiguous() or T_s2s.numel() != 7 * n:
                raise ValueError("T_s2s must be a contiguous float64 tensor of (n, 7)")
            kT, pT = T_s2s, ctypes.c_void_p(T_s2s.data_ptr())
        else:
            kT = np.ascontiguousarray(T_s2s, np.float64).reshape(-1, 7)
            if kT.shape[0] != n:
                raise ValueError("T_s2s must hold one row per time")
            pT = nat.ptr(kT)
        if hasattr(good, "data_ptr"):
            if str(good.dtype) != "torch.int32" or not good.is_contiguous() or good.numel() != n:
                raise ValueError("good must be a contiguous int32 tensor of (n,)")
            kg, pg = good, ctypes.c_void_p(good.data_ptr())
        else:
            kg = np.ascontiguousarray(good, np.int32).reshape(-1)
            if kg.shape[0] != n:
                raise ValueError("good must hold one flag per time")
            pg = nat.ptr(kg)
        ids, nsel, T, node = self._out(n)
        nat.check(self.ctx.lib.lislam_keysel_step(self.h, pT if n else None, pg if n else None, nat.ptr(t) if n else None, n,
                                                  nat.ptr(ids), ctypes.byref(nsel), nat.ptr(T), nat.ptr(node)), self.ctx.h,
                  "lislam_keysel_step")
        return ids, T, node[:nsel.value].copy()

    def step_batch(self, batch, first: int, n: int, times):
        """The same for scans [first, first + n) of a batch whose intensity_odometry has run: the OUT_ORB_T rows
        and OUT_ORB_STATS[0] == 1 are read on the device."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        if t.shape[0] != int(n):
            raise ValueError("times must hold one entry per scan")
        m = max(int(n), 0)
        ids, nsel, T, node = self._out(m)
        nat.check(self.ctx.lib.lislam_keysel_step_batch(self.h, batch.h, int(first), int(n), nat.ptr(t) if m else None,
                                                        nat.ptr(ids), ctypes.byref(nsel), nat.ptr(T), nat.ptr(node)), self.ctx.h,
                  "lislam_keysel_step_batch")
        return ids, T, node[:nsel.value].copy()

    def state(self):
        """(keyframes selected so far, T_s2m (4, 4), the last keyframe's time: NaN before the first)."""
        n, T, t = ctypes.c_int32(), np.zeros((4, 4)), np.zeros(1)
        nat.check(self.ctx.lib.lislam_keysel_state(self.h, ctypes.byref(n), nat.ptr(T), nat.ptr(t)), self.ctx.h,
                  "lislam_keysel_state")
        return n.value, T, float(t[0])


def close_loops(pool: KeyframePool, pose_graph, cur_ids, loop_ids, cfg: IcpConfig | None = None, robust: bool = False):
    """loopClosureThread's block :216-363 for a batch of candidates: the keyframe poses come from
    ``pose_graph.key_poses_6d()`` through ``loop.get_transform_matrix``, the candidates are verified
    in one ``verify_loops`` call, and every accepted one adds its loop factor
    (``pose_graph.add_loop``) in candidate order.  Returns verify_loops' outputs."""
    T_kf = np.stack([get_transform_matrix(*(float(v) for v in p)) for p in pose_graph.key_poses_6d(0, len(pool))])
    cur = np.atleast_1d(np.asarray(cur_ids, np.int32))
    loop = np.atleast_1d(np.asarray(loop_ids, np.int32))
    T_icp, T_c2m, fit, info = pool.verify_loops(cur, loop, T_kf, cfg)
    for k in range(cur.shape[0]):
        if info[k, 0] == ACCEPTED:
            pose_graph.add_loop(int(cur[k]), int(loop[k]), T_c2m[k], T_kf[loop[k]], float(fit[k]), robust)
    return T_icp, T_c2m, fit, info
