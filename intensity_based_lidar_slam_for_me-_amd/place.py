"""Scan Context place recognition over the lislam C ABI: the reference's ``SCManager``
(``include/Scancontext.h``, ``src/Scancontext.cpp``) as a device-resident database.

``ScanContext.make_and_save_and_detect`` plays the ``USE_SCANCONTEXT`` block of
``loopClosureHandler::keyframeProcessor`` (``src/loop_closure_handler.cpp:99-105``); ``add_batch``
describes the scans of an extracted batch straight from its device ``cloud_track`` and ``detect``
replays ``detectLoopClosureID`` for a whole range of keyframes in one launch.  ``(loop_id, yaw)``
is what ``loop.loop_closure_icp`` takes as its history keyframe and initial yaw.  All compute runs
in ``liblislam.so`` on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import native as nat

PlaceConfig = nat.PlaceConfig


class Detection(NamedTuple):
    loop_id: np.ndarray   # (n,) int32, -1 = no loop
    yaw: np.ndarray       # (n,) float32, deg2rad(nn_align * 360 / num_sector)
    min_dist: np.ndarray  # (n,) float64
    nn_idx: np.ndarray    # (n,) int32
    nn_align: np.ndarray  # (n,) int32


class ScanContext:
    """``SCManager`` with its descriptors and keys on the device; ``config`` = the fields of
    ``PlaceConfig`` (defaults: Scancontext.h:77-96)."""

    def __init__(self, ctx, capacity: int = 4096, **config):
        self.ctx = ctx
        self.cfg = PlaceConfig(**config)
        h = ctypes.c_void_p()
        nat.check(ctx.lib.lislam_place_create(ctx.h, ctypes.byref(self.cfg), int(capacity), ctypes.byref(h)), ctx.h,
                  "lislam_place_create")
        self.h = h

    def close(self):
        if self.h:
            self.ctx.lib.lislam_place_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_place_size(self.h, ctypes.byref(n)), self.ctx.h, "lislam_place_size")
        return n.value

    def add(self, clouds) -> None:
        """makeAndSaveScancontextAndKeys of each cloud ((n, 4) float32 x, y, z, intensity) of the list."""
        cs = [np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in clouds]
        if not cs:
            return
        counts = np.array([c.shape[0] for c in cs], np.int32)
        pts = np.ascontiguousarray(np.concatenate(cs))
        nat.check(self.ctx.lib.lislam_place_add_clouds(self.h, nat.ptr(pts) if pts.size else None, nat.ptr(counts), len(cs)),
                  self.ctx.h, "lislam_place_add_clouds")

    def add_batch(self, batch, first: int, n: int) -> None:
        """The same for cloud_track of scans [first, first + n) of an extracted batch, on the device."""
        nat.check(self.ctx.lib.lislam_place_add_batch(self.h, batch.h, int(first), int(n)), self.ctx.h,
                  "lislam_place_add_batch")

    def add_batch_scans(self, batch, scans) -> None:
        """The listed scans of an extracted batch (any order, repeats allowed) in one set of launches: what
        ``add_batch(batch, s, 1)`` for every s in ``scans`` would leave."""
        s = np.ascontiguousarray(np.atleast_1d(scans), np.int32).reshape(-1)
        nat.check(self.ctx.lib.lislam_place_add_batch_scans(self.h, batch.h, nat.ptr(s) if s.size else None, s.shape[0]),
                  self.ctx.h, "lislam_place_add_batch_scans")

    def detect(self, first: int | None = None, n: int | None = None) -> Detection:
        """detectLoopClosureID as it returned when keyframe k was the newest, k in [first, first + n)
        (default: every keyframe)."""
        first = 0 if first is None else int(first)
        n = len(self) - first if n is None else int(n)
        out = Detection(np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.float32), np.zeros(max(n, 0), np.float64),
                        np.zeros(max(n, 0), np.int32), np.zeros(max(n, 0), np.int32))
        nat.check(self.ctx.lib.lislam_place_detect(self.h, first, n, *(nat.ptr(a) for a in out)), self.ctx.h,
                  "lislam_place_detect")
        return out

    def make_and_save_and_detect(self, cloud):
        """keyframeProcessor's USE_SCANCONTEXT block for one keyframe -> (loop_id, yaw)."""
        self.add([cloud])
        d = self.detect(len(self) - 1, 1)
        return int(d.loop_id[0]), d.yaw[0]

    def distance(self, a, b):
        """distanceBtnScanContext(desc[a[k]], desc[b[k]]) -> (dist (n,) float64, shift (n,) int32)."""
        ia = np.ascontiguousarray(np.atleast_1d(a), np.int32)
        ib = np.ascontiguousarray(np.atleast_1d(b), np.int32)
        if ia.shape != ib.shape:
            raise ValueError("a and b must hold the same number of indices")
        dist = np.zeros(ia.shape[0], np.float64)
        shift = np.zeros(ia.shape[0], np.int32)
        nat.check(self.ctx.lib.lislam_place_distance(self.h, nat.ptr(ia), nat.ptr(ib), ia.shape[0], nat.ptr(dist),
                                                     nat.ptr(shift)), self.ctx.h, "lislam_place_distance")
        return dist, shift

    def _download(self, what, index, count, dtype):
        buf = np.zeros(count, dtype)
        n = ctypes.c_int32()
        nat.check(self.ctx.lib.lislam_place_download(self.h, what, int(index), nat.ptr(buf), count, ctypes.byref(n)),
                  self.ctx.h, "lislam_place_download")
        return buf[:n.value]

    def descriptor(self, i: int) -> np.ndarray:
        """(num_ring, num_sector) float64."""
        R, S = self.cfg.num_ring, self.cfg.num_sector
        return self._download(nat.PLACE_DESC, i, R * S, np.float64).reshape(R, S)

    def ring_key(self, i: int) -> np.ndarray:
        return self._download(nat.PLACE_RING_KEY, i, self.cfg.num_ring, np.float32)

    def sector_key(self, i: int) -> np.ndarray:
        return self._download(nat.PLACE_SECTOR_KEY, i, self.cfg.num_sector, np.float64)
