"""Cases shared by the oracle-side and the GPU tests of the batched loop verification
(lislam_loop_verify): a pool of 12 corridor keyframes at 16 x 256 plus degenerate clouds, the
per-keyframe poses, and per ICP configuration one list of candidates that goes through ONE
verify_loops call.  Everything here is host data and the CPU oracle; nothing needs a GPU."""
from __future__ import annotations

import numpy as np

from loop_cases import drift, pose_T, random_room

N_CORRIDOR = 12
EMPTY, TINY, NAN_X, ROOM, CUBE = 12, 13, 14, 15, 16  # the extra keyframes' ids
POOL_SIZE = 17

# the drift of a current keyframe's pose, by keyframe id (T_kf has one row per keyframe, so two
# candidates with the same current keyframe share its drift)
DRIFTS = {11: (0.3, -0.2, 0.05, 2.0, 0.5), 10: (1.0, 0.4, 0.0, -5.0, 0.0), 9: (0.1, 0.0, 0.0, 0.5, 0.0)}


def submap_ids(cur, loop, w=1):
    """getSubmapOfhistory (intensity_feature_tracker.cpp:174-193) when keyframe cur was the newest:
    for i = -w..w: idx = loop + i; skipped unless 0 <= idx < keyframe_pool_.size() (= cur + 1)."""
    out = []
    for i in range(-w, w + 1):
        idx = loop + i
        if idx < 0 or idx >= cur + 1:
            continue
        out.append(idx)
    return out


def voxel_overflows(cloud, voxel_size):
    """pcl::VoxelGrid::applyFilter's own rule (voxel_grid.hpp:241-250) on the finite points: the
    leaf is too small when dx * dy * dz > INT_MAX, d = int64((max - min) * inverse_leaf) + 1 in float."""
    p = cloud[np.isfinite(cloud[:, :3]).all(1), :3].astype(np.float32)
    inv = np.float32(1.0) / np.float32(voxel_size)
    d = [int(np.int64((p[:, a].max() - p[:, a].min()) * inv)) + 1 for a in range(3)]
    return d[0] * d[1] * d[2] > 2**31 - 1


_POOL = None


def pool_clouds(synth):
    """The 17 keyframe clouds (built once, never modified)."""
    global _POOL
    if _POOL is None:
        clouds = [synth.make_scan(k, 16, 256).reshape(-1, 4) for k in range(N_CORRIDOR)]
        clouds.append(np.zeros((0, 4), np.float32))                  # EMPTY
        clouds.append(clouds[3][100:108].copy())                      # TINY: 8 points
        nan = clouds[5].copy()
        nan[:, 0] = np.nan
        clouds.append(nan)                                            # NAN_X
        rng = np.random.default_rng(3)
        clouds.append(random_room(rng, 1500))                         # ROOM
        cube = (rng.random((600, 4)) * [0.9, 0.9, 0.9, 255.0]).astype(np.float32)
        clouds.append(np.repeat(cube, 2, axis=0))                     # CUBE: every point twice, < 1 m
        for c in clouds:
            c.setflags(write=False)
        _POOL = clouds
    return _POOL


def keyframe_poses(synth):
    """T_kf (POOL_SIZE, 4, 4): ground truth for the corridor keyframes, the DRIFTS on top for 9, 10
    and 11, identity for the extra clouds."""
    T = np.stack([np.eye(4)] * POOL_SIZE)
    for k in range(N_CORRIDOR):
        T[k] = pose_T(synth.ground_truth_pose(k))
        if k in DRIFTS:
            T[k] = drift(*DRIFTS[k]) @ T[k]
    return T


DEFAULT_CANDIDATES = [(11, 0), (10, 3), (9, 8), (11, 10)]

# (name, IcpConfig fields, submap_window, candidates); loop = -1 entries are "no candidate" rows
CONFIGS = [
    ("default", {}, 1, [(11, 0), (7, -1), (10, 3), (9, 8), (11, -1), (11, 10), (10, 3)]),
    ("max_iterations", dict(max_iterations=3), 1, [(11, 0), (10, 3)]),
    ("max_distance", dict(max_correspondence_distance=0.001), 1, [(11, 0), (9, 8)]),
    ("fitness", dict(fitness_threshold=1e-4), 1, [(11, 0), (10, 3)]),
    ("no_downsample", dict(use_downsample=False), 1, [(10, 3), (9, 8)]),
    ("crop", dict(use_crop=True, crop_size=6.0), 1, [(11, 0), (10, 3), (9, 8)]),
    ("window0", {}, 0, [(11, 0), (10, 3), (11, 11)]),
    ("window2", {}, 2, [(10, 3), (11, 10), (9, 1)]),
    # window 0, so that a degenerate cloud is the whole submap
    ("degenerate", {}, 0, [(ROOM, EMPTY), (11, 0), (ROOM, NAN_X), (TINY, 3), (ROOM, ROOM), (CUBE, -1), (NAN_X, 3)]),
]


def mixed_overflow_config(synth):
    """One voxel size under which, by voxel_overflows, the doubled-points cube does not overflow
    (VoxelGrid halves it) and a corridor keyframe under its pose does (it passes unchanged)."""
    clouds, T = pool_clouds(synth), keyframe_poses(synth)

    def posed(i):
        c = clouds[i].copy()
        c[:, :3] = (c[:, :3].astype(np.float64) @ T[i][:3, :3].T + T[i][:3, 3]).astype(np.float32)
        return c

    for v in (1e-3, 5e-4, 2e-4, 1e-4, 5e-5):
        if not voxel_overflows(posed(CUBE), v) and voxel_overflows(posed(8), v) and voxel_overflows(posed(7), v):
            return ("mixed_overflow", dict(voxel_size=v), 0, [(CUBE, CUBE), (8, 8), (8, 7)])
    raise AssertionError("no voxel size separates the cube from the corridor")


def all_configs(synth):
    return CONFIGS + [mixed_overflow_config(synth)]


def oracle_rows(oracle, synth, cfg_kw, window, candidates):
    """What the single path gives per candidate: oracle.loop_icp on its submap (None for loop < 0)."""
    clouds, T = pool_clouds(synth), keyframe_poses(synth)
    rows = []
    for cur, loop in candidates:
        if loop < 0:
            rows.append(None)
            continue
        ids = submap_ids(cur, loop, window)
        rows.append(oracle.loop_icp(clouds[cur], T[cur], [clouds[i] for i in ids], [T[i] for i in ids],
                                    oracle.IcpConfig(**cfg_kw)))
    return rows


_ROWS = {}


def cached_oracle_rows(oracle, synth, name):
    """oracle_rows of the named configuration, computed once per process."""
    if name not in _ROWS:
        _, kw, w, cands = next(c for c in all_configs(synth) if c[0] == name)
        _ROWS[name] = oracle_rows(oracle, synth, kw, w, cands)
    return _ROWS[name]
