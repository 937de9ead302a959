"""Synthetic inputs of the Scan Context tests (the reference ships no data): a there-and-back drive
of the synthetic corridor and a hand-seeded cloud that holds every special case of makeScancontext."""
from __future__ import annotations

import math

import numpy as np

# points on the four axes and the diagonals: sectors 15, 30, 45, 60 and 8, 23, 38, 53 at 60 sectors
AXES_AND_DIAGONALS = [[0, 10, 0, 0], [-10, 0, 0, 0], [0, -10, 0, 0], [10, -1e-6, 0, 0],  # 90, 180, 270, 360 deg
                      [7, 7, 0, 0], [-7, 7, 0, 0], [-7, -7, 0, 0], [7, -7, 0, 0]]           # 45, 135, 225, 315 deg

N_OUT = 60  # keyframes of the outbound leg; the return leg revisits them in reverse


def drive_pose(synth, j):
    """Pose of keyframe j < 2 N_OUT: out over ground_truth_pose(8 j), then back over the same poses
    reversed, turned by pi and offset by (0.2, -0.1) m."""
    if j < N_OUT:
        return synth.ground_truth_pose(8 * j)
    p = synth.ground_truth_pose(8 * (2 * N_OUT - 1 - j))
    return synth.Pose(x=p.x + 0.2, y=p.y - 0.1, yaw=p.yaw + math.pi)


def there_and_back(synth, n_scans=16, width=256):
    """(2 N_OUT, n_scans, width, 4) float32 scans of the drive."""
    return np.stack([synth.make_scan(j, n_scans, width, pose=drive_pose(synth, j)) for j in range(2 * N_OUT)])


def tricky_cloud(seed=5):
    """5,000 random points in +-100 m (some beyond max_radius), heights in +-5, 50 duplicated points,
    a NaN height, a NaN x, a NaN y, the axis and diagonal points, -0.0 coordinates, dropouts."""
    rng = np.random.default_rng(seed)
    p = np.zeros((5000, 4), np.float32)
    p[:, :2] = rng.uniform(-100, 100, (5000, 2))
    p[:, 2] = rng.uniform(-5, 5, 5000)
    p[:, 3] = rng.uniform(0, 255, 5000)
    dup = p[rng.integers(0, 5000, 50)].copy()
    dup[::2, 2] += 1.0  # same bin, another height
    special = np.array(AXES_AND_DIAGONALS + [
        [3.0, 4.0, np.nan, 0], [np.nan, 4.0, 9.0, 0], [3.0, np.nan, 9.0, 0],
        [-0.0, 5.0, 1.0, 0], [5.0, -0.0, 1.0, 0], [-0.0, -0.0, 0.5, 0], [-0.0, -5.0, 1.0, 0], [0.0, -5.0, 1.0, 0],
        [0, 0, 0, 0], [0, 0, 0, 0],
        [80.0, 0, 4.0, 0], [np.nextafter(np.float32(80.0), np.float32(np.inf)), 0, 400.0, 0],
        [20.0, 20.0, -1002.0, 0], [np.inf, 1.0, 50.0, 0], [1.0, 1.0, -np.inf, 0]], np.float32)
    out = np.concatenate([p, dup, special])
    return out[rng.permutation(out.shape[0])]
