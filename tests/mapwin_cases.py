"""Inputs of the sliding-window tests (test_mapwin_cpu.py checks the properties the GPU cases rely
on; test_gpu_mapwin.py runs them on the device).  Everything is constructed: no recorded data."""
from __future__ import annotations

import numpy as np

MAX_SUM = 32 * 255 * 255  # 2,080,800

# lislam_mapwin_match: three keyframes of different sizes per call, every nt of the list once
MATCH_WINDOWS = ((0, 63, 257), (1, 64, 256), (65, 255, 0))
MATCH_NQ = (1, 64, 300)

# (nq, nt): M > 100 (:309), G > 50 and nt != nq (:327) on both sides of each boundary
SELECT_CASES = ((100, 150), (101, 150), (250, 300), (251, 300), (300, 300), (299, 300))


def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def noisy(rng, desc, nbytes=3, amp=4):
    """A near-duplicate of every row: nbytes bytes moved by up to +-amp."""
    d = desc.astype(np.int32)
    for i in range(len(d)):
        at = rng.choice(32, nbytes, replace=False)
        d[i, at] += rng.integers(-amp, amp + 1, nbytes)
    return np.clip(d, 0, 255).astype(np.uint8)


def match_case(nq, nts, seed=0):
    """(query descriptors, [train descriptors per keyframe, oldest first]): random rows, near-duplicates of
    queries, exact duplicates of one train row (the first index must win)."""
    rng = np.random.default_rng(1000 + seed)
    q = random_desc(rng, nq)
    trains = []
    for nt in nts:
        t = random_desc(rng, nt)
        if nt >= 1:  # near-duplicates of random queries
            at = rng.choice(nt, max(1, nt // 3), replace=False)
            t[at] = noisy(rng, q[rng.integers(0, nq, len(at))])
        if nt >= 8:  # rows 2, 5 and nt - 1 are one row, an exact copy of query 0
            t[2] = q[0]
            t[5] = q[0]
            t[nt - 1] = q[0]
        trains.append(t)
    return q, trains


def extreme_case():
    """Query 0 is all 0, query 1 all 255.  Keyframe A holds one all-255 row: query 0 meets the maximum
    sum.  Keyframe B holds 255, 0, 0, 255 rows: the first of the equal rows wins."""
    q = np.zeros((2, 32), np.uint8)
    q[1] = 255
    a = np.full((1, 32), 255, np.uint8)
    b = np.zeros((4, 32), np.uint8)
    b[0] = 255
    b[3] = 255
    return q, [a, b]


def select_case(nq, nt, seed=0):
    """One keyframe whose row 0 is all 0 and whose other rows are far away (bytes >= 128); query i has
    i % 4 bytes of 1, so its match is row 0 at the integer sum i % 4: a quarter of the queries share each
    sum, and the G-th place falls inside a run of equal sums.  Points coincide (all pass the gate).
    Returns (desc, p3d, pose) of the current keyframe and of the window keyframe."""
    rng = np.random.default_rng(2000 + seed)
    t = rng.integers(128, 256, (nt, 32), dtype=np.uint8)
    t[0] = 0
    q = np.zeros((nq, 32), np.uint8)
    for i in range(nq):
        q[i, : i % 4] = 1
    pt = np.zeros((nt, 4), np.float32)
    pt[:, :3] = rng.uniform(-20, 20, (nt, 3))
    pq = np.zeros((nq, 4), np.float32)
    pq[:, :3] = pt[0, :3] + rng.uniform(-0.05, 0.05, (nq, 3)).astype(np.float32)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    return (q, pq, ident), (t, pt, ident)


def _quat(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = 0.5 * np.radians(deg)
    return np.concatenate([np.sin(h) * a, [np.cos(h)]])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def observe(pose, world, rng, sigma=0.01):
    """Sensor-frame float32 (n, 4) observations of world points from `pose` with Gaussian noise."""
    R = _rot(pose[:4])
    p = (world - pose[4:]) @ R + rng.normal(0, sigma, world.shape)
    out = np.zeros((len(world), 4), np.float32)
    out[:, :3] = p
    return out


def records_case():
    """400 landmarks seen from a current pose and from three window keyframes (350, 400 and 380 of
    them: the 400 one has nt == nq and is not used) with centimetre noise.  The first 24 landmarks carry
    exact descriptor copies, so they lead the sorted matches, and are planted outliers: displaced by
    0.2 m (inside the gate) or 0.4 m (outside) in the current keyframe (0-11) or in the window keyframes
    (12-23).  Returns ((desc, p3d, pose) current, [(desc, p3d, pose)] window, oldest first)."""
    rng = np.random.default_rng(3000)
    n = 400
    world = np.concatenate([rng.uniform(0, 40, (n, 1)), rng.uniform(-8, 8, (n, 1)), rng.uniform(-1, 3, (n, 1))], axis=1)
    base = random_desc(rng, n)
    poses = [np.concatenate([_quat((0, 0, 1), 2.0), [1.0, 0.1, 0.0]]),
             np.concatenate([_quat((0, 0.1, 1), -3.0), [2.0, -0.1, 0.02]]),
             np.concatenate([_quat((0.1, 0, 1), 4.0), [3.0, 0.2, -0.01]])]
    cur_pose = np.concatenate([_quat((0.05, 0.05, 1), 5.0), [4.0, 0.0, 0.0]])
    subsets = [np.arange(0, 350), np.arange(0, 400), np.arange(0, 380)]

    def shifted(idx, at, rng_):
        w = world[idx].copy()
        for i in at:
            d = rng_.normal(size=3)
            w[i] += d / np.linalg.norm(d) * (0.2 if i % 2 == 0 else 0.4)
        return w

    cur_desc = noisy(rng, base)
    cur_desc[:24] = base[:24]
    cur = (cur_desc, observe(cur_pose, shifted(np.arange(n), range(0, 12), rng), rng), cur_pose)
    window = []
    for pose, idx in zip(poses, subsets):
        d = noisy(rng, base[idx])
        d[:24] = base[:24]
        window.append((d, observe(pose, shifted(idx, range(12, 24), rng), rng), pose))
    return cur, window


DRIVE_FRAMES = 6
DRIVE_WINDOW = 3
DRIVE_BAD_FRAME = 4  # its odometry is far off: the solve must not converge (test_mapwin_cpu checks)


def drive_case(synth):
    """A 6-frame drive: synthetic ground clouds and drifting odometry as test_gpu_map's
    test_mapopt_sequence, constructed features (landmarks along the corridor seen with centimetre noise,
    a different number per frame) and one frame whose odometry is far off.
    Returns a list of (ground (n, 4), odom (7,), (desc, p3d))."""
    rng = np.random.default_rng(4000)
    n = 700
    world = np.concatenate([rng.uniform(-2, 25, (n, 1)), rng.uniform(-4, 4, (n, 1)), rng.uniform(-1, 2.5, (n, 1))], axis=1)
    base = random_desc(rng, n)
    frames = []
    for k in range(DRIVE_FRAMES):
        scan = synth.make_scan(k).reshape(-1, 4)
        ground = np.ascontiguousarray(scan[np.abs(scan[:, :3]).sum(1) > 0], np.float32)
        q, t = synth.ground_truth_pose(k).as_qt()
        odom = synth.perturb_pose(q, t, 0.02, 0.2, seed=10 + k)
        if k == DRIVE_BAD_FRAME:
            odom = synth.perturb_pose(q, t, 1.5, 12.0, seed=10 + k)
        nk = 420 + 37 * k
        idx = rng.permutation(n)[:nk]
        truth = np.concatenate([q, t])
        frames.append((ground, odom, (noisy(rng, base[idx]), observe(truth, world[idx], rng))))
    return frames


def map_filter_track(track, keep_xyz):
    """The cloud_track on which the feature tracker's filter (|x| < 0.01 drops) decides as
    mapOptimization's does on `track`: x = 1 wherever the three-axis test keeps the point."""
    t = np.array(track, np.float32).reshape(-1, 4).copy()
    t[keep_xyz.reshape(-1), 0] = 1.0
    return t
