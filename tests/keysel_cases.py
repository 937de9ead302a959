"""Streams for the keyframe selector's tests (tests/test_keysel_cpu.py, tests/test_gpu_keysel.py): no
images, just (T_s2s, good, times) arrays.  The hand-written cases carry their expected keyframe ids;
the seeded random ones are compared with the restatement only."""
from typing import NamedTuple

import numpy as np

SIZES = (0, 1, 2, 7, 64, 65, 300)  # 65 crosses the wave
MARGIN = 1e-9  # no gate comparison of any case lies closer to its threshold than this


class Case(NamedTuple):
    T_s2s: np.ndarray  # (n, 7) q x,y,z,w, t
    good: np.ndarray   # (n,) int32
    times: np.ndarray  # (n,)
    time_interval: float
    distance_interval: float
    expected: object   # the keyframe ids written out by hand, or None


def _rows(translations, quats=None):
    t = np.asarray(translations, np.float64).reshape(-1, 3)
    q = np.tile([0.0, 0.0, 0.0, 1.0], (t.shape[0], 1)) if quats is None else np.asarray(quats, np.float64)
    return np.ascontiguousarray(np.concatenate([q, t], axis=1))


def random_stream(n: int, seed: int, p_good: float = 0.85, time_interval=0.3, distance_interval=0.3):
    """Small motions of about 0.1 m and 0.01 rad per frame, unit quaternions, frames about 0.1 s apart
    (jittered: the gaps are no bare multiples of 0.1)."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(n, 3)) * 0.01
    ang = np.linalg.norm(w, axis=1, keepdims=True)
    q = np.concatenate([np.sin(ang / 2) * w / np.maximum(ang, 1e-300), np.cos(ang / 2)], axis=1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    t = np.array([0.1, 0.0, 0.0]) + rng.normal(size=(n, 3)) * [0.02, 0.01, 0.005]
    good = (rng.random(n) < p_good).astype(np.int32)
    times = 1000.0 + np.cumsum(rng.uniform(0.08, 0.12, size=n))
    return Case(_rows(t, q), good, times, time_interval, distance_interval, None)


def cases():
    out = {}
    for n in SIZES:
        out[f"random{n}"] = random_stream(n, 100 + n)
    x = lambda d, n: [[d, 0.0, 0.0]] * n  # noqa: E731
    # the distance passes at once (1 m per frame); the time gate blocks: frame 3 is 0.34 s after frame 0,
    # frame 5 is 0.36 s after frame 3
    out["time_blocks"] = Case(_rows(x(1.0, 6)), np.ones(6, np.int32), np.array([0.0, 0.11, 0.22, 0.34, 0.45, 0.70]), 0.3, 0.3,
                              [0, -1, -1, 1, -1, 2])
    # the time passes at once (1 s per frame); the distance gate blocks: 0.11 m per frame, 0.33 m after 3
    out["distance_blocks"] = Case(_rows(x(0.11, 6)), np.ones(6, np.int32), np.arange(6) * 1.0 + 5.0, 0.3, 0.3,
                                  [0, -1, -1, 1, -1, -1])
    r = random_stream(7, 7)
    out["none_good"] = Case(r.T_s2s, np.zeros(7, np.int32), r.times, 0.3, 0.3, [-1] * 7)
    # the first frames skipped (good 0, and the first frame's -1), then good ones 1 s and 0.5 m apart
    out["skipped_first"] = Case(_rows(x(0.5, 6)), np.array([-1, 0, 0, 1, 1, 1], np.int32), np.arange(6) * 1.0, 0.3, 0.3,
                                [-1, -1, -1, 0, 1, 2])
    out["stationary"] = Case(_rows(x(0.0, 5)), np.ones(5, np.int32), np.arange(5) * 1.0, 0.3, 0.3, [0, -1, -1, -1, -1])
    # a frame marked not good moves 0.25 m: the product still applies (tfBroadcast runs on both branches), so
    # frame 2 is 0.35 m from keyframe 0; without it 0.1 m would not pass
    out["bad_frame_moves"] = Case(_rows([[0.1, 0, 0], [0.25, 0, 0], [0.1, 0, 0]]), np.array([1, 0, 1], np.int32),
                                  np.array([0.0, 1.0, 2.0]), 0.3, 0.3, [0, -1, 1])
    r = random_stream(20, 20, p_good=0.7, time_interval=0.0, distance_interval=0.0)
    ids = np.full(20, -1)
    ids[r.good == 1] = np.arange(int((r.good == 1).sum()))
    out["zero_intervals"] = r._replace(expected=[int(v) for v in ids])
    return out
