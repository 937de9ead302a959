"""Inputs of the degenerate-odometry tests (test_odom_cases_cpu.py, test_gpu_odom_degenerate.py): pairs
of feature sets with blank, tiny or one-line clouds for the node API, less-flat targets around the
target index's in-register / global sort boundary, and scan streams with blank and thin scans for the
batch path.  Everything is cut from synthetic corridor scans by index, so every cloud stays ordered by
scan line (the ABI's contract).  numpy only; `oracle` and `synth` are passed in by the tests."""
from __future__ import annotations

import dataclasses

import numpy as np

CLOUDS = ("sharp", "less_sharp", "flat", "less_flat")
TARGETS_K = (0, 1, 2, 3, 15, 16, 17, 31, 33, 64, 200)
QUERIES_K = (0, 1, 2, 3, 6, 15, 16, 17, 64)
LARGE_POOLED = (16383, 16384, 16385, 20000, 40000)  # around k_target_index<8,32>'s 16384 register keys
LARGE_SINGLE = (1023, 1024, 1025)                    # around the sort's P = 1024 floor
SORT_BOUNDARY = 16384

# Cases whose oracle result is exactly: no correspondence in either pass, para carried, 0 / 0 iterations.
ZERO_NODE_CASES = ("targets_0", "targets_1", "targets_2", "targets_3", "queries_0", "one_line", "every_4th_line",
                   "identical_targets", "all_empty")


def sub(f, **counts_or_indices):
    """A copy of the oracle.ScanFeatures `f` with the named clouds cut down: an int k keeps k points
    evenly spaced by index, anything else is used as an index (or boolean mask) array.  Indices are
    taken in the order given, so ascending indices keep the cloud line-sorted."""
    new = {}
    for name, sel in counts_or_indices.items():
        cloud = getattr(f, name)
        if isinstance(sel, (int, np.integer)):
            sel = np.linspace(0, cloud.shape[0] - 1, int(sel)).astype(int) if sel else np.zeros(0, int)
        new[name] = np.ascontiguousarray(cloud[np.asarray(sel)], np.float32).reshape(-1, 4)
    return dataclasses.replace(f, **new)


def empty(f):
    return sub(f, sharp=0, less_sharp=0, flat=0, less_flat=0)


def shifted(f, dx):
    """Every feature cloud of the frame translated by dx metres in x."""
    new = {}
    for name in CLOUDS:
        c = getattr(f, name).copy()
        c[:, 0] += np.float32(dx)
        new[name] = c
    return dataclasses.replace(f, **new)


def nudged(f, towards):
    """Every x, y, z of the frame's feature clouds moved one float ulp towards `towards`."""
    new = {}
    for name in CLOUDS:
        c = getattr(f, name).copy()
        c[:, :3] = np.nextafter(c[:, :3], np.float32(towards))
        new[name] = c
    return dataclasses.replace(f, **new)


def line_of(cloud):
    return cloud[:, 3].astype(np.int32)  # int(intensity): the scan line (laserOdometry.cpp:467)


def targets_where(f, pred):
    return sub(f, less_sharp=pred(line_of(f.less_sharp)), less_flat=pred(line_of(f.less_flat)))


def base_pair(oracle, synth):
    scans = synth.make_sequence(2, 16, 256, start=10)
    return [oracle.scan_registration(s) for s in scans]


def node_cases(oracle, synth):
    """name -> (f_last, f_curr), one pair for LaserOdometry.step each."""
    f0, f1 = base_pair(oracle, synth)
    cases = {}
    for k in TARGETS_K:
        cases[f"targets_{k}"] = (sub(f0, less_sharp=k, less_flat=k), f1)
    for k in QUERIES_K:
        cases[f"queries_{k}"] = (f0, sub(f1, sharp=k, flat=k))
    cases["one_line"] = (targets_where(f0, lambda l: l == 5), f1)
    cases["lines_0_1"] = (targets_where(f0, lambda l: l <= 1), f1)
    cases["every_2nd_line"] = (targets_where(f0, lambda l: l % 2 == 0), f1)
    cases["every_4th_line"] = (targets_where(f0, lambda l: l % 4 == 0), f1)
    cases["identical_targets"] = (sub(f0, less_sharp=np.full(40, f0.less_sharp.shape[0] // 2),
                                      less_flat=np.full(40, f0.less_flat.shape[0] // 2)), f1)
    cases["shift_0.4"] = (f0, shifted(f1, 0.4))
    cases["shift_6"] = (f0, shifted(f1, 6.0))
    cases["all_empty"] = (empty(f0), empty(f1))
    return cases


def living_node_frames(oracle, synth):
    """Five frames for one node: a full frame, a frame without targets (targets_0 style; its own
    queries are kept), a full frame, a frame with one sharp and one flat query, a full frame.  Pair 2
    has no targets, pair 3 a tiny system, pairs 1 and 4 follow them on the same device slots."""
    f = [oracle.scan_registration(s) for s in synth.make_sequence(5, 16, 256, start=10)]
    return [f[0], sub(f[1], less_sharp=0, less_flat=0), f[2], sub(f[3], sharp=1, flat=1), f[4]]


def large_target_cases(oracle, synth):
    """name -> (f_last, f_curr) at 64 x 1024: the last frame's less-flat cloud is n points drawn from
    the pooled less-flat clouds of five consecutive scans (re-sorted by scan line) or, for the small
    sizes, from one scan's cloud; the sixth scan is the current frame."""
    scans = synth.make_sequence(6, 64, 1024, start=10)
    feats = [oracle.scan_registration(s) for s in scans]
    pool = np.concatenate([f.less_flat for f in feats[:5]])
    pool = pool[np.argsort(line_of(pool), kind="stable")]
    cases = {}
    for n in LARGE_POOLED:
        pick = np.sort(np.random.default_rng(n).choice(pool.shape[0], n, replace=False))
        cases[f"large_{n}"] = (dataclasses.replace(feats[4], less_flat=np.ascontiguousarray(pool[pick])), feats[5])
    for n in LARGE_SINGLE:
        pick = np.sort(np.random.default_rng(n).choice(feats[4].less_flat.shape[0], n, replace=False))
        cases[f"large_{n}"] = (sub(feats[4], less_flat=pick), feats[5])
    return cases


CHAIN_VARIANTS = ("default", "blank_first", "blank_last")
USE_ALOAM = (0, 1, 1, 1, 0, 1, 1, 1, 1)


def chain_scans(synth, variant="default"):
    """Nine 16 x 256 scans: scan 3 blank, scan 5 with columns 40 and up dropped (a thin cloud), scan 7
    all points nearer than min_range (extraction removes every one).  blank_first / blank_last blank
    scan 0 / scan 8 as well."""
    scans = synth.make_sequence(9, 16, 256, start=10).copy()
    scans[3] = 0
    scans[5][:, 40:] = 0
    scans[7] = np.random.default_rng(0).uniform(-0.2, 0.2, size=scans[7].shape).astype(np.float32)
    if variant == "blank_first":
        scans[0] = 0
    elif variant == "blank_last":
        scans[8] = 0
    elif variant != "default":
        raise ValueError(variant)
    return scans


def chain_blank_pairs(variant="default"):
    """Pairs k (scan k against scan k - 1) where one side has no features at all."""
    blank = {3, 7} | ({0} if variant == "blank_first" else set()) | ({8} if variant == "blank_last" else set())
    return sorted(k for k in range(1, 9) if k in blank or k - 1 in blank)
