"""Inputs shared by test_deskew_restate_cpu.py and test_gpu_deskew.py: the 16 x 256 frames of
tests/odom_cases.py, plus the reference's negative-relTime quirk made explicit.  The
synthetic scans carry queries with s > 1 on their own but none with s < 0, so `quirky` lowers the
intensity of a few sharp / flat points of a frame by 0.003 below their line: int(intensity) then
truncates to the line below (s near 10) or, on line 0, towards zero (s slightly negative).  numpy only."""
from __future__ import annotations

import dataclasses

import numpy as np

import odom_cases as C

NODE_NAMES = ("targets_0", "targets_1", "targets_17", "queries_0", "queries_1", "queries_16", "one_line", "all_empty")
MODES = (1, 2)


def quirky(f, every=7):
    """A copy of the frame where every `every`-th sharp and flat point on line 0, and every `every`-th
    on the other lines starting one later, has intensity line - 0.003."""
    new = {}
    for name in ("sharp", "flat"):
        c = getattr(f, name).copy()
        line = C.line_of(c)
        on0 = np.flatnonzero(line == 0)[::every]
        rest = np.flatnonzero(line > 0)[1::every]
        for idx in (on0, rest):
            c[idx, 3] = line[idx].astype(np.float32) - np.float32(0.003)
        new[name] = c
    return dataclasses.replace(f, **new)


def living_frames(oracle, synth):
    """odom_cases.living_node_frames with the quirk in frames 1 and 4 (the two whose pairs have full
    targets and all their queries; pair 2 has no targets, pair 3 one query of each kind)."""
    f = C.living_node_frames(oracle, synth)
    return [f[0], quirky(f[1]), f[2], f[3], quirky(f[4])]


def node_pairs(oracle, synth):
    cases = C.node_cases(oracle, synth)
    return {name: cases[name] for name in NODE_NAMES}


def chain_features(oracle, synth, variant):
    return [oracle.scan_registration(s) for s in C.chain_scans(synth, variant)]
