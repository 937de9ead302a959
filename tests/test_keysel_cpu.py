"""CPU checks of the keyframe selector's contract (tests/restate_keysel.py) and of the new entry points'
boundary; nothing here needs a GPU.

The hand-written cases of tests/keysel_cases.py carry their expected ids; the restatement must give
them.  Two conditions keep the GPU comparison meaningful and are checked here, on every case: no
time[k] - last_time lies within 1e-9 of time_interval and no distance within 1e-9 of
distance_interval, so a last-ulp difference in a subtraction or a square root cannot flip a gate."""
import ctypes
import os
import re

import numpy as np
import pytest

import keysel_cases as KC
import restate_keysel as RK

CASES = KC.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_on_the_cases(name):
    c = CASES[name]
    r = RK.Selector(c.time_interval, c.distance_interval)
    ids, T, nodes = r.step(c.T_s2s, c.good, c.times)
    n = c.times.shape[0]
    assert ids.shape == (n,) and T.shape == (n, 4, 4) and nodes.shape == (int((ids >= 0).sum()), RK.NODE)
    if c.expected is not None:
        assert list(ids) == list(c.expected)
    assert np.all(ids[c.good != 1] == -1)
    assert list(ids[ids >= 0]) == list(range(nodes.shape[0])) and list(nodes[:, 1]) == list(range(nodes.shape[0]))
    mt, md = r.margins()
    print(name, "selected", nodes.shape[0], "of", n, "margins", mt, md)
    assert mt > KC.MARGIN and md > KC.MARGIN
    if n:
        assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))


def test_random_streams_select_some_and_skip_some():
    for n in (64, 65, 300):
        c = CASES[f"random{n}"]
        ids, _, _ = RK.Selector(c.time_interval, c.distance_interval).step(c.T_s2s, c.good, c.times)
        good = int((c.good == 1).sum())
        assert 0 < int((ids >= 0).sum()) < good < n


def test_node_rows_chain():
    """prev_position_ / prev_rotation_ of a node are cur_position_ / cur_rotation_ of the node before; the
    first node's are the constructor's zeros (:33-36)."""
    c = CASES["random65"]
    _, T, nodes = RK.Selector(c.time_interval, c.distance_interval).step(c.T_s2s, c.good, c.times)
    assert not nodes[0, 5:8].any() and not nodes[0, 17:26].any()
    assert np.array_equal(nodes[1:, 5:8], nodes[:-1, 2:5]) and np.array_equal(nodes[1:, 17:26], nodes[:-1, 8:17])


def test_split_invariance_of_the_restatement():
    c = CASES["random65"]
    whole = RK.Selector(c.time_interval, c.distance_interval).step(c.T_s2s, c.good, c.times)
    r = RK.Selector(c.time_interval, c.distance_interval)
    parts = [r.step(c.T_s2s[a:b], c.good[a:b], c.times[a:b]) for a, b in ((0, 32), (32, 65))]
    for k in range(3):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])


def test_rotation_is_a_rotation():
    R = np.array(RK.rotation(*(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]))))
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1) < 1e-15


def test_new_kernels_are_in_the_library(pkg):
    n = pkg.native
    data = open(n.LIB_PATH, "rb").read()
    for k in n.KEYSEL_KERNELS + ("k_bow_scan_list", "k_pgo_add_keyframes"):
        assert k.encode() in data, k
    assert "k_bow_scan_list" in n.BOW_KERNELS and "k_pgo_add_keyframes" in n.PGO_KERNELS


def test_feeds_header_declares_what_the_library_exports(pkg):
    """include/lislam_feeds.h against native.FEED_SYMBOLS, as tests/test_abi_cpu.py does for include/lislam.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lislam_feeds.h")).read()
    declared = sorted(set(re.findall(r"^\s*int\s+(lislam_\w+)\s*\(", text, re.M)))
    assert declared == sorted(pkg.native.FEED_SYMBOLS) and '#include "lislam.h"' in text
    lib = pkg.native.load()
    assert all(hasattr(lib, f) for f in declared)
    assert not set(declared) & set(pkg.native.EXPORTED_SYMBOLS)
    main = open(os.path.join(root, "include", "lislam.h")).read()
    assert sorted(set(re.findall(r"^\s*int\s+(lislam_keysel_\w+)\s*\(", main, re.M))) == sorted(
        s for s in pkg.native.EXPORTED_SYMBOLS if s.startswith("lislam_keysel_"))


def test_abi_of_the_new_entry_points(pkg):
    n, lib = pkg.native, pkg.native.load()
    assert ctypes.sizeof(n.KeyselConfig) == 16
    h = ctypes.c_void_p()
    assert lib.lislam_keysel_create(None, None, ctypes.byref(h)) == n.ERR_ARG
    assert lib.lislam_keysel_destroy(None) == n.ERR_ARG
    assert lib.lislam_keysel_step(None, None, None, None, 0, None, None, None, None) == n.ERR_ARG
    assert lib.lislam_keysel_step_batch(None, None, 0, 0, None, None, None, None, None) == n.ERR_ARG
    assert lib.lislam_keysel_state(None, None, None, None) == n.ERR_ARG
    assert lib.lislam_keyframes_add_batch_scans(None, None, None, 0) == n.ERR_ARG
    assert lib.lislam_place_add_batch_scans(None, None, None, 0) == n.ERR_ARG
    assert lib.lislam_bow_add_batch_scans(None, None, None, 0) == n.ERR_ARG
    assert lib.lislam_pgo_add_keyframes(None, None, 0, None, 0, None) == n.ERR_ARG
    assert lib.lislam_pgo_add_batch_scans(None, None, None, 0, None) == n.ERR_ARG
