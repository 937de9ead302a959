"""CPU checks of the Scan Context place database (lislam_place_*): the header declares the ABI and
the library exports it, the config struct's layout, null arguments, and self-checks of the
restatement (tests/restate_sc.py) on hand-made inputs.  No compute call without a GPU."""
import ctypes
import math
import os
import re

import numpy as np

import restate_sc as SC
from place_cases import AXES_AND_DIAGONALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lislam.h")
PLACE_FUNCTIONS = ["lislam_place_add_batch", "lislam_place_add_clouds", "lislam_place_create", "lislam_place_destroy",
                   "lislam_place_detect", "lislam_place_distance", "lislam_place_download", "lislam_place_size"]
f32 = np.float32


def test_header_declares_and_library_exports_place_api(pkg):
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"^\s*int\s+(lislam_place_\w+)\s*\(", text, re.M)))
    assert declared == PLACE_FUNCTIONS
    lib = pkg.native.load()
    assert all(hasattr(lib, f) for f in PLACE_FUNCTIONS)
    assert set(PLACE_FUNCTIONS) <= set(pkg.native.EXPORTED_SYMBOLS)
    for name, value in (("LISLAM_PLACE_DESC", pkg.native.PLACE_DESC), ("LISLAM_PLACE_RING_KEY", pkg.native.PLACE_RING_KEY),
                        ("LISLAM_PLACE_SECTOR_KEY", pkg.native.PLACE_SECTOR_KEY)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value


def test_place_config_layout_and_defaults(pkg):
    n = pkg.native
    assert ctypes.sizeof(n.PlaceConfig) == 56
    c = n.PlaceConfig()
    got = {k: getattr(c, k) for k, _ in n.PlaceConfig._fields_}
    assert got == SC.DEFAULTS  # Scancontext.h:77-96
    assert pkg.ScanContext is pkg.place.ScanContext


def test_place_kernels_are_in_the_library(pkg):
    data = open(pkg.native.LIB_PATH, "rb").read()
    for k in pkg.native.PLACE_KERNELS:
        assert k.encode() in data, k


def test_place_null_arguments(pkg):
    lib, E = pkg.native.load(), pkg.native.ERR_ARG
    h = ctypes.c_void_p()
    n = ctypes.c_int32()
    assert lib.lislam_place_create(None, None, 16, ctypes.byref(h)) == E
    assert lib.lislam_place_destroy(None) == E
    assert lib.lislam_place_size(None, ctypes.byref(n)) == E
    assert lib.lislam_place_add_clouds(None, None, None, 0) == E
    assert lib.lislam_place_add_batch(None, None, 0, 0) == E
    assert lib.lislam_place_detect(None, 0, 0, None, None, None, None, None) == E
    assert lib.lislam_place_distance(None, None, None, 0, None, None) == E
    assert lib.lislam_place_download(None, 0, 0, None, 0, ctypes.byref(n)) == E


def _cloud(rows):
    return np.array(rows, f32).reshape(-1, 4)


def test_restatement_dropout_point_lands_in_first_bin():
    d = SC.make_scancontext(_cloud([[0, 0, 0, 0]]))
    assert d.shape == (20, 60)
    assert d[0, 0] == 2.0 and np.count_nonzero(d) == 1
    # a higher point of that bin wins, a lower one does not
    assert SC.make_scancontext(_cloud([[0, 0, 0, 0], [0.5, 0.01, 1.5, 0]]))[0, 0] == 3.5
    assert SC.make_scancontext(_cloud([[0, 0, 0, 0], [0.5, 0.01, -1.5, 0]]))[0, 0] == 2.0


def test_restatement_max_radius_boundary():
    above = np.nextafter(f32(80.0), f32(np.inf))
    d = SC.make_scancontext(_cloud([[80.0, 0, 1, 0]]))
    assert d[19, 0] == 3.0 and np.count_nonzero(d) == 1  # atan(0) = 0: sector index max(0, 1) = 1
    assert np.count_nonzero(SC.make_scancontext(_cloud([[above, 0, 1, 0]]))) == 0
    assert np.count_nonzero(SC.make_scancontext(_cloud([[0, -above, 1, 0]]))) == 0


def test_restatement_axis_and_diagonal_sectors():
    keep, ring, sector, z = SC.bins(_cloud(AXES_AND_DIAGONALS))
    assert keep.all() and np.all(z == f32(2.0)) and np.all(ring == 2)
    # the +x axis reaches sector 60 from below (y < 0: 360 - atan(..), which rounds to 360.0f) ...
    assert list(sector + 1) == [15, 30, 45, 60, 8, 23, 38, 53]
    # ... while y = +0.0 and y = -0.0 (which counts as >= 0) take the first branch: 0 deg, sector max(0, 1) = 1
    _, _, s1, _ = SC.bins(_cloud([[10, 0.0, 0, 0], [10, -0.0, 0, 0], [-0.0, 0.0, 0, 0]]))
    assert list(s1 + 1) == [1, 1, 1]
    ang, defined = SC.xy2theta(np.array([np.nan, 1.0], f32), np.array([1.0, np.nan], f32))
    assert not defined.any()
    keep, _, _, _ = SC.bins(_cloud([[np.nan, 1, 0, 0], [1, np.nan, 0, 0], [1, 1, np.nan, 0]]))
    assert list(keep) == [False, False, True]  # a NaN height passes the binning and never wins the maximum
    assert np.count_nonzero(SC.make_scancontext(_cloud([[1, 1, np.nan, 0]]))) == 0


def test_restatement_no_point_height_becomes_zero():
    d = SC.make_scancontext(_cloud([[5, 5, -1002.0, 0], [30, -5, -1001.5, 0], [-20, 1, -1003.0, 0]]))
    assert np.count_nonzero(d) == 1 and np.sum(d) == 0.5 - 1000.0  # -1002 + 2 == NO_POINT -> 0; below it never wins
    assert SC.make_scancontext(np.zeros((0, 4), f32)).any() == False  # noqa: E712


def test_restatement_zero_descriptors_distance():
    z = np.zeros((20, 60))
    assert SC.distance_btn_scancontext(z, z) == (1e7, 0)
    assert math.isnan(SC.dist_direct(z, SC.column_norms(z), z, SC.column_norms(z), 0))
    rng = np.random.default_rng(0)
    a = rng.random((20, 60)).astype(f32).astype(np.float64)
    d, s = SC.distance_btn_scancontext(a, np.roll(a, 7, axis=1))
    assert s == 60 - 7 and abs(d) < 1e-12  # circshift(b, 53) == a
    assert SC.shift_set(2, 60, 0.1) == [0, 1, 2, 3, 4, 5, 59]
    assert len(SC.shift_set(5, 60, 1.0)) == 61 and set(SC.shift_set(5, 60, 1.0)) == set(range(60))


def test_restatement_knn_float_metric_and_ties():
    keys = np.zeros((5, 20), f32)
    keys[1, 3] = 1.0
    keys[2, 7] = -1.0
    keys[3, 19] = 0.5
    idx, d = SC.knn(keys, np.zeros(20, f32), 4)
    assert list(idx) == [0, 4, 3, 1] and list(d) == [0.0, 0.0, 0.25, 1.0]  # equal distances: lower index first


def test_stateful_manager_matches_closed_form_prefix():
    cloud = _cloud([[1, 1, 0, 0]])
    for E, P in ((50, 50), (5, 4), (3, 1)):
        m = SC.SCManager(num_exclude_recent=E, tree_making_period=P, num_candidates=2)
        for i in range(401):
            m.make_and_save(cloud)
            loop_id, yaw = m.detect()
            assert m.last["prefix"] == SC.tree_prefix(i, E, P), (E, P, i)
            if i < E:
                assert (loop_id, yaw) == (-1, 0.0)
            else:
                assert 1 <= m.last["prefix"] <= i + 1 - E
                assert loop_id == 0 and yaw == 0.0 and m.last["min_dist"] == 0.0  # identical clouds: first candidate, no shift
