"""The ORB edge cases (tests/orb_cases.py) have the properties they are named for, checked on the CPU
oracle alone: the GPU test (test_gpu_orb_edges.py) compares the kernels with the oracle on these
inputs, so a case that lost its point (a "tied" image without ties, a capacity case that fits) would
let that comparison pass for nothing.  No GPU."""
import numpy as np
import pytest

import orb_cases as C


@pytest.fixture(scope="module")
def detected(oracle):
    """name -> (case, the oracle's (keypoints, descriptors, points)) of every detect and capacity case."""
    out = {}
    for case in C.detect_cases(oracle) + C.capacity_cases():
        name, img, tr, mask, n = case
        out[name] = (case, oracle.orb_detect(img, tr, n, mask))
    return out


def test_budget_restatement():
    for n, nper in C.BUDGET_NPER.items():
        assert C.features_per_level(n) == nper
    assert C.features_per_level(1000)[0] == 217 and sum(C.features_per_level(1000)) == 1000
    assert C.lcap(100)[0] == 108 and C.lcap(200)[0] == 150 and C.lcap(1000)[0] == 498
    for n in (1, 7, 100, 200, 500, 1000, 2000, 16384):
        assert sum(C.features_per_level(n)) >= n and all(v >= 0 for v in C.features_per_level(n))


def test_case_lists_are_complete(oracle, detected):
    names = set(detected)
    assert tuple(c[0] for c in C.detect_cases(oracle)) == C.DETECT_NAMES
    assert tuple(c[0] for c in C.capacity_cases()) == C.CAPACITY_CASES
    assert tuple(c[0] for c in C.match_cases()) == C.MATCH_NAMES
    for H, W in C.SHAPES + (C.ODD_WIDTH,):
        assert f"shape_{H}x{W}" in names
    for H, W in C.MASKED_SHAPES:
        assert f"shape_{H}x{W}_masked" in names
    assert {"content_zeros", "content_255", "content_checker4", "content_blocks8", "content_noise", "content_frame",
            "content_tied", "mask_zero", "mask_one_pixel", "mask_not_255", "track_zero_axes"} <= names
    assert {f"budget_{n}" for n in C.BUDGETS} <= names and set(C.CAPACITY_CASES) <= names
    assert C.ODD_WIDTH[1] % 4 == 2
    assert [n for n, _, _ in C.match_cases()][:len(C.MATCH_SIZES)] == [f"sizes_{q}x{t}" for q, t in C.MATCH_SIZES]


def test_both_pyramid_paths_are_covered():
    """The shape lists of the GPU test's docstring follow from the `fused` condition, and each side of
    it has at least two shapes among the cases."""
    for hw in C.FUSED_SHAPES:
        assert C.takes_fused_path(*hw), hw
    for hw in C.UNFUSED_SHAPES:
        assert not C.takes_fused_path(*hw), hw
    shapes = set(C.SHAPES + (C.ODD_WIDTH,))
    assert len(shapes & set(C.FUSED_SHAPES)) >= 2 and len(shapes & set(C.UNFUSED_SHAPES)) >= 2
    assert shapes <= set(C.FUSED_SHAPES) | set(C.UNFUSED_SHAPES)
    assert C.level_sizes(8, 8)[7] == (2, 2)


def test_shape_cases_have_keypoints(detected):
    for name, (case, (kp, de, p3)) in detected.items():
        if name.startswith("shape_"):
            assert len(kp) >= 2, (name, len(kp))
            assert len(de) == len(kp) == len(p3)


def test_empty_cases(detected):
    for name in C.EMPTY_CASES + ("mask_zero",):
        assert len(detected[name][1][0]) == 0, name


def test_content_cases(detected):
    nper, cap = C.features_per_level(1000), C.lcap(1000)
    # the checkerboard and the blocks: nothing on level 0 (a FAST-9 arc needs a corner the 4 / 8 px
    # squares of level 0 do not have), every other level populated, and past its budget on ties
    for name in ("content_checker4", "content_blocks8"):
        lc = C.level_counts(detected[name][1][0])
        assert lc[0] == 0 and all(v > 0 for v in lc[1:]), (name, lc)
        assert all(v <= c for v, c in zip(lc, cap)), (name, lc)
    lc = C.level_counts(detected["content_checker4"][1][0])
    assert any(v > n for v, n in zip(lc, nper)), lc
    # uniform noise fills the budget of every level but the last
    lc = C.level_counts(detected["content_noise"][1][0])
    assert lc[:7] == nper[:7], lc
    # tied: ties cross the n-th response at level 0 and stay within the library's room
    lc = C.level_counts(detected["content_tied"][1][0])
    assert nper[0] < lc[0] <= cap[0], lc
    assert all(v <= c for v, c in zip(lc, cap)), lc


def test_frame_case_keypoints_lie_at_the_borders(detected):
    (_, img, _, _, _), (kp, _, _) = detected["content_frame"]
    H, W = img.shape
    x, y = kp[:, 0], kp[:, 1]
    assert (x <= 3).any() and (x >= W - 1 - 3).any() and (y <= 3).any() and (y >= H - 1 - 3).any()
    # none in the interior: every keypoint within the 6 px frame (level-0 coordinates)
    assert np.minimum.reduce([x, W - 1 - x, y, H - 1 - y]).max() < 6.0
    # reflect-101 borders in play: on the noise image a good part of the keypoints lies within 16 px of the left or top edge
    nk = detected["content_noise"][1][0]
    assert ((nk[:, 0] < 16) | (nk[:, 1] < 16)).sum() >= 100


def test_budget_cases(detected):
    for n, nper in C.BUDGET_NPER.items():
        assert C.level_counts(detected[f"budget_{n}"][1][0]) == nper, n
    lc = C.level_counts(detected["budget_16384"][1][0])
    assert all(0 < v <= n for v, n in zip(lc, C.features_per_level(16384))), lc  # every corner there is, no level full


def test_mask_cases(detected):
    (_, _, _, one, _), (kp, _, _) = detected["mask_one_pixel"]
    assert int((one > 0).sum()) == 1 and len(kp) == 1
    assert one[int(kp[0, 1]), int(kp[0, 0])] == 255
    (_, _, _, odd, _), (kp, _, _) = detected["mask_not_255"]
    assert set(np.unique(odd)) == {0, 1, 2, 3} and len(kp) > 0
    assert (odd[kp[:, 1].astype(int), kp[:, 0].astype(int)] > 0).all()
    assert len(kp) < len(detected["content_noise"][1][0])


def test_track_case_makes_the_filters_differ(oracle, detected):
    (_, img, tr, mask, n), (kp, _, _) = detected["track_zero_axes"]
    mkp, mde, mp3 = C.map_filter_reference(oracle, img, tr, n, mask)
    full = len(detected["content_noise"][1][0])
    assert len(kp) < len(mkp) < full, (len(kp), len(mkp), full)
    assert (np.abs(mp3[:, 0]) < 0.01).sum() >= 100  # kept by mapOptimization's filter alone
    assert (np.abs(mp3) < 0.01).all(1).sum() == 0


def test_capacity_cases_exceed_the_room(detected):
    for name in C.CAPACITY_CASES:
        (_, _, _, _, n), (kp, _, _) = detected[name]
        lc, cap = C.level_counts(kp), C.lcap(n)
        assert any(v > c for v, c in zip(lc, cap)), (name, lc, cap)


def test_match_cases_oracle_equals_numpy(oracle):
    for name, a, b in C.match_cases():
        r = oracle.orb_match(a, b)
        assert np.array_equal(r, C.crosscheck_match(a, b)), name
        if name == "train_65535":
            assert r[0].tolist() == [0, 65534, 0] and r[1].tolist() == [1, 40000, 0]
        if name == "zeros_vs_ones":
            assert r.tolist() == [[0, 0, 256]]
        if name == "permuted":
            assert len(r) == len(a) and (r[:, 2] == 0).all()
        if name == "low_bytes":
            assert r[:, 2].max() <= 16
        if name in ("sizes_0x5", "sizes_5x0"):
            assert r.shape == (0, 3)


def test_small_sequence(oracle, synth):
    """The 16 x 512 sequence: the scans' a1 images are the intended ones, the repeated frame
    re-detects, the moving frames solve, and the last pair selects 0 < G < 4 matches and is skipped."""
    imgs, scans = C.small_sequence(synth)
    feats = [oracle.scan_registration(s) for s in scans]
    for f, im in zip(feats, imgs):
        assert np.array_equal(f.img_intensity, im)
    st, T = oracle.intensity_odometry(np.stack(imgs), np.stack([f.cloud_track for f in feats]), C.SEQ_NFEATURES,
                                      C.hand_held_mask(C.SEQ_H, C.SEQ_W))
    assert st[0, 0] == -1
    assert st[1, 0] == 1 and st[1, 1] == 0 and st[3, 0] == 1
    assert st[2, 1] == 1 and st[2, 0] == 0  # the repeated frame
    assert st[5, 0] == 0 and st[5, 1] == 1 and 0 < st[5, 4] < 4, st[5]
