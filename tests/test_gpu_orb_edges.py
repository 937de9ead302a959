"""GPU parity of the ORB front end (lislam_orb_detect, lislam_orb_match, the intensity tracker, the batch
and the sliding window's batch detect) with the CPU oracle on the edge cases of tests/orb_cases.py,
whose properties tests/test_orb_cases_cpu.py asserts on the oracle alone.

Keypoints, descriptors, points, matches and stats words are bit-exact; T_s2s within POSE_TOL.

Pyramid paths, from engine_detect_slots' `fused` condition (W % 4 == 0, level 1 at most 64 rows, a
padded level-0 row of at most 1024 dwords, H * W <= 64 KiB, level 1 <= 48 KiB, level 2 <= 32 KiB;
orb_cases.takes_fused_path restates it and the CPU test holds these lists to it):
  k_orb_pyramid + k_orb_roiblur (fused):  16x512, 32x1024, 32x2048 (H * W = 64 KiB exactly, level 2 =
                                          1422 x 22 = 31284 B), 24x100, 8x1024, 8x8, and every 64x1024 case
  k_orb_level + k_orb_blur:               128x1024 (H * W = 128 KiB), 17x67 (W % 4 = 3), 9x9 (W % 4 = 1),
                                          24x102 (W % 4 = 2)

Capacity: a pyramid level has room for 2 * n_l + 64 keypoints, the reference's retainBest for any
number of tied responses.  Every entry point either returns the oracle's full set or fails with
LISLAM_ERR_CAPACITY and an error text naming the ORB level capacity; it never returns a cut set with
status OK, and the object works again on the next ordinary input.
"""
import numpy as np
import pytest

import orb_cases as C

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # BASELINE.json north_star
CAPACITY_TEXT = "ORB level keypoint capacity"


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_ctx(pkg):
    c = pkg.Context(n_scans=C.SEQ_H, width=C.SEQ_W)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return {c[0]: c for c in C.detect_cases(oracle) + C.capacity_cases()}


@pytest.fixture(scope="module")
def matches():
    return {name: (a, b) for name, a, b in C.match_cases()}


@pytest.fixture(scope="module")
def ordinary(oracle, synth):
    """Six synthetic 64 x 1024 scans with their a1 images and tracks."""
    scans = synth.make_sequence(6, start=20)
    feats = [oracle.scan_registration(s) for s in scans]
    return scans, np.stack([f.img_intensity for f in feats]), np.stack([f.cloud_track for f in feats])


@pytest.fixture
def own():
    """own(obj) registers a tracker, batch or map for close() when the test ends, passed or failed: an
    object that outlived its module-scoped context would be destroyed after it."""
    objs = []

    def add(o):
        objs.append(o)
        return o

    yield add
    for o in reversed(objs):
        o.close()


def assert_same_features(got, ref, what):
    kp, de, p3 = got
    rkp, rde, rp3 = ref
    assert kp.shape == rkp.shape and de.shape == rde.shape and p3[:, :3].shape == rp3.shape, (what, kp.shape, rkp.shape)
    assert np.array_equal(kp, rkp), what
    assert np.array_equal(de, rde), what
    assert np.array_equal(p3[:, :3], rp3), what


def assert_pairs_equal(st, T, rst, rT, k):
    assert list(st[:5]) == list(rst[:5]) and st[7] == rst[7], (k, st, rst)
    assert np.max(np.abs(T - rT)) < POSE_TOL, (k, T, rT)


def full_or_capacity(pkg, call):
    """The capacity contract: the result of `call`, or None after a LISLAM_ERR_CAPACITY failure whose
    error text names the ORB level capacity."""
    try:
        return call()
    except pkg.native.LislamError as e:
        assert "status -3" in str(e) and CAPACITY_TEXT in str(e), str(e)
        return None


# ------------------------------------------------------------------ detect
@pytest.mark.parametrize("name", C.DETECT_NAMES)
def test_detect_bit_exact(pkg, oracle, ctx, cases, name):
    _, img, tr, mask, n = cases[name]
    got = pkg.intensity.orb_detect(ctx, img, tr, n, mask)
    ref = oracle.orb_detect(img, tr, n, mask)
    print(name, img.shape, n, "keypoints", len(ref[0]), "per level", C.level_counts(ref[0]))
    assert_same_features(got, ref, name)


@pytest.mark.parametrize("name", ["track_zero_axes", "shape_17x67_masked", "content_tied"])
def test_detect_map_filter_bit_exact(pkg, oracle, ctx, cases, name):
    """mapOptimization's three-axis zero filter on the same inputs (lislam_orb_detect_map)."""
    _, img, tr, mask, n = cases[name]
    got = pkg.intensity.orb_detect(ctx, img, tr, n, mask, map_filter=True)
    assert_same_features(got, C.map_filter_reference(oracle, img, tr, n, mask), name)
    assert np.all(got[2][:, 3] == 0)


# ------------------------------------------------------------------ match
@pytest.mark.parametrize("name", C.MATCH_NAMES)
def test_match_bit_exact(pkg, oracle, ctx, matches, name):
    a, b = matches[name]
    got = pkg.intensity.orb_match(ctx, a, b)
    ref = oracle.orb_match(a, b)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), name
    assert np.array_equal(got, C.crosscheck_match(a, b)), name


# ------------------------------------------------------------------ small shapes through the pair kernels
@pytest.fixture(scope="module")
def small(oracle, synth):
    imgs, scans = C.small_sequence(synth)
    feats = [oracle.scan_registration(s) for s in scans]
    for f, im in zip(feats, imgs):
        assert np.array_equal(f.img_intensity, im)
    tracks = np.stack([f.cloud_track for f in feats])
    mask = C.hand_held_mask(C.SEQ_H, C.SEQ_W)
    rst, rT = oracle.intensity_odometry(np.stack(imgs), tracks, C.SEQ_NFEATURES, mask)
    return np.stack(imgs), scans, tracks, mask, rst, rT


def test_small_shape_tracker(pkg, small_ctx, small, own):
    """16 x 512 frames: moving noise, a repeated frame (re-detection with 2n), and a last pair that
    selects fewer than 4 matches and is skipped by the G >= 4 rule."""
    imgs, _, tracks, mask, rst, rT = small
    assert rst[2, 1] == 1 and rst[5, 0] == 0 and 0 < rst[5, 4] < 4
    tr = own(pkg.intensity.IntensityTracker(small_ctx, C.SEQ_H, C.SEQ_W, C.SEQ_NFEATURES, mask))
    for k in range(len(imgs)):
        T, st = tr.detectfeatures(imgs[k], tracks[k])
        print(k, st, rst[k])
        assert_pairs_equal(st, T, rst[k], rT[k], k)


def test_small_shape_batch(pkg, small_ctx, small, own):
    imgs, scans, tracks, mask, rst, rT = small
    nat = pkg.native
    n = len(scans)
    b = own(pkg.Batch(small_ctx, n))
    b.upload(scans)
    b.extract(n)
    b.intensity_odometry(n, C.SEQ_NFEATURES, mask)
    assert b.download(nat.OUT_ORB_STATS, 0)[0] == -1
    for k in range(1, n):
        assert_pairs_equal(b.download(nat.OUT_ORB_STATS, k), b.download(nat.OUT_ORB_T, k), rst[k], rT[k], k)


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("map_filter", [False, True])
@pytest.mark.parametrize("name", C.CAPACITY_CASES)
def test_capacity_detect(pkg, oracle, ctx, cases, name, map_filter):
    _, img, tr, mask, n = cases[name]
    got = full_or_capacity(pkg, lambda: pkg.intensity.orb_detect(ctx, img, tr, n, mask, map_filter=map_filter))
    if got is not None:
        ref = C.map_filter_reference(oracle, img, tr, n, mask) if map_filter else oracle.orb_detect(img, tr, n, mask)
        assert_same_features(got, ref, name)
    # the next ordinary call on the context is unaffected
    _, img, tr, mask, n = cases["shape_16x512"]
    assert_same_features(pkg.intensity.orb_detect(ctx, img, tr, n, mask), oracle.orb_detect(img, tr, n, mask), "after " + name)


@pytest.mark.parametrize("good_before", [0, 2])
@pytest.mark.parametrize("name", C.CAPACITY_CASES)
def test_capacity_tracker(pkg, oracle, ctx, cases, ordinary, own, name, good_before):
    """The overflowing frame as the tracker's first frame and after two good ones: the step fails (or
    reports the oracle's full keypoint count), and the frames after it equal the oracle again."""
    _, img, tr, _, n = cases[name]
    _, imgs, tracks = ordinary
    mask = C.hand_held_mask(64, 1024)
    seq_i = np.concatenate([imgs[:good_before], img[None]])
    seq_t = np.concatenate([tracks[:good_before], tr[None]])
    rst, rT = oracle.intensity_odometry(seq_i, seq_t, n, mask)
    t = own(pkg.intensity.IntensityTracker(ctx, 64, 1024, n, mask))
    for k in range(good_before):
        T, st = t.detectfeatures(seq_i[k], seq_t[k])
        assert_pairs_equal(st, T, rst[k], rT[k], k)
    got = full_or_capacity(pkg, lambda: t.detectfeatures(img, tr))
    if got is not None:  # the full set: the oracle's counts and pose, nothing cut
        assert_pairs_equal(got[1], got[0], rst[-1], rT[-1], "overflowing frame")
        return
    # the failed frame is dropped: the tracker starts over with the next frame
    rst, rT = oracle.intensity_odometry(imgs[2:5], tracks[2:5], n, mask)
    for k in range(3):
        T, st = t.detectfeatures(imgs[2 + k], tracks[2 + k])
        assert_pairs_equal(st, T, rst[k], rT[k], ("after the failure", k))


@pytest.mark.parametrize("name", C.CAPACITY_CASES)
def test_capacity_batch(pkg, oracle, synth, ctx, cases, ordinary, own, name):
    """One overflowing scan among ordinary ones: the batch call or the first read of its outputs fails
    (or every scan's keypoints are the oracle's), every later read of that batch fails alike, and the
    same batch object given ordinary scans equals the oracle again."""
    _, img, _, _, n = cases[name]
    scans, imgs, tracks = ordinary
    nat = pkg.native
    mask = C.hand_held_mask(64, 1024)
    seq = np.stack([scans[0], scans[1], C.scan_of(synth, img, 22), scans[2]])
    feats = [oracle.scan_registration(s) for s in seq]
    assert np.array_equal(feats[2].img_intensity, img)
    b = own(pkg.Batch(ctx, 4))
    b.upload(seq)
    b.extract(4)

    def run():
        b.intensity_odometry(4, n, mask)
        return [b.download(nat.OUT_ORB_KEYPOINTS, k) for k in range(4)]

    got = full_or_capacity(pkg, run)
    if got is not None:
        for k in range(4):
            rkp, _, _ = oracle.orb_detect(feats[k].img_intensity, feats[k].cloud_track, n, mask)
            assert got[k].shape == rkp.shape and np.array_equal(got[k], rkp), (name, k, got[k].shape, rkp.shape)
    else:
        for what in (nat.OUT_ORB_STATS, nat.OUT_ORB_T, nat.OUT_ORB_KEYPOINTS, nat.OUT_ORB_DESCRIPTORS):
            assert full_or_capacity(pkg, lambda: b.download(what, 1)) is None, what
    # recovery: ordinary scans through the same batch
    rst, rT = oracle.intensity_odometry(imgs[:4], tracks[:4], n, mask)
    b.upload(scans[:4])
    b.extract(4)
    b.intensity_odometry(4, n, mask)
    for k in range(1, 4):
        assert_pairs_equal(b.download(nat.OUT_ORB_STATS, k), b.download(nat.OUT_ORB_T, k), rst[k], rT[k], ("recovery", k))
    rkp, _, _ = oracle.orb_detect(imgs[2], tracks[2], n, mask)
    assert np.array_equal(b.download(nat.OUT_ORB_KEYPOINTS, 2), rkp)


@pytest.mark.parametrize("name", C.CAPACITY_CASES)
def test_capacity_mapwin_batch_detect(pkg, oracle, synth, ctx, cases, ordinary, own, name):
    """lislam_batch_mapopt_window detects the scan's features on the device: an overflowing scan fails
    the call (or gives the window the oracle's full set), and the next ordinary scan steps as on an
    untouched MapOptimization."""
    _, img, _, _, n = cases[name]
    scans, _, _ = ordinary
    seq = np.stack([scans[0], C.scan_of(synth, img, 22), scans[1]])
    f1 = oracle.scan_registration(seq[1])
    assert np.array_equal(f1.img_intensity, img)
    b = own(pkg.Batch(ctx, 3))
    b.upload(seq)
    b.extract(3)
    b.ground(3)
    odom = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    kw = dict(corner=True, sliding_window_size=2, feature_capacity=4096)
    hit = own(pkg.mapping.MapOptimization(ctx, 0.4, 0.2, **kw))
    clean = own(pkg.mapping.MapOptimization(ctx, 0.4, 0.2, **kw))
    for m in (hit, clean):  # the first step builds the map and pushes nothing
        m.callback_batch(b, 0, odom, nfeatures=n)
    got = full_or_capacity(pkg, lambda: hit.callback_batch(b, 1, odom, nfeatures=n))
    if got is not None:
        _, rde, rp3 = C.map_filter_reference(oracle, f1.img_intensity, f1.cloud_track, n, None)
        d, p, _ = hit.window.keyframe(len(hit.window) - 1)
        assert d.shape == rde.shape and np.array_equal(d, rde) and np.array_equal(p[:, :3], rp3)
    else:
        assert len(hit.window) == 0 and hit.state.tobytes() == clean.state.tobytes()
        ph, sh = hit.callback_batch(b, 2, odom, nfeatures=n)
        pc, sc = clean.callback_batch(b, 2, odom, nfeatures=n)
        assert ph.tobytes() == pc.tobytes() and list(sh) == list(sc) and hit.state.tobytes() == clean.state.tobytes()
        assert len(hit.window) == len(clean.window) == 1
        dh, p_h, _ = hit.window.keyframe(0)
        dc, p_c, _ = clean.window.keyframe(0)
        assert len(dh) > 0 and np.array_equal(dh, dc) and np.array_equal(p_h, p_c)
