"""GPU parity of the Scan Context place database (lislam_place_*: k_sc_describe, k_sc_finish,
k_sc_detect, k_sc_distance) against the stateful numpy restatement of the reference's SCManager
(tests/restate_sc.py).

Everything is compared by equality: descriptors, ring and sector keys, nn_idx, nn_align, loop_id,
yaw, and min_dist as doubles.  The kernels and the restatement run the same floating-point
operations in the same fixed order (see lislam_place.hip's header), so nothing needs a tolerance."""
import ctypes
import math

import numpy as np
import pytest

import place_cases as PC
import restate_sc as SC
from loop_cases import pose_T

pytestmark = pytest.mark.gpu

SHORT = dict(num_exclude_recent=5, tree_making_period=4, num_candidates=3, search_ratio=1.0)


@pytest.fixture(scope="module")
def ctx16(pkg):
    c = pkg.Context(n_scans=16, width=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx64(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


def _extract(pkg, ctx, scans):
    """A batch holding the extracted scans and their downloaded cloud_track."""
    b = pkg.Batch(ctx, scans.shape[0])
    b.upload(scans)
    b.extract(scans.shape[0])
    return b, [b.download(pkg.native.OUT_CLOUD_TRACK, k) for k in range(scans.shape[0])]


@pytest.fixture(scope="module")
def drive(pkg, synth, ctx16):
    """The there-and-back drive, extracted: (batch, cloud_track of its 120 keyframes)."""
    b, tracks = _extract(pkg, ctx16, PC.there_and_back(synth))
    yield b, tracks
    b.close()


def _entry_equals(sc, i, desc):
    assert np.array_equal(sc.descriptor(i), desc), i
    assert np.array_equal(sc.ring_key(i), SC.ring_key(desc)), i
    assert np.array_equal(sc.sector_key(i), SC.sector_key(desc)), i


def _entry_bytes(sc, i):
    return sc.descriptor(i).tobytes() + sc.ring_key(i).tobytes() + sc.sector_key(i).tobytes()


@pytest.mark.parametrize("shape", [(8, 16, 256), (2, 64, 1024)])
def test_descriptors_of_a_batch(pkg, synth, ctx16, ctx64, shape):
    """add_batch reads cloud_track on the device: byte-equal to add of the downloaded clouds, and
    equal to the restatement.  64x1024 takes several workgroups per cloud."""
    n, H, W = shape
    ctx = ctx16 if H == 16 else ctx64
    b, tracks = _extract(pkg, ctx, synth.make_sequence(n, H, W))
    dev, host = pkg.ScanContext(ctx, capacity=n + 2), pkg.ScanContext(ctx, capacity=n)
    dev.add_batch(b, 0, n)
    dev.add_batch(b, n - 2, 2)  # a range that starts inside the batch
    host.add(tracks)
    assert len(dev) == n + 2 and len(host) == n
    for k in range(n):
        desc = SC.make_scancontext(tracks[k])
        assert desc[0, 0] >= 2.0  # the dropouts (0, 0, 0) land in bin (0, 0) with lidar_height
        _entry_equals(dev, k, desc)
        assert _entry_bytes(dev, k) == _entry_bytes(host, k)
    for k in (n - 2, n - 1):
        assert _entry_bytes(dev, k + 2) == _entry_bytes(host, k)
    for o in (dev, host, b):
        o.close()


@pytest.mark.parametrize("cfg", [{}, dict(num_ring=40, num_sector=120), dict(num_ring=7, num_sector=13, max_radius=55.5,
                                                                              lidar_height=-0.25)])
def test_descriptor_special_cases(pkg, synth, ctx16, cfg):
    """Points beyond max_radius, duplicates, NaN height / x / y, axes and diagonals, -0.0, dropouts,
    the radius boundary, a height of exactly NO_POINT; an empty cloud; a 64x1024 scan in the same
    call, so the small clouds meet a launch shaped for the large one."""
    full = dict(SC.DEFAULTS, **cfg)
    tricky = PC.tricky_cloud()
    clouds = [tricky, np.zeros((0, 4), np.float32), synth.make_scan(3).reshape(-1, 4), tricky[:300], tricky[::-1]]
    sc = pkg.ScanContext(ctx16, capacity=8, **cfg)
    sc.add(clouds)
    sc.add([tricky[:1]])
    assert len(sc) == 6
    for k, c in enumerate(clouds + [tricky[:1]]):
        _entry_equals(sc, k, SC.make_scancontext(c, full))
    assert not sc.descriptor(1).any() and not sc.ring_key(1).any() and not sc.sector_key(1).any()
    assert _entry_bytes(sc, 0) == _entry_bytes(sc, 4)  # the maximum does not depend on the order of the points
    if not cfg:
        d = sc.descriptor(0)
        special = np.array(PC.AXES_AND_DIAGONALS, np.float32)
        keep, ring, sector, _ = SC.bins(special)
        assert list(sector + 1) == [15, 30, 45, 60, 8, 23, 38, 53] and np.all(d[ring, sector] >= 2.0)
        assert d[19, 0] >= 6.0  # (80, 0, 4): exactly max_radius is kept
        assert d.max() < 100.0  # one float above it (height 400) and the point at infinity are dropped
    sc.close()


@pytest.fixture(scope="module")
def mixed_db(pkg, drive, ctx16):
    """Descriptors of every kind above in one database, with their restated descriptors."""
    tricky = PC.tricky_cloud()
    clouds = [tricky, np.zeros((0, 4), np.float32), tricky[:400], tricky[2000:3000]] + drive[1][::6]
    sc = pkg.ScanContext(ctx16, capacity=len(clouds))
    sc.add(clouds)
    yield sc, [SC.make_scancontext(c) for c in clouds]
    sc.close()


def test_pair_distance(mixed_db):
    sc, descs = mixed_db
    rng = np.random.default_rng(17)
    n = len(descs)
    a = np.concatenate([rng.integers(0, n, 200), [1, 1, 0]]).astype(np.int32)
    b = np.concatenate([rng.integers(0, n, 200), [1, 0, 1]]).astype(np.int32)
    dist, shift = sc.distance(a, b)
    ref = [SC.distance_btn_scancontext(descs[i], descs[j]) for i, j in zip(a, b)]
    assert np.array_equal(dist, np.array([r[0] for r in ref]))
    assert np.array_equal(shift, np.array([r[1] for r in ref], np.int32))
    assert (dist[200], shift[200]) == (1e7, 0)  # two all-zero descriptors: no column counts, NaN never wins
    assert np.all(dist[201:] == 1e7) and np.count_nonzero(dist[:200] < 1e7) > 150


def test_add_clouds_device_resident_points(pkg, drive, ctx16):
    """Points already in HBM (a torch tensor) give what the same points give from host memory."""
    import torch

    tracks = drive[1][:3]
    host = pkg.ScanContext(ctx16, capacity=3)
    host.add(tracks)
    dev = pkg.ScanContext(ctx16, capacity=3)
    pts = torch.from_numpy(np.concatenate(tracks)).cuda()
    counts = np.array([t.shape[0] for t in tracks], np.int32)
    torch.cuda.synchronize()
    rc = ctx16.lib.lislam_place_add_clouds(dev.h, ctypes.c_void_p(pts.data_ptr()), pkg.native.ptr(counts), 3)
    assert rc == 0 and len(dev) == 3
    for k in range(3):
        assert _entry_bytes(dev, k) == _entry_bytes(host, k)
    host.close()
    dev.close()


def _restate_sequence(clouds, cfg):
    """One make_and_save + detect per keyframe through the stateful restatement."""
    m = SC.SCManager(**cfg)
    rows, gaps = [], []
    for c in clouds:
        m.make_and_save(c)
        loop_id, yaw = m.detect()
        rows.append((loop_id, yaw, m.last["min_dist"], m.last["nn_idx"], m.last["nn_align"]))
        d = sorted(x[1] for x in m.last["cands"] if x[1] == x[1])
        gaps.append(d[1] - d[0] if len(d) > 1 else math.inf)
    cols = list(zip(*rows))
    return (np.array(cols[0], np.int32), np.array(cols[1], np.float32), np.array(cols[2], np.float64),
            np.array(cols[3], np.int32), np.array(cols[4], np.int32)), np.array(gaps)


@pytest.fixture(scope="module")
def drive_restated(drive):
    return {name: _restate_sequence(drive[1], cfg) for name, cfg in (("default", {}), ("short", SHORT))}


@pytest.mark.parametrize("name", ["default", "short"])
def test_sequence_detect(pkg, drive, drive_restated, ctx16, name):
    """detect(0, 120) in one launch == 120 make_and_save_and_detect calls == the stateful restatement."""
    cfg = {} if name == "default" else SHORT
    batch, tracks = drive
    (loop_id, yaw, min_dist, nn_idx, nn_align), gaps = drive_restated[name]
    # equal nn_idx rests on no exact distance tie between a query's best two candidates
    tied = gaps == 0
    assert tied.mean() <= 0.02
    once = pkg.ScanContext(ctx16, capacity=120, **cfg)
    once.add_batch(batch, 0, 120)
    got = once.detect(0, 120)
    step = pkg.ScanContext(ctx16, capacity=120, **cfg)
    calls = [step.make_and_save_and_detect(c) for c in tracks]
    assert np.array_equal(got.loop_id, np.array([c[0] for c in calls], np.int32))
    assert np.array_equal(got.yaw, np.array([c[1] for c in calls], np.float32))
    later = step.detect()  # the closed-form prefix replays what each call saw
    for x, y in zip(got, later):
        assert np.array_equal(x, y)
    assert np.array_equal(got.min_dist, min_dist)
    assert np.array_equal(got.nn_align[~tied], nn_align[~tied])
    assert np.array_equal(got.yaw[~tied], yaw[~tied])
    assert np.array_equal(got.nn_idx[~tied], nn_idx[~tied])
    assert np.array_equal(got.loop_id[~tied], loop_id[~tied])
    part = once.detect(100, 7)
    assert np.array_equal(part.nn_idx, got.nn_idx[100:107]) and np.array_equal(part.min_dist, got.min_dist[100:107])
    E = SC.DEFAULTS["num_exclude_recent"] if name == "default" else SHORT["num_exclude_recent"]
    assert np.all(got.loop_id[:E] == -1) and np.all(got.yaw[:E] == 0) and np.all(got.min_dist[:E] == 1e7)
    if name == "default":
        # keyframe 119 stands where keyframe 0 stood, turned by pi: 30 of 60 sectors
        assert got.loop_id[119] == 0 and got.nn_align[119] == 30 and got.yaw[119] == np.float32(math.pi)
        assert 0.002 < got.min_dist[119] < 0.004 < 0.13
    once.close()
    step.close()


def test_long_prefix_and_equal_keys(pkg, drive, ctx16):
    """A prefix longer than the workgroup, every candidate slot in use, a ring count that is no
    multiple of 4 (nanoflann's scalar tail), and a database that holds every cloud three times, so
    equal key distances must come out by lower index."""
    cfg = dict(num_ring=18, num_exclude_recent=5, tree_making_period=1, num_candidates=32)
    clouds = drive[1] * 3
    sc = pkg.ScanContext(ctx16, capacity=len(clouds), **cfg)
    sc.add(clouds)
    first = len(clouds) - 6
    got = sc.detect(first, 6)
    m = SC.SCManager(**cfg)
    descs = [SC.make_scancontext(c, m.cfg) for c in drive[1]] * 3
    for k, desc in enumerate(descs):
        m.save(desc)
        r = m.detect(search=k >= first)
        if k >= first:
            j = k - first
            assert m.last["prefix"] == k + 1 - 5 > 256
            assert (got.loop_id[j], got.yaw[j], got.min_dist[j], got.nn_idx[j], got.nn_align[j]) == \
                (r[0], r[1], m.last["min_dist"], m.last["nn_idx"], m.last["nn_align"]), k
            assert got.nn_idx[j] == k - 240 and abs(got.min_dist[j]) < 1e-12  # its first copy, not the later one
    sc.close()


def test_hand_off_to_loop_icp(pkg, oracle, synth, drive, ctx16):
    """(loop_id, yaw) of keyframe 119 as hist and initial yaw of loop_closure_icp: the two stages compose."""
    batch, tracks = drive
    sc = pkg.ScanContext(ctx16, capacity=120)
    sc.add_batch(batch, 0, 120)
    d = sc.detect(119, 1)
    sc.close()
    loop_id, yaw = int(d.loop_id[0]), float(d.yaw[0])
    assert loop_id == 0
    # circshift(candidate, nn_align) matches the query: the query's heading is the candidate's minus yaw
    c, s = math.cos(-yaw), math.sin(-yaw)
    Rz = np.eye(4)
    Rz[:2, :2] = [[c, -s], [s, c]]
    T_hist = pose_T(PC.drive_pose(synth, loop_id))
    T_cur = T_hist @ Rz
    ref = oracle.loop_icp(tracks[119], T_cur, [tracks[loop_id]], [T_hist])
    got = pkg.loop.loop_closure_icp(ctx16, tracks[119], T_cur, [tracks[loop_id]], [T_hist])
    assert list(got[3]) == list(ref[3])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert got[3][0] == pkg.loop.ACCEPTED


def test_argument_errors_leave_the_database_unchanged(pkg, synth, drive, ctx16):
    n = pkg.native
    lib = ctx16.lib
    batch, tracks = drive
    sc = pkg.ScanContext(ctx16, capacity=3)
    sc.add(tracks[:2])
    before = _entry_bytes(sc, 0) + _entry_bytes(sc, 1)

    def err():
        return lib.lislam_last_error(ctx16.h).decode()

    two = np.ascontiguousarray(np.concatenate(tracks[2:4]))
    counts = np.array([tracks[2].shape[0], tracks[3].shape[0]], np.int32)
    assert lib.lislam_place_add_clouds(sc.h, n.ptr(two), n.ptr(counts), 2) == n.ERR_CAPACITY and "capacity" in err()
    assert lib.lislam_place_add_batch(sc.h, batch.h, 0, 2) == n.ERR_CAPACITY and "capacity" in err()
    assert lib.lislam_place_add_batch(sc.h, batch.h, 119, 2) == n.ERR_ARG and "range" in err()
    assert lib.lislam_place_add_batch(sc.h, batch.h, -1, 1) == n.ERR_ARG
    bad = np.array([5, -1], np.int32)
    assert lib.lislam_place_add_clouds(sc.h, n.ptr(two), n.ptr(bad), 2) == n.ERR_ARG
    out = np.zeros(1200)
    cnt = ctypes.c_int32()
    for what, idx in ((n.PLACE_DESC, 2), (n.PLACE_DESC, -1), (7, 0)):
        assert lib.lislam_place_download(sc.h, what, idx, n.ptr(out), 1200, ctypes.byref(cnt)) == n.ERR_ARG and err()
    assert lib.lislam_place_download(sc.h, n.PLACE_DESC, 0, n.ptr(out), 100, ctypes.byref(cnt)) == n.ERR_CAPACITY
    assert cnt.value == 1200
    assert lib.lislam_place_detect(sc.h, 1, 2, None, None, None, None, None) == n.ERR_ARG and "range" in err()
    assert lib.lislam_place_detect(sc.h, -1, 1, None, None, None, None, None) == n.ERR_ARG
    ia, ib = np.array([0, 2], np.int32), np.array([1, 0], np.int32)
    assert lib.lislam_place_distance(sc.h, n.ptr(ia), n.ptr(ib), 2, None, None) == n.ERR_ARG and "range" in err()
    # a batch of another context
    other = pkg.Context(n_scans=16, width=256)
    ob = pkg.Batch(other, 1)
    ob.upload(synth.make_sequence(1, 16, 256))
    ob.extract(1)
    assert lib.lislam_place_add_batch(sc.h, ob.h, 0, 1) == n.ERR_ARG and "another context" in err()
    ob.close()
    other.close()
    # a batch that was not extracted that far, and one without cloud_track
    fresh = pkg.Batch(ctx16, 2)
    assert lib.lislam_place_add_batch(sc.h, fresh.h, 0, 1) == n.ERR_STATE
    fresh.close()
    bare = pkg.Context(n_scans=16, width=256, want_images=False)
    bsc, bb = pkg.ScanContext(bare, capacity=1), pkg.Batch(bare, 1)
    assert lib.lislam_place_add_batch(bsc.h, bb.h, 0, 1) == n.ERR_STATE
    for o in (bsc, bb, bare):
        o.close()
    # unsupported configurations
    h = ctypes.c_void_p()
    for kw in (dict(num_ring=41), dict(num_ring=0), dict(num_sector=121), dict(num_sector=0), dict(num_candidates=33),
               dict(num_candidates=0), dict(tree_making_period=0), dict(num_exclude_recent=-1), dict(max_radius=0.0)):
        cfg = n.PlaceConfig(**kw)
        assert lib.lislam_place_create(ctx16.h, ctypes.byref(cfg), 4, ctypes.byref(h)) == n.ERR_ARG, kw
    assert lib.lislam_place_create(ctx16.h, None, 0, ctypes.byref(h)) == n.ERR_ARG
    with pytest.raises(n.LislamError):
        sc.add(tracks[2:4])
    # nothing above changed the database, and it still takes what fits
    assert len(sc) == 2 and _entry_bytes(sc, 0) + _entry_bytes(sc, 1) == before
    sc.add(tracks[2:3])
    assert len(sc) == 3
    _entry_equals(sc, 2, SC.make_scancontext(tracks[2]))
    d = sc.detect()
    assert list(d.loop_id) == [-1, -1, -1]
    sc.close()
