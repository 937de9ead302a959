"""GPU checks of keyframe selection (lislam_keysel_*: k_keysel) against its literal restatement
(tests/restate_keysel.py), and of the feeds that take a list of scans
(lislam_keyframes_add_batch_scans: k_kf_gather; lislam_place_add_batch_scans;
lislam_bow_add_batch_scans: k_bow_scan_list; lislam_pgo_add_keyframes / lislam_pgo_add_batch_scans:
k_pgo_add_keyframes) against the single-scan range calls they are defined by.

Selection is compared by equality: the kernel and the restatement run the same double operations in
the same order, and tests/test_keysel_cpu.py keeps every gate comparison 1e-9 away from its threshold.
keyframe_id, n_selected and the node rows must match exactly; T_s2m as doubles.  The list feeds are
compared in bytes with a second object fed by single-scan calls.  The pose graph's measurements are
held to 1e-12 against restate_pgo.between, the bound tests/test_gpu_pgo.py::test_add_batch uses for the
range form."""
import ctypes
import math

import numpy as np
import pytest

import bow_cases as BC
import keysel_cases as KC
import pgo_cases as C
import restate_keysel as RK
import restate_pgo as PG

pytestmark = pytest.mark.gpu

CASES = KC.cases()
VAR = np.array(PG.ODOMETRY_VARIANCES)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx16(pkg):
    c = pkg.Context(n_scans=16, width=256)
    yield c
    c.close()


def _same(got, ref):
    ids, T, nodes = got
    rids, rT, rnodes = ref
    assert ids.dtype == np.int32 and np.array_equal(ids, rids)
    assert nodes.shape == rnodes.shape and nodes.tobytes() == rnodes.tobytes()  # n_selected and the rows
    assert T.shape == rT.shape and np.array_equal(T, rT)


def _same_state(sel, r):
    n, T, t = sel.state()
    assert n == r.next_id and np.array_equal(T, np.array(r.T))
    assert math.isnan(t) if r.last_time is None else t == r.last_time


# ---------------------------------------------------------------- selection from arrays
@pytest.mark.parametrize("name", sorted(CASES))
def test_selection_equals_the_restatement(pkg, ctx, name):
    c = CASES[name]
    r = RK.Selector(c.time_interval, c.distance_interval)
    ref = r.step(c.T_s2s, c.good, c.times)
    if c.expected is not None:
        assert list(ref[0]) == list(c.expected)
    sel = pkg.KeyframeSelector(ctx, c.time_interval, c.distance_interval)
    _same(sel.step(c.T_s2s, c.good, c.times), ref)
    _same_state(sel, r)
    sel.close()


def test_inputs_in_device_memory(pkg, ctx):
    import torch

    c = CASES["random65"]
    ref = RK.Selector(c.time_interval, c.distance_interval).step(c.T_s2s, c.good, c.times)
    T_dev, good_dev = torch.from_numpy(c.T_s2s).cuda(), torch.from_numpy(c.good).cuda()
    torch.cuda.synchronize()
    for T, good in ((T_dev, c.good), (c.T_s2s, good_dev), (T_dev, good_dev)):
        sel = pkg.KeyframeSelector(ctx, c.time_interval, c.distance_interval)
        _same(sel.step(T, good, c.times), ref)
        sel.close()


@pytest.mark.parametrize("cuts", [(1,), (32,), tuple(range(1, 65))], ids=["1+64", "32+33", "65x1"])
def test_split_invariance(pkg, ctx, cuts):
    c = CASES["random65"]
    r = RK.Selector(c.time_interval, c.distance_interval)
    ref = r.step(c.T_s2s, c.good, c.times)
    whole = pkg.KeyframeSelector(ctx, c.time_interval, c.distance_interval)
    _same(whole.step(c.T_s2s, c.good, c.times), ref)
    sel = pkg.KeyframeSelector(ctx, c.time_interval, c.distance_interval)
    edges = (0,) + cuts + (65,)
    parts = [sel.step(c.T_s2s[a:b], c.good[a:b], c.times[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    _same(tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), ref)
    _same_state(sel, r)  # the state of the single call
    _same_state(whole, r)
    sel.close()
    whole.close()


def test_selector_rejects_bad_arguments(pkg, ctx):
    nat = pkg.native
    h = ctypes.c_void_p()
    bad = nat.KeyselConfig(float("nan"), 0.3)
    assert ctx.lib.lislam_keysel_create(ctx.h, ctypes.byref(bad), ctypes.byref(h)) == nat.ERR_ARG
    sel = pkg.KeyframeSelector(ctx)
    assert (sel.cfg.time_interval, sel.cfg.distance_interval) == (0.3, 0.3)
    t = np.zeros(1)
    assert ctx.lib.lislam_keysel_step(sel.h, None, None, nat.ptr(t), 1, None, None, None, None) == nat.ERR_ARG
    assert ctx.lib.lislam_keysel_step(sel.h, None, None, None, -1, None, None, None, None) == nat.ERR_ARG
    n = ctypes.c_int32(7)
    assert ctx.lib.lislam_keysel_step(sel.h, None, None, None, 0, None, ctypes.byref(n), None, None) == 0 and n.value == 0
    assert sel.state()[0] == 0
    sel.close()


# ---------------------------------------------------------------- selection from a batch
N_BATCH = 10
TIMES = 50.0 + 0.1037 * np.arange(N_BATCH)


@pytest.fixture(scope="module")
def orb_batch(pkg, synth, ctx):
    """10 scans of 64x1024, extracted; the selector's answer before the ORB front end has run; then that run."""
    nat = pkg.native
    b = pkg.Batch(ctx, N_BATCH)
    b.upload(synth.make_sequence(N_BATCH, 64, 1024))
    b.extract(N_BATCH)
    sel = pkg.KeyframeSelector(ctx)
    ids = np.zeros(N_BATCH, np.int32)
    early = ctx.lib.lislam_keysel_step_batch(sel.h, b.h, 0, N_BATCH, nat.ptr(TIMES), nat.ptr(ids), None, None, None)
    early_text = ctx.lib.lislam_last_error(ctx.h).decode()
    assert sel.state()[0] == 0
    sel.close()
    b.intensity_odometry(N_BATCH, 1000)
    T = np.array([b.download(nat.OUT_ORB_T, k) for k in range(N_BATCH)]).reshape(N_BATCH, 7)
    stats = np.array([b.download(nat.OUT_ORB_STATS, k) for k in range(N_BATCH)]).reshape(N_BATCH, 8)
    yield b, T, stats, (early, early_text)
    b.close()


def _thresholds(T, good):
    """Thresholds from the downloaded trajectory: the first pair, among a few multiples of the frame gap
    and of the median step, for which the restatement selects 2 to 5 keyframes with the 1e-9 margins."""
    step = float(np.median(np.linalg.norm(T[good == 1, 4:], axis=1)))
    for ti in (0.05, 0.15, 0.25):
        for f in (0.5, 1.5, 2.5, 3.5):
            r = RK.Selector(ti, f * step)
            ids, _, _ = r.step(T, good, TIMES)
            if 2 <= int((ids >= 0).sum()) <= 5 and min(r.margins()) > KC.MARGIN:
                return ti, f * step
    return None


def test_selection_from_a_batch(pkg, ctx, orb_batch):
    b, T, stats, _ = orb_batch
    good = (stats[:, 0] == 1).astype(np.int32)
    print("good", list(stats[:, 0]), "steps", np.linalg.norm(T[:, 4:], axis=1))
    assert good.sum() >= 2
    th = _thresholds(T, good)
    assert th is not None
    r = RK.Selector(*th)
    ref = r.step(T, good, TIMES)
    assert 2 <= ref[2].shape[0] <= 5 and min(r.margins()) > KC.MARGIN
    whole = pkg.KeyframeSelector(ctx, *th)
    _same(whole.step_batch(b, 0, N_BATCH, TIMES), ref)
    _same_state(whole, r)
    halves = pkg.KeyframeSelector(ctx, *th)
    parts = [halves.step_batch(b, 0, 4, TIMES[:4]), halves.step_batch(b, 4, 6, TIMES[4:])]
    _same(tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), ref)
    _same_state(halves, r)
    halves.close()
    whole.close()


def test_selection_from_a_batch_errors(pkg, synth, ctx, ctx16, orb_batch):
    nat = pkg.native
    b, _, _, (early, early_text) = orb_batch
    assert early == nat.ERR_STATE and "lislam_batch_intensity_odometry" in early_text
    sel = pkg.KeyframeSelector(ctx)
    ids = np.zeros(N_BATCH + 1, np.int32)
    t = np.zeros(N_BATCH + 1)
    call = lambda *a: ctx.lib.lislam_keysel_step_batch(sel.h, b.h, *a, nat.ptr(t), nat.ptr(ids), None, None, None)  # noqa: E731
    assert call(0, N_BATCH + 1) == nat.ERR_ARG and b"out of range" in ctx.lib.lislam_last_error(ctx.h)
    assert call(-1, 2) == nat.ERR_ARG and call(3, -1) == nat.ERR_ARG and call(N_BATCH, 1) == nat.ERR_ARG
    other = pkg.KeyframeSelector(ctx16)  # a selector of another context
    assert ctx16.lib.lislam_keysel_step_batch(other.h, b.h, 0, 2, nat.ptr(t), nat.ptr(ids), None, None, None) == nat.ERR_ARG
    assert b"another context" in ctx16.lib.lislam_last_error(ctx16.h)
    # the ORB front end ran over fewer scans than asked for
    b2 = pkg.Batch(ctx, 4)
    b2.upload(synth.make_sequence(4, 64, 1024))
    b2.extract(4)
    b2.intensity_odometry(3, 1000)
    assert ctx.lib.lislam_keysel_step_batch(sel.h, b2.h, 0, 4, nat.ptr(t), nat.ptr(ids), None, None, None) == nat.ERR_STATE
    n = ctypes.c_int32(-5)
    assert ctx.lib.lislam_keysel_step_batch(sel.h, b2.h, 1, 0, None, None, ctypes.byref(n), None, None) == 0 and n.value == 0
    assert sel.state()[0] == 0 and other.state()[0] == 0
    for o in (b2, other, sel):
        o.close()


# ---------------------------------------------------------------- the feeds that take a list of scans
N_FEED = 6
LISTS = ([4], [0, 2, 5], [5, 0, 0], [])


@pytest.fixture(scope="module")
def feed_batch(pkg, synth, ctx):
    b = pkg.Batch(ctx, N_FEED)
    b.upload(synth.make_sequence(N_FEED, 64, 1024))
    b.extract(N_FEED)
    b.intensity_odometry(N_FEED, 1000)
    yield b
    b.close()


@pytest.fixture(scope="module")
def raw_batch(pkg, synth, ctx):
    """Uploaded, not extracted."""
    b = pkg.Batch(ctx, N_FEED)
    b.upload(synth.make_sequence(N_FEED, 64, 1024))
    yield b
    b.close()


def _ptr(pkg, a):
    return pkg.native.ptr(np.ascontiguousarray(a, np.int32))


def _err(ctx):
    return ctx.lib.lislam_last_error(ctx.h).decode()


def test_keyframe_pool_list_feed(pkg, ctx, feed_batch, raw_batch):
    nat, b = pkg.native, feed_batch
    N = 64 * 1024
    total = sum(len(s) for s in LISTS)
    got, ref = pkg.KeyframePool(ctx, total, total * N), pkg.KeyframePool(ctx, total, total * N)
    for scans in LISTS:
        got.add_batch_scans(b, scans)
        for s in scans:
            ref.add_batch(b, s, 1)
        assert got.size() == ref.size()
    assert got.size() == (total, total * N)
    clouds = [got.cloud(i) for i in range(total)]
    assert all(clouds[i].tobytes() == ref.cloud(i).tobytes() for i in range(total))
    flat = [s for scans in LISTS for s in scans]
    assert all(clouds[i].tobytes() == b.download(nat.OUT_CLOUD_TRACK, flat[i]).tobytes() for i in (0, 3, 6))
    assert clouds[0].tobytes() != clouds[1].tobytes()
    # errors: nothing is added, the text names the entry
    small = pkg.KeyframePool(ctx, 2, 8 * N)
    short = pkg.KeyframePool(ctx, 8, 3 * N - 1)
    call = lambda p, bb, s: ctx.lib.lislam_keyframes_add_batch_scans(p.h, bb.h, _ptr(pkg, s), len(s))  # noqa: E731
    assert call(small, b, [0, 6]) == nat.ERR_ARG and "scans[1] = 6" in _err(ctx)
    assert call(small, b, [-1]) == nat.ERR_ARG and "scans[0] = -1" in _err(ctx)
    assert call(small, raw_batch, [0]) == nat.ERR_STATE and "extract" in _err(ctx)
    assert call(small, b, [0, 1, 2]) == nat.ERR_CAPACITY and "0 + 3 keyframes exceed the capacity 2" in _err(ctx)
    assert call(short, b, [0, 1, 2]) == nat.ERR_CAPACITY and "points exceed the capacity" in _err(ctx)
    assert small.size() == (0, 0) and short.size() == (0, 0)
    small.add_batch_scans(b, [1, 1])  # exactly full
    assert small.size() == (2, 2 * N) and call(small, b, [0]) == nat.ERR_CAPACITY and small.size() == (2, 2 * N)
    for o in (got, ref, small, short):
        o.close()


def test_scan_context_list_feed(pkg, ctx, feed_batch, raw_batch):
    nat, b = pkg.native, feed_batch
    total = sum(len(s) for s in LISTS)
    got, ref = pkg.ScanContext(ctx, capacity=total), pkg.ScanContext(ctx, capacity=total)
    for scans in LISTS:
        got.add_batch_scans(b, scans)
        for s in scans:
            ref.add_batch(b, s, 1)
        assert len(got) == len(ref)
    assert len(got) == total
    for i in range(total):
        for get in ("descriptor", "ring_key", "sector_key"):
            assert getattr(got, get)(i).tobytes() == getattr(ref, get)(i).tobytes(), (i, get)
    assert got.descriptor(0).any() and got.descriptor(0).tobytes() != got.descriptor(1).tobytes()
    small = pkg.ScanContext(ctx, capacity=2)
    call = lambda p, bb, s: ctx.lib.lislam_place_add_batch_scans(p.h, bb.h, _ptr(pkg, s), len(s))  # noqa: E731
    assert call(small, b, [0, 6]) == nat.ERR_ARG and "scans[1] = 6" in _err(ctx)
    assert call(small, b, [-1]) == nat.ERR_ARG and "scans[0] = -1" in _err(ctx)
    assert call(small, raw_batch, [0]) == nat.ERR_STATE and "extract" in _err(ctx)
    assert call(small, b, [0, 1, 2]) == nat.ERR_CAPACITY and "exceed the capacity 2" in _err(ctx)
    assert len(small) == 0
    for o in (got, ref, small):
        o.close()


def test_bag_of_words_list_feed(pkg, ctx, feed_batch, raw_batch):
    nat, b = pkg.native, feed_batch
    voc = BC.vocabulary("k10L3")
    total = sum(len(s) for s in LISTS)
    got = pkg.BowDatabase(ctx, *voc, capacity=total, max_features=1000)
    ref = pkg.BowDatabase(ctx, *voc, capacity=total, max_features=1000)
    for scans in LISTS:
        got.add_batch_scans(b, scans)
        for s in scans:
            ref.add_batch(b, s, 1)
        assert len(got) == len(ref)
    assert len(got) == total
    vecs = [got.bow_vector(i) for i in range(total)]
    for i in range(total):
        w, v = ref.bow_vector(i)
        assert vecs[i][0].tobytes() == w.tobytes() and vecs[i][1].tobytes() == v.tobytes(), i
    assert vecs[0][0].shape[0] > 0 and vecs[0][1].tobytes() != vecs[1][1].tobytes()
    small = pkg.BowDatabase(ctx, *voc, capacity=2, max_features=1000)
    call = lambda p, bb, s: ctx.lib.lislam_bow_add_batch_scans(p.h, bb.h, _ptr(pkg, s), len(s))  # noqa: E731
    assert call(small, b, [0, 6]) == nat.ERR_ARG and "scans[1] = 6" in _err(ctx)
    assert call(small, b, [-1]) == nat.ERR_ARG and "scans[0] = -1" in _err(ctx)
    assert call(small, raw_batch, [0]) == nat.ERR_STATE and "lislam_batch_intensity_odometry" in _err(ctx)
    assert call(small, b, [0, 1, 2]) == nat.ERR_CAPACITY and "exceed the capacity 2" in _err(ctx)
    assert len(small) == 0
    for o in (got, ref, small):
        o.close()


# ---------------------------------------------------------------- the pose graph's keyframe feed
N_PGO = 8


@pytest.fixture(scope="module")
def odom_batch(pkg, synth, ctx16):
    b = pkg.Batch(ctx16, N_PGO)
    b.upload(synth.make_sequence(N_PGO, 16, 256))
    b.extract(N_PGO)
    b.odometry(N_PGO, N_PGO - 1)
    pose = np.array([b.download(pkg.native.OUT_POSE, k) for k in range(N_PGO)]).reshape(N_PGO, 7)
    assert np.abs(pose[1:, 4:] - pose[:-1, 4:]).max() > 1e-3  # the odometry moved
    yield b, pose
    b.close()


KEYS = [0, 2, 5, 6, 7]


def _assert_keyframe_graph(g, pose):
    assert g.size() == (5, 4)
    assert g.poses().tobytes() == pose[KEYS].tobytes()
    i, j, z, var, robust = g.edges()
    assert list(i) == [0, 1, 2, 3] and list(j) == [1, 2, 3, 4] and not robust.any()
    assert np.allclose(var, VAR, rtol=1e-14, atol=0)
    for k in range(4):
        ref = PG.between(PG.normalized(pose[KEYS[k]]), PG.normalized(pose[KEYS[k + 1]]))
        assert np.abs(z[k] - ref).max() < 1e-12, k
    return z


def test_pose_graph_from_listed_scans(pkg, ctx16, odom_batch):
    b, pose = odom_batch
    g = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
    g.add_batch_scans(b, [0, 2, 5])
    assert g.size() == (3, 2)
    g.set_prior(0, pose[0])
    s = g.optimize()  # a prior and odometry only: the estimates barely move
    assert s.final_cost <= s.initial_cost
    g.add_batch_scans(b, [6, 7])
    # nodes 0..2 hold the optimiser's estimates now, the new ones their OUT_POSE rows
    assert g.poses(3, 2).tobytes() == pose[[6, 7]].tobytes()
    assert C.pose_gap(g.poses(0, 3), pose[[0, 2, 5]])[0] < 1e-9
    i, j, z, var, robust = g.edges()
    assert list(i) == [0, 1, 2, 3] and list(j) == [1, 2, 3, 4] and not robust.any()
    for k in range(4):
        ref = PG.between(PG.normalized(pose[KEYS[k]]), PG.normalized(pose[KEYS[k + 1]]))
        assert np.abs(z[k] - ref).max() < 1e-12, k
    # the whole list in one call gives the joining edge the same bytes: it is measured from pose[5] as added
    one = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
    one.add_batch_scans(b, KEYS)
    assert _assert_keyframe_graph(one, pose).tobytes() == z.tobytes()
    one.close()
    g.close()


def test_joining_edge_uses_the_pose_the_node_was_added_with(pkg, ctx16, odom_batch):
    """The prior pulls the whole chain 0.5 m sideways, so the last node's estimate is far from the pose it
    was added with; the next call's first edge still measures from the added pose (graph_prev_rotation_ /
    graph_prev_translation_, :513-514)."""
    b, pose = odom_batch
    g = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
    g.add_batch_scans(b, [0, 2, 5])
    moved = pose[0].copy()
    moved[5] += 0.5
    g.set_prior(0, moved)
    g.optimize()
    est = g.poses(2, 1)[0]
    assert abs(est[5] - pose[5][5] - 0.5) < 1e-3
    g.add_batch_scans(b, [6, 7])
    z = g.edges()[2][2]
    from_added = PG.between(PG.normalized(pose[5]), PG.normalized(pose[6]))
    from_estimate = PG.between(PG.normalized(est), PG.normalized(pose[6]))
    assert np.abs(z - from_added).max() < 1e-12 and np.abs(z - from_estimate).max() > 0.1
    g.close()


def test_add_keyframes_from_host_and_device(pkg, ctx16, odom_batch):
    import torch

    b, pose = odom_batch
    ref = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
    ref.add_batch_scans(b, [0, 2, 5])
    ref.add_batch_scans(b, [6, 7])
    z = _assert_keyframe_graph(ref, pose)
    dev = torch.from_numpy(pose).cuda()
    torch.cuda.synchronize()
    for poses in (pose, dev):
        g = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
        g.add_keyframes(poses, [0, 2, 5])
        g.add_keyframes(poses, [6, 7])
        assert _assert_keyframe_graph(g, pose).tobytes() == z.tobytes()
        g.close()
    # after add_nodes and after add_batch the next keyframe joins the last node as it was added
    for first in ("nodes", "batch"):
        g = pkg.PoseGraph(ctx16, node_capacity=5, edge_capacity=4)
        if first == "nodes":
            g.add_nodes(pose[[1, 4]])
        else:
            g.add_batch(b, 3, 2)
        g.add_keyframes(pose, [7])
        zz = g.edges()[2][-1]
        assert np.abs(zz - PG.between(PG.normalized(pose[4]), PG.normalized(pose[7]))).max() < 1e-12
        assert g.poses(2, 1).tobytes() == pose[[7]].tobytes()
        g.close()
    ref.close()


def test_pose_graph_list_errors(pkg, ctx, ctx16, odom_batch):
    nat = pkg.native
    b, pose = odom_batch
    g = pkg.PoseGraph(ctx16, node_capacity=3, edge_capacity=2)
    kf = lambda idx, n_poses=N_PGO: ctx16.lib.lislam_pgo_add_keyframes(  # noqa: E731
        g.h, nat.ptr(pose), n_poses, _ptr(pkg, idx), len(idx), None)
    bs = lambda idx: ctx16.lib.lislam_pgo_add_batch_scans(g.h, b.h, _ptr(pkg, idx), len(idx), None)  # noqa: E731
    for call in (kf, bs):
        assert call([2, 1]) == nat.ERR_ARG and "strictly increasing" in _err(ctx16)
        assert call([1, 1]) == nat.ERR_ARG and call([0, 8]) == nat.ERR_ARG and "[1] = 8" in _err(ctx16)
        assert call([-1, 2]) == nat.ERR_ARG
        assert call([0, 1, 2, 3]) == nat.ERR_CAPACITY and "exceed the capacity" in _err(ctx16)
        assert g.size() == (0, 0)
    assert kf([3], 3) == nat.ERR_ARG
    other = pkg.PoseGraph(ctx, node_capacity=3, edge_capacity=2)  # a graph of another context
    assert ctx.lib.lislam_pgo_add_batch_scans(other.h, b.h, _ptr(pkg, [0]), 1, None) == nat.ERR_ARG
    bad = np.array([1e-6, 0, 1, 1, 1, 1.0])
    assert ctx16.lib.lislam_pgo_add_keyframes(g.h, nat.ptr(pose), N_PGO, _ptr(pkg, [0]), 1, nat.ptr(bad)) == nat.ERR_ARG
    g.add_batch_scans(b, [])
    g.add_keyframes(pose, [])
    assert g.size() == (0, 0) and other.size() == (0, 0)
    var = VAR * 4
    g.add_batch_scans(b, [1, 3], var)
    assert np.allclose(g.edges()[3], var, rtol=1e-14, atol=0)
    other.close()
    g.close()


def test_range_form_is_unchanged(pkg, ctx16, odom_batch):
    """lislam_pgo_add_batch over the whole batch, as tests/test_gpu_pgo.py::test_add_batch expects it."""
    b, pose = odom_batch
    n = N_PGO
    g = pkg.PoseGraph(ctx16, node_capacity=n, edge_capacity=n)
    g.add_batch(b, 0, n)
    assert g.size() == (n, n - 1)
    assert g.poses().tobytes() == pose.tobytes()
    i, j, z, var, robust = g.edges()
    assert list(i) == list(range(n - 1)) and list(j) == list(range(1, n)) and not robust.any()
    assert np.allclose(var, VAR, rtol=1e-14, atol=0)
    for k in range(n - 1):
        assert np.abs(z[k] - PG.between(PG.normalized(pose[k]), PG.normalized(pose[k + 1]))).max() < 1e-12, k
    # consecutive scans through the list form: the same kernel arithmetic, the same bytes
    lst = pkg.PoseGraph(ctx16, node_capacity=n, edge_capacity=n)
    lst.add_batch_scans(b, list(range(n)))
    assert lst.poses().tobytes() == pose.tobytes() and lst.edges()[2].tobytes() == z.tobytes()
    lst.close()
    g.close()
