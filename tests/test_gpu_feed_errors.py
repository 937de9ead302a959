"""The argument checks of the ten batch feeds, through the C ABI: every entry point's bad-argument table
gives the status and the exact lislam_last_error text, one row per entry where two checks fail at once
pins which of them wins, and the valid range and list feeds equal single-scan range calls made in the
same order (the equality tests/test_gpu_backend.py relies on).  The shapes are the smallest the other
files use: a 16 x 256 batch of max_scans 4 with two scans extracted (and their odometry run, for the pose
graph), pools of capacity 2; the bag-of-words feeds that need ORB descriptors read a 2-scan 64 x 1024
batch, the shape of tests/test_gpu_bow.py."""
import ctypes

import numpy as np
import pytest

import bow_cases as BC

pytestmark = pytest.mark.gpu

N = 16 * 256
BAD_VAR = np.array([1e-6, 0, 1, 1, 1, 1.0])


@pytest.fixture(scope="module")
def ctx16(pkg):
    c = pkg.Context(n_scans=16, width=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(pkg, synth, ctx16):
    """max_scans 4, scans 0 and 1 extracted, their odometry run; no intensity odometry."""
    b = pkg.Batch(ctx16, 4)
    b.upload(synth.make_sequence(4, 16, 256))
    b.extract(2)
    b.odometry(2, 1)
    yield b
    b.close()


@pytest.fixture(scope="module")
def fresh(pkg, ctx16):
    """Nothing extracted."""
    b = pkg.Batch(ctx16, 2)
    yield b
    b.close()


@pytest.fixture(scope="module")
def foreign(pkg):
    """A batch of another context."""
    c = pkg.Context(n_scans=16, width=256)
    b = pkg.Batch(c, 1)
    yield b
    b.close()
    c.close()


@pytest.fixture(scope="module")
def orb(pkg, synth):
    """(context, 2-scan 64 x 1024 batch whose intensity odometry has run)."""
    c = pkg.Context(n_scans=64, width=1024)
    b = pkg.Batch(c, 2)
    b.upload(synth.make_sequence(2, 64, 1024))
    b.extract(2)
    b.intensity_odometry(2, 1000)
    yield c, b
    b.close()
    c.close()


def _list(pkg, scans):
    s = np.ascontiguousarray(scans, np.int32)
    return (pkg.native.ptr(s) if s.size else None), s  # the array is kept alive by the caller's tuple


def _table(ctx, rows):
    """rows: (call, expected status, expected text)."""
    for k, (call, code, text) in enumerate(rows):
        rc = call()
        got = ctx.lib.lislam_last_error(ctx.h).decode()
        assert (rc, got) == (code, text), k


def _range_rows(nat, who, fn, batch, foreign):
    """The checks every range feed starts with: fn(batch handle, first, n) -> status."""
    return [
        (lambda: fn(foreign.h, 0, 1), nat.ERR_ARG, f"{who}: the batch belongs to another context"),
        (lambda: fn(batch.h, -1, 1), nat.ERR_ARG, f"{who}: scans [-1, -1 + 1) out of range"),
        (lambda: fn(batch.h, 0, -1), nat.ERR_ARG, f"{who}: scans [0, 0 + -1) out of range"),
        (lambda: fn(batch.h, 4, 1), nat.ERR_ARG, f"{who}: scans [4, 4 + 1) out of range"),
        (lambda: fn(batch.h, 2**31 - 1, 1), nat.ERR_ARG, f"{who}: scans [2147483647, 2147483647 + 1) out of range"),
        # two at once: the context is checked before the range
        (lambda: fn(foreign.h, 4, 1), nat.ERR_ARG, f"{who}: the batch belongs to another context"),
    ]


def _scans_fn(pkg, lib_fn, pool, *tail):
    def fn(bh, scans):
        p, keep = _list(pkg, scans)
        return lib_fn(pool.h, bh, p, len(keep), *tail)
    return fn


# ---------------------------------------------------------------- keyframe pool, Scan Context
def _cloud_pool_errors(pkg, ctx16, batch, fresh, foreign, name, noun, make, bare_make):
    nat, lib = pkg.native, ctx16.lib
    pool = make(ctx16)
    rng_fn = lambda bh, first, n: getattr(lib, f"lislam_{name}_add_batch")(pool.h, bh, first, n)  # noqa: E731
    who = f"lislam_{name}_add_batch"
    _table(ctx16, _range_rows(nat, who, rng_fn, batch, foreign) + [
        (lambda: rng_fn(batch.h, 1, 2), nat.ERR_STATE, f"{who}: extract 3 scans first"),
        (lambda: rng_fn(fresh.h, 0, 1), nat.ERR_STATE, f"{who}: extract 1 scans first"),
        # two at once: 3 scans are more than were extracted and more than fit
        (lambda: rng_fn(batch.h, 0, 3), nat.ERR_STATE, f"{who}: extract 3 scans first"),
    ])
    lst_fn = _scans_fn(pkg, getattr(lib, f"lislam_{name}_add_batch_scans"), pool)
    who = f"lislam_{name}_add_batch_scans"
    _table(ctx16, [
        (lambda: lst_fn(foreign.h, [0]), nat.ERR_ARG, f"{who}: the batch belongs to another context"),
        (lambda: lst_fn(fresh.h, [0]), nat.ERR_STATE, f"{who}: extract the batch first"),
        (lambda: lst_fn(batch.h, [0, 2]), nat.ERR_ARG, f"{who}: scans[1] = 2 outside [0, 2)"),
        (lambda: lst_fn(batch.h, [-1]), nat.ERR_ARG, f"{who}: scans[0] = -1 outside [0, 2)"),
        # two at once: a scan out of bounds in a list longer than the capacity; nothing extracted and out of bounds
        (lambda: lst_fn(batch.h, [0, 1, 2]), nat.ERR_ARG, f"{who}: scans[2] = 2 outside [0, 2)"),
        (lambda: lst_fn(fresh.h, [7]), nat.ERR_STATE, f"{who}: extract the batch first"),
    ])
    assert lst_fn(batch.h, []) == nat.OK and lst_fn(fresh.h, []) == nat.OK and len(pool) == 0
    # without cloud_track: checked after the range, before the extraction
    bare = pkg.Context(n_scans=16, width=256, want_images=False)
    bpool, bb = bare_make(bare), pkg.Batch(bare, 1)
    text = "cloud_track not materialized (want_images=0)"
    _table(bare, [
        (lambda: getattr(lib, f"lislam_{name}_add_batch")(bpool.h, bb.h, 0, 1), nat.ERR_STATE, f"lislam_{name}_add_batch: {text}"),
        (lambda: getattr(lib, f"lislam_{name}_add_batch")(bpool.h, bb.h, 0, 2), nat.ERR_ARG,
         f"lislam_{name}_add_batch: scans [0, 0 + 2) out of range"),
        (lambda: _scans_fn(pkg, getattr(lib, f"lislam_{name}_add_batch_scans"), bpool)(bb.h, [0]), nat.ERR_STATE,
         f"lislam_{name}_add_batch_scans: {text}"),
    ])
    for o in (bpool, bb, bare):
        o.close()
    # full: exactly 2 fit, one more does not
    pool.add_batch(batch, 0, 2)
    assert len(pool) == 2
    _table(ctx16, [
        (lambda: rng_fn(batch.h, 0, 1), nat.ERR_CAPACITY, f"lislam_{name}_add_batch: 2 + 1 {noun} exceed the capacity 2"),
        (lambda: lst_fn(batch.h, [1]), nat.ERR_CAPACITY, f"lislam_{name}_add_batch_scans: 2 + 1 {noun} exceed the capacity 2"),
    ])
    assert len(pool) == 2 and rng_fn(batch.h, 1, 0) == nat.OK
    pool.close()


def _cloud_pool_feeds(ctx16, batch, make, entry):
    for feed, order in ((lambda p: p.add_batch(batch, 0, 2), (0, 1)), (lambda p: p.add_batch_scans(batch, [1, 0]), (1, 0))):
        got, ref = make(ctx16), make(ctx16)
        feed(got)
        for s in order:
            ref.add_batch(batch, s, 1)
        assert len(got) == len(ref) == 2
        assert [entry(got, i) for i in range(2)] == [entry(ref, i) for i in range(2)]
        assert entry(got, 0) != entry(got, 1)
        got.close()
        ref.close()


def test_keyframe_pool_feeds(pkg, ctx16, batch, fresh, foreign):
    make = lambda c: pkg.KeyframePool(c, 2, 2 * N)  # noqa: E731
    _cloud_pool_errors(pkg, ctx16, batch, fresh, foreign, "keyframes", "keyframes", make, make)
    _cloud_pool_feeds(ctx16, batch, make, lambda p, i: p.cloud(i).tobytes())


def _place_entry(p, i):
    return p.descriptor(i).tobytes() + p.ring_key(i).tobytes() + p.sector_key(i).tobytes()


def test_scan_context_feeds(pkg, ctx16, batch, fresh, foreign):
    make = lambda c: pkg.ScanContext(c, capacity=2)  # noqa: E731
    _cloud_pool_errors(pkg, ctx16, batch, fresh, foreign, "place", "entries", make, make)
    _cloud_pool_feeds(ctx16, batch, make, _place_entry)


def test_scan_context_staging_grows_between_calls(pkg, ctx16, batch):
    """The second add_clouds is larger than the first: the staging is reallocated behind the first call."""
    track = batch.download(pkg.native.OUT_CLOUD_TRACK, 0)
    small, big = track[:100], track
    two, a, b = (pkg.ScanContext(ctx16, capacity=2) for _ in range(3))
    two.add([small])
    two.add([big])
    a.add([small])
    b.add([big])
    assert _place_entry(two, 0) == _place_entry(a, 0) and _place_entry(two, 1) == _place_entry(b, 0)
    assert _place_entry(two, 0) != _place_entry(two, 1)
    for o in (two, a, b):
        o.close()


# ---------------------------------------------------------------- bag of words, its trainer
def _bow_entry(db, i):
    w, v = db.bow_vector(i)
    return w.tobytes() + v.tobytes()


def test_bag_of_words_feeds(pkg, ctx16, batch, foreign, orb):
    nat, lib = pkg.native, ctx16.lib
    voc = BC.vocabulary("k10L3")
    make = lambda c, **kw: pkg.BowDatabase(c, *voc, capacity=2, **kw)  # noqa: E731
    db = make(ctx16)
    rng_fn = lambda bh, first, n: lib.lislam_bow_add_batch(db.h, bh, first, n)  # noqa: E731
    lst_fn = _scans_fn(pkg, lib.lislam_bow_add_batch_scans, db)
    first = "run lislam_batch_intensity_odometry"
    _table(ctx16, _range_rows(nat, "lislam_bow_add_batch", rng_fn, batch, foreign) + [
        (lambda: rng_fn(batch.h, 0, 1), nat.ERR_STATE, f"lislam_bow_add_batch: {first} over 1 scans first"),
        (lambda: rng_fn(batch.h, 1, 0), nat.ERR_STATE, f"lislam_bow_add_batch: {first} over 1 scans first"),
        # two at once: no descriptors yet and more scans than fit
        (lambda: rng_fn(batch.h, 0, 3), nat.ERR_STATE, f"lislam_bow_add_batch: {first} over 3 scans first"),
        (lambda: lst_fn(foreign.h, [0]), nat.ERR_ARG, "lislam_bow_add_batch_scans: the batch belongs to another context"),
        (lambda: lst_fn(batch.h, [0]), nat.ERR_STATE, f"lislam_bow_add_batch_scans: {first} first"),
        # two at once: no descriptors yet and a scan out of bounds
        (lambda: lst_fn(batch.h, [9]), nat.ERR_STATE, f"lislam_bow_add_batch_scans: {first} first"),
        (lambda: lst_fn(batch.h, []), nat.ERR_STATE, f"lislam_bow_add_batch_scans: {first} first"),
    ])
    assert len(db) == 0
    db.close()
    # with descriptors: the batch of the 64 x 1024 context
    c, b = orb
    db, few = make(c), make(c, max_features=999)
    rng_fn = lambda bh, first, n: lib.lislam_bow_add_batch(db.h, bh, first, n)  # noqa: E731
    lst_fn = _scans_fn(pkg, lib.lislam_bow_add_batch_scans, db)
    _table(c, [
        (lambda: rng_fn(b.h, 1, 2), nat.ERR_ARG, "lislam_bow_add_batch: scans [1, 1 + 2) out of range"),
        (lambda: lst_fn(b.h, [0, 2]), nat.ERR_ARG, "lislam_bow_add_batch_scans: scans[1] = 2 outside [0, 2)"),
        (lambda: lst_fn(b.h, [-1]), nat.ERR_ARG, "lislam_bow_add_batch_scans: scans[0] = -1 outside [0, 2)"),
        # two at once: out of bounds in a list longer than the capacity; out of bounds and too many features
        (lambda: lst_fn(b.h, [0, 1, 2]), nat.ERR_ARG, "lislam_bow_add_batch_scans: scans[2] = 2 outside [0, 2)"),
        (lambda: _scans_fn(pkg, lib.lislam_bow_add_batch_scans, few)(b.h, [2]), nat.ERR_ARG,
         "lislam_bow_add_batch_scans: scans[0] = 2 outside [0, 2)"),
        (lambda: _scans_fn(pkg, lib.lislam_bow_add_batch_scans, few)(b.h, [0]), nat.ERR_ARG,
         "lislam_bow_add_batch_scans: the batch detects 1000 features, max_features is 999"),
        (lambda: lib.lislam_bow_add_batch(few.h, b.h, 0, 1), nat.ERR_ARG,
         "lislam_bow_add_batch: the batch detects 1000 features, max_features is 999"),
    ])
    assert lst_fn(b.h, []) == nat.OK and len(db) == 0
    for feed, order in ((lambda p: p.add_batch(b, 0, 2), (0, 1)), (lambda p: p.add_batch_scans(b, [1, 0]), (1, 0))):
        got, ref = make(c), make(c)
        feed(got)
        for s in order:
            ref.add_batch(b, s, 1)
        assert len(got) == len(ref) == 2
        assert [_bow_entry(got, i) for i in range(2)] == [_bow_entry(ref, i) for i in range(2)]
        assert _bow_entry(got, 0) != _bow_entry(got, 1)
        got.close()
        ref.close()
    db.add_batch(b, 0, 2)
    _table(c, [
        (lambda: rng_fn(b.h, 0, 1), nat.ERR_CAPACITY, "lislam_bow_add_batch: 2 + 1 entries exceed the capacity 2"),
        (lambda: lst_fn(b.h, [1]), nat.ERR_CAPACITY, "lislam_bow_add_batch_scans: 2 + 1 entries exceed the capacity 2"),
    ])
    assert len(db) == 2
    db.close()
    few.close()


def test_bag_of_words_staging_grows_between_calls(pkg, ctx16):
    """The second add is larger than the first: the staging is reallocated behind the first call."""
    voc = BC.vocabulary("k10L3")
    rng = np.random.default_rng(5)
    small, big = rng.integers(0, 256, (10, 32), dtype=np.uint8), rng.integers(0, 256, (500, 32), dtype=np.uint8)
    two, a, b = (pkg.BowDatabase(ctx16, *voc, capacity=2) for _ in range(3))
    two.add([small])
    two.add([big])
    a.add([small])
    b.add([big])
    assert _bow_entry(two, 0) == _bow_entry(a, 0) and _bow_entry(two, 1) == _bow_entry(b, 0)
    assert _bow_entry(two, 0) != _bow_entry(two, 1)
    for o in (two, a, b):
        o.close()


def test_bow_trainer_feed(pkg, ctx16, batch, foreign, orb):
    nat, lib = pkg.native, ctx16.lib
    who = "lislam_bow_trainer_add_batch"
    tr = pkg.BowTrainer(ctx16, 2, 4000)
    fn = lambda bh, first, n: lib.lislam_bow_trainer_add_batch(tr.h, bh, first, n)  # noqa: E731
    _table(ctx16, _range_rows(nat, who, fn, batch, foreign) + [
        (lambda: fn(batch.h, 0, 1), nat.ERR_STATE, f"{who}: run lislam_batch_intensity_odometry over 1 scans first"),
        (lambda: fn(batch.h, 1, 0), nat.ERR_STATE, f"{who}: run lislam_batch_intensity_odometry over 1 scans first"),
        # two at once: no descriptors yet and more images than fit
        (lambda: fn(batch.h, 0, 3), nat.ERR_STATE, f"{who}: run lislam_batch_intensity_odometry over 3 scans first"),
    ])
    assert tr.size() == (0, 0)
    tr.close()
    c, b = orb
    tr, one, ref = pkg.BowTrainer(c, 2, 4000), pkg.BowTrainer(c, 1, 4000), pkg.BowTrainer(c, 2, 4000)
    _table(c, [
        (lambda: lib.lislam_bow_trainer_add_batch(tr.h, b.h, 1, 2), nat.ERR_ARG, f"{who}: scans [1, 1 + 2) out of range"),
        (lambda: lib.lislam_bow_trainer_add_batch(one.h, b.h, 0, 2), nat.ERR_CAPACITY, f"{who}: 0 + 2 images exceed the capacity 1"),
    ])
    tr.add_batch(b, 0, 2)
    ref.add_batch(b, 0, 1)
    ref.add_batch(b, 1, 1)
    assert tr.size() == ref.size() and tr.size()[0] == 2 and tr.size()[1] > 0
    _table(c, [(lambda: lib.lislam_bow_trainer_add_batch(tr.h, b.h, 0, 1), nat.ERR_CAPACITY,
                f"{who}: 2 + 1 images exceed the capacity 2")])
    for o in (tr, one, ref):
        o.close()


# ---------------------------------------------------------------- keyframe selection
def test_keysel_step_batch_errors(pkg, ctx16, batch, foreign):
    nat, lib = pkg.native, ctx16.lib
    who = "lislam_keysel_step_batch"
    sel = pkg.KeyframeSelector(ctx16)
    t, ids, n = np.array([1.0, 2.0, 3.0, 4.0]), np.zeros(4, np.int32), ctypes.c_int32(7)
    fn = lambda bh, first, k, time=t: lib.lislam_keysel_step_batch(  # noqa: E731
        sel.h, bh, first, k, None if time is None else nat.ptr(time), nat.ptr(ids), ctypes.byref(n), None, None)
    _table(ctx16, _range_rows(nat, who, fn, batch, foreign) + [
        (lambda: fn(batch.h, 0, 1, None), nat.ERR_ARG, f"{who}: null time"),
        (lambda: fn(batch.h, 0, 1), nat.ERR_STATE, f"{who}: run lislam_batch_intensity_odometry over 1 scans first"),
        (lambda: fn(batch.h, 1, 0, None), nat.ERR_STATE, f"{who}: run lislam_batch_intensity_odometry over 1 scans first"),
        # two at once: the range before the null time, the null time before the missing descriptors
        (lambda: fn(batch.h, 4, 1, None), nat.ERR_ARG, f"{who}: scans [4, 4 + 1) out of range"),
        (lambda: fn(batch.h, 0, 2, None), nat.ERR_ARG, f"{who}: null time"),
    ])
    assert sel.state()[0] == 0 and n.value == 7
    sel.close()


# ---------------------------------------------------------------- pose graph
def _graph_bytes(g):
    i, j, z, var, robust = g.edges()
    return g.size(), g.poses().tobytes(), i.tobytes(), j.tobytes(), z.tobytes(), var.tobytes(), robust.tobytes()


def test_pose_graph_feeds(pkg, ctx16, batch, fresh, foreign):
    nat, lib = pkg.native, ctx16.lib
    make = lambda: pkg.PoseGraph(ctx16, node_capacity=2, edge_capacity=2)  # noqa: E731
    g = make()
    rng_fn = lambda bh, first, n, var=None: lib.lislam_pgo_add_batch(  # noqa: E731
        g.h, bh, first, n, None if var is None else nat.ptr(var))
    who = "lislam_pgo_add_batch"
    _table(ctx16, _range_rows(nat, who, rng_fn, batch, foreign) + [
        (lambda: rng_fn(batch.h, 0, 1, BAD_VAR), nat.ERR_ARG, f"{who}: variances must be positive"),
        (lambda: rng_fn(batch.h, 1, 2), nat.ERR_STATE, f"{who}: extract and run the odometry of 3 scans first"),
        (lambda: rng_fn(fresh.h, 0, 1), nat.ERR_STATE, f"{who}: extract and run the odometry of 1 scans first"),
        # two at once: the range before the variances, the variances before the extraction, that before the capacity
        (lambda: rng_fn(batch.h, 4, 1, BAD_VAR), nat.ERR_ARG, f"{who}: scans [4, 4 + 1) out of range"),
        (lambda: rng_fn(batch.h, 1, 2, BAD_VAR), nat.ERR_ARG, f"{who}: variances must be positive"),
        (lambda: rng_fn(batch.h, 0, 3), nat.ERR_STATE, f"{who}: extract and run the odometry of 3 scans first"),
    ])

    def lst_fn(bh, scans, var=None):
        p, keep = _list(pkg, scans)
        return lib.lislam_pgo_add_batch_scans(g.h, bh, p, len(keep), None if var is None else nat.ptr(var))

    who = "lislam_pgo_add_batch_scans"
    _table(ctx16, [
        (lambda: lst_fn(foreign.h, [0]), nat.ERR_ARG, f"{who}: the batch belongs to another context"),
        (lambda: lst_fn(batch.h, [0], BAD_VAR), nat.ERR_ARG, f"{who}: variances must be positive"),
        (lambda: lst_fn(fresh.h, [0]), nat.ERR_STATE, f"{who}: extract the batch and run its odometry first"),
        (lambda: lst_fn(batch.h, [0, 2]), nat.ERR_ARG, f"{who}: scans[1] = 2 outside [0, 2)"),
        (lambda: lst_fn(batch.h, [-1]), nat.ERR_ARG, f"{who}: scans[0] = -1 outside [0, 2)"),
        (lambda: lst_fn(batch.h, [1, 1]), nat.ERR_ARG, f"{who}: scans[1] = 1 after 1: the list must be strictly increasing"),
        (lambda: lst_fn(batch.h, [1, 0]), nat.ERR_ARG, f"{who}: scans[1] = 0 after 1: the list must be strictly increasing"),
        # two at once: the variances before the extraction, the extraction before the list, the list before the capacity
        (lambda: lst_fn(fresh.h, [0], BAD_VAR), nat.ERR_ARG, f"{who}: variances must be positive"),
        (lambda: lst_fn(fresh.h, [7]), nat.ERR_STATE, f"{who}: extract the batch and run its odometry first"),
        (lambda: lst_fn(batch.h, [0, 1, 2]), nat.ERR_ARG, f"{who}: scans[2] = 2 outside [0, 2)"),
    ])
    assert lst_fn(batch.h, []) == nat.OK and lst_fn(fresh.h, []) == nat.OK and g.size() == (0, 0)
    # the valid feeds against single-scan range calls
    g.add_batch(batch, 0, 2)
    lst, ref = make(), make()
    lst.add_batch_scans(batch, [0, 1])
    ref.add_batch(batch, 0, 1)
    ref.add_batch(batch, 1, 1)
    assert g.size() == (2, 1)
    assert _graph_bytes(g) == _graph_bytes(ref) == _graph_bytes(lst)
    pose = np.array([batch.download(nat.OUT_POSE, k) for k in range(2)]).reshape(2, 7)
    assert g.poses().tobytes() == pose.tobytes() and pose[0].tobytes() != pose[1].tobytes()
    # full
    _table(ctx16, [
        (lambda: rng_fn(batch.h, 0, 1), nat.ERR_CAPACITY,
         "lislam_pgo_add_batch: 2 + 1 nodes / 1 + 0 edges exceed the capacity 2 / 2"),
        (lambda: rng_fn(batch.h, 1, 1), nat.ERR_CAPACITY,
         "lislam_pgo_add_batch: 2 + 1 nodes / 1 + 1 edges exceed the capacity 2 / 2"),
        (lambda: lst_fn(batch.h, [1]), nat.ERR_CAPACITY,
         "lislam_pgo_add_batch_scans: 2 + 1 nodes / 1 + 1 edges exceed the capacity 2 / 2"),
    ])
    assert g.size() == (2, 1)
    for o in (g, lst, ref):
        o.close()
