"""GPU parity of the ORB bag-of-words loop detector (lislam_bow_*: k_bow_words, k_bow_vector,
k_bow_query, k_bow_select, k_bow_score) against the restatement of detectLoop and its DBoW3 calls
(tests/restate_bow.py).

Everything is compared by equality: word ids, the bytes of the BoW vectors' words and values,
result ids, scores as doubles, loop ids.  The kernels and the restatement run the same double
operations in the same order (lislam_bow.hip's header), so nothing needs a tolerance."""
import ctypes

import numpy as np
import pytest

import bow_cases as BC
import restate_bow as RB

pytestmark = pytest.mark.gpu

SCRIPT_KW = dict(min_loop_search_gap=5, min_loop_bow_threshold=0.013)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


def _db(pkg, ctx, name, capacity, max_features=1000, **cfg):
    return pkg.BowDatabase(ctx, *BC.vocabulary(name), capacity=capacity, max_features=max_features, **cfg)


def _vector_equals(db, i, v):
    words, values = db.bow_vector(i)
    rw, rv = RB.vector_arrays(v)
    assert words.tobytes() == rw.tobytes() and values.tobytes() == rv.tobytes(), i


def _dump(db):
    return b"".join(a.tobytes() for i in range(len(db)) for a in db.bow_vector(i))


@pytest.mark.parametrize("name", BC.VOCABULARIES)
def test_transform_and_vectors(pkg, ctx, name):
    """The descent and the BoW vector of every descriptor set: ties between siblings, all-zero and
    all-ones descriptors, node descriptors, counts 0 / 1 / 63 / 64 / 65 / 1000, a 1,000-fold repeat,
    only weight-0 words.  k17L2 and k64L1 take one wave per descriptor, the others a 16-lane row."""
    voc, sets = BC.restated(name), BC.descriptor_sets(name)
    biggest = max(s.shape[0] for s in sets.values())
    db = _db(pkg, ctx, name, capacity=len(sets), max_features=biggest)
    for s in sets.values():
        words, weights = db.transform(s)
        rw, rwt = voc.transform(s)
        assert np.array_equal(words, rw) and weights.tobytes() == rwt.tobytes()
    db.add(list(sets.values()))
    assert len(db) == len(sets)
    for i, (key, s) in enumerate(sets.items()):
        v = RB.bow_vector(voc, s)
        _vector_equals(db, i, v)
        if key in ("random0", "weight0"):
            assert db.bow_vector(i)[0].shape[0] == 0
        if key == "repeat1000" and v:
            assert list(db.bow_vector(i)[1]) == [1.0]
    db.close()


def test_add_from_a_device_pointer(pkg, ctx):
    import torch

    sets = BC.descriptor_sets("k10L3")
    images = [sets["random65"], sets["random0"], sets["random1000"], sets["mixed"]]
    host, dev = _db(pkg, ctx, "k10L3", 4), _db(pkg, ctx, "k10L3", 4)
    host.add(images)
    rows = torch.from_numpy(np.concatenate(images)).cuda()
    counts = np.array([im.shape[0] for im in images], np.int32)
    torch.cuda.synchronize()
    assert ctx.lib.lislam_bow_add(dev.h, ctypes.c_void_p(rows.data_ptr()), pkg.native.ptr(counts), 4) == 0
    assert len(dev) == 4 and _dump(dev) == _dump(host)
    host.close()
    dev.close()


def test_add_batch_reads_the_orb_descriptors_on_the_device(pkg, synth, ctx):
    """add_batch on 3 scans of 64x1024 at nfeatures 1,000 is byte-equal to add of the downloaded
    OUT_ORB_DESCRIPTORS; a range that starts inside the batch works; LISLAM_ERR_STATE before the ORB
    front end has run."""
    nat = pkg.native
    b = pkg.Batch(ctx, 3)
    b.upload(synth.make_sequence(3, 64, 1024))
    b.extract(3)
    dev, host = _db(pkg, ctx, "k10L3", 5), _db(pkg, ctx, "k10L3", 3)
    assert ctx.lib.lislam_bow_add_batch(dev.h, b.h, 0, 3) == nat.ERR_STATE and ctx.lib.lislam_last_error(ctx.h)
    assert len(dev) == 0
    b.intensity_odometry(3, 1000)
    dev.add_batch(b, 0, 3)
    dev.add_batch(b, 1, 2)
    desc = [b.download(nat.OUT_ORB_DESCRIPTORS, k) for k in range(3)]
    assert all(0 < d.shape[0] <= 1000 for d in desc)
    host.add(desc)
    assert len(dev) == 5 and len(host) == 3
    voc = BC.restated("k10L3")
    for k in range(3):
        _vector_equals(dev, k, RB.bow_vector(voc, desc[k]))
    assert _dump(dev) == _dump(host) + b"".join(a.tobytes() for i in (1, 2) for a in host.bow_vector(i))
    # a database for fewer features than the batch detects
    small = _db(pkg, ctx, "k10L3", 3, max_features=500)
    assert ctx.lib.lislam_bow_add_batch(small.h, b.h, 0, 1) == nat.ERR_ARG and len(small) == 0
    for o in (small, dev, host, b):
        o.close()


def _restated(cfg_kw):
    cfg = dict(RB.DEFAULTS, **cfg_kw)
    return RB.run_stateful(BC.restated("script"), BC.scripted_keyframes(), cfg)


def _detection_equals(got, loops, rets, first=0):
    assert list(got.loop_id) == loops[first:first + len(got.loop_id)]
    for k, (ids, scores) in enumerate(zip(got.ids, got.scores)):
        ref = rets[first + k]
        assert list(ids) == [r[0] for r in ref], first + k
        assert scores.tobytes() == np.array([r[1] for r in ref], np.float64).tobytes(), first + k


def _same_detection(a, b):
    return (np.array_equal(a.loop_id, b.loop_id) and all(x.tobytes() == y.tobytes() for x, y in zip(a.ids, b.ids))
            and all(x.tobytes() == y.tobytes() for x, y in zip(a.scores, b.scores)) and len(a.ids) == len(b.ids))


@pytest.fixture(scope="module")
def script_restated():
    return {"script": _restated(SCRIPT_KW), "default": _restated({})}


@pytest.mark.parametrize("name", ["script", "default"])
def test_detect_on_the_scripted_database(pkg, ctx, script_restated, name):
    """detect over [0, 70) in one call == piecewise calls == one detect_loop per keyframe == the
    stateful restatement, and it does not change when 10 more entries are added.  Under the defaults
    (gap 50) keyframes 48..51 meet max_id -2, -1, 0 and 1."""
    kw = SCRIPT_KW if name == "script" else {}
    frames = list(BC.scripted_keyframes())
    loops, rets, events, rdb = script_restated[name]
    db = _db(pkg, ctx, "script", capacity=80, max_features=500, **kw)
    db.add(frames)
    for k in (0, 4, 22, BC.SCRIPT_EMPTY, BC.SCRIPT_WEIGHT0, 60):
        _vector_equals(db, k, rdb.vectors[k])
    got = db.detect(0, 70)
    _detection_equals(got, loops, rets)
    for first, n in ((0, 1), (1, 21), (22, 1), (23, 40), (63, 7)):
        _detection_equals(db.detect(first, n), loops, rets, first)
    if name == "script":
        assert [k for k in range(70) if got.loop_id[k] >= 0] == [22, 25, 30, 35, 49, 60]
        assert list(got.ids[4]) == [0, 1] and got.loop_id[4] == -1  # the unrestricted query of i - gap == -1
    else:
        assert len(got.ids[48]) == 0 and len(got.ids[49]) > 0 and len(got.ids[50]) == 0 and got.loop_id[49] == -1
        assert got.loop_id[60] == 1
    db.add(frames[:10])
    assert _same_detection(db.detect(0, 70), got)
    _detection_equals(db.detect(70, 10), *_restated_more(kw), first=70)
    db.close()
    step = _db(pkg, ctx, "script", capacity=30, max_features=500, **kw)
    assert [step.detect_loop(f) for f in frames[:30]] == loops[:30]
    step.close()


def _restated_more(kw):
    cfg = dict(RB.DEFAULTS, **kw)
    frames = list(BC.scripted_keyframes())
    loops, rets, _, _ = RB.run_stateful(BC.restated("script"), frames + frames[:10], cfg)
    return loops, rets


@pytest.mark.parametrize("gap,max_results", [(3, 16), (50, 4)])
def test_detect_on_random_keyframes(pkg, ctx, gap, max_results):
    """200 keyframes that all share words: every entry below the limit is a result, max_results 16."""
    voc, frames = BC.restated("k10L3"), list(BC.random_keyframes())
    cfg = dict(RB.DEFAULTS, min_loop_search_gap=gap, max_results=max_results)
    loops, rets, _, _ = RB.run_stateful(voc, frames, cfg)
    db = _db(pkg, ctx, "k10L3", capacity=200, max_features=150, min_loop_search_gap=gap, max_results=max_results)
    db.add(frames)
    _detection_equals(db.detect(), loops, rets)
    db.close()


def test_score_of_pairs(pkg, ctx):
    voc, frames = BC.restated("k10L3"), list(BC.random_keyframes())[:40]
    vectors = [RB.bow_vector(voc, f) for f in frames]
    assert vectors[36] == {}
    db = _db(pkg, ctx, "k10L3", capacity=40, max_features=150)
    db.add(frames)
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.integers(0, 40, 100), [36, 36, 5, 7]]).astype(np.int32)
    b = np.concatenate([rng.integers(0, 40, 100), [36, 5, 36, 7]]).astype(np.int32)
    got = db.score(a, b)
    ref = np.array([RB.l1_score(vectors[i], vectors[j]) for i, j in zip(a, b)])
    assert got.tobytes() == ref.tobytes()
    distinct = a != b
    assert np.all(got[100:103] == 0) and np.all((got[distinct] >= 0) & (got[distinct] <= 1))
    # an entry against itself: the sum of its own n values, within n ulps of 1 (test_bow_cpu.test_scores)
    for i, s in zip(a[~distinct], got[~distinct]):
        assert abs(s - 1.0) <= len(vectors[i]) * 2.0 ** -52 if vectors[i] else s == 0
    db.close()


def test_tied_scores_come_lower_id_first(pkg, ctx):
    """Two identical entries score equal against any query: the lower id comes first (DBoW3 leaves the
    order to std::sort; unpinned)."""
    frames = list(BC.random_keyframes())
    twin, other, query = frames[0], frames[1], np.concatenate([frames[0][:60], frames[2]])
    db = _db(pkg, ctx, "k10L3", capacity=5, max_features=300, min_loop_search_gap=1, max_results=3)
    db.add([other, twin, twin, other, query])
    d = db.detect(4, 1)
    assert list(d.ids[0]) == [1, 2, 0] and d.scores[0][0] == d.scores[0][1] > d.scores[0][2]
    voc = BC.restated("k10L3")
    _, rets, _, _ = RB.run_stateful(voc, [other, twin, twin, other, query], dict(RB.DEFAULTS, min_loop_search_gap=1, max_results=3))
    assert list(d.ids[0]) == [r[0] for r in rets[4]] and list(d.scores[0]) == [r[1] for r in rets[4]]
    db.close()


def test_two_fresh_databases_agree_bytewise(pkg, ctx):
    frames = list(BC.scripted_keyframes())
    outs = []
    for _ in range(2):
        db = _db(pkg, ctx, "script", capacity=70, max_features=500, **SCRIPT_KW)
        db.add(frames)
        d = db.detect()
        pairs = np.arange(70, dtype=np.int32)
        outs.append(_dump(db) + d.loop_id.tobytes() + b"".join(x.tobytes() for x in d.ids + d.scores) +
                    db.score(pairs, pairs[::-1].copy()).tobytes() + db.transform(frames[3])[0].tobytes())
        db.close()
    assert outs[0] == outs[1]


def test_errors_add_nothing_and_set_the_message(pkg, synth, ctx):
    nat, lib = pkg.native, ctx.lib
    sets = BC.descriptor_sets("k10L3")

    def err():
        return lib.lislam_last_error(ctx.h).decode()

    # bad trees
    parent, desc, weight = (np.array(x) for x in BC.vocabulary("unbalanced"))
    h = ctypes.c_void_p()

    def create(p, d, w, cfg=None, capacity=4, max_features=100):
        p, d, w = np.ascontiguousarray(p, np.int32), np.ascontiguousarray(d, np.uint8), np.ascontiguousarray(w, np.float64)
        return lib.lislam_bow_create(ctx.h, p.shape[0], nat.ptr(p), nat.ptr(d), nat.ptr(w), None if cfg is None else
                                     ctypes.byref(cfg), capacity, max_features, ctypes.byref(h))

    def changed(arr, i, v):
        out = arr.copy()
        out[i] = v
        return out

    assert create(changed(parent, 0, 0), desc, weight) == nat.ERR_ARG and "parent[0]" in err()
    assert create(changed(parent, 5, 5), desc, weight) == nat.ERR_ARG and "parent[5]" in err()
    assert create(changed(parent, 5, 9), desc, weight) == nat.ERR_ARG and "parent[5]" in err()
    assert create(changed(parent, 5, -1), desc, weight) == nat.ERR_ARG
    assert create(parent[:1], desc[:1], weight[:1]) == nat.ERR_ARG and err()  # a root without children
    many = np.concatenate([[-1], np.zeros(65, np.int32)])
    assert create(many, np.zeros((66, 32), np.uint8), np.ones(66)) == nat.ERR_ARG and "children" in err()
    for bad in (-0.5, np.nan, np.inf):
        assert create(parent, desc, changed(weight, 12, bad)) == nat.ERR_ARG and "weight[12]" in err()
    for kw in (dict(max_results=0), dict(max_results=17), dict(min_loop_search_gap=-1)):
        assert create(parent, desc, weight, nat.BowConfig(**kw)) == nat.ERR_ARG and err(), kw
    assert create(parent, desc, weight, capacity=0) == nat.ERR_ARG
    assert create(parent, desc, weight, max_features=0) == nat.ERR_ARG
    assert create(parent, desc, weight, max_features=2049) == nat.ERR_ARG and "max_features" in err()
    assert create(many[:65], np.zeros((65, 32), np.uint8), np.ones(65)) == 0  # 64 children are fine
    assert lib.lislam_bow_destroy(h) == 0

    db = _db(pkg, ctx, "k10L3", capacity=3, max_features=65)
    db.add([sets["random65"], sets["random1"]])
    before = _dump(db)
    rows = np.ascontiguousarray(np.concatenate([sets["random64"], sets["random65"]]))
    two = np.array([64, 65], np.int32)
    assert lib.lislam_bow_add(db.h, nat.ptr(rows), nat.ptr(two), 2) == nat.ERR_CAPACITY and "capacity" in err()
    big = np.array([66], np.int32)
    assert lib.lislam_bow_add(db.h, nat.ptr(sets["random1000"]), nat.ptr(big), 1) == nat.ERR_ARG and "max_features" in err()
    assert lib.lislam_bow_add(db.h, nat.ptr(rows), nat.ptr(np.array([-1], np.int32)), 1) == nat.ERR_ARG and err()
    assert lib.lislam_bow_add(db.h, None, nat.ptr(np.array([3], np.int32)), 1) == nat.ERR_ARG and "null" in err()
    assert lib.lislam_bow_detect(db.h, 1, 2, None, None, None, None) == nat.ERR_ARG and "range" in err()
    assert lib.lislam_bow_detect(db.h, -1, 1, None, None, None, None) == nat.ERR_ARG
    ia, ib = np.array([0, 2], np.int32), np.array([1, 0], np.int32)
    assert lib.lislam_bow_score(db.h, nat.ptr(ia), nat.ptr(ib), 2, None) == nat.ERR_ARG and "range" in err()
    out, cnt = np.zeros(100), ctypes.c_int32()
    for what, idx in ((nat.BOW_WORDS, 2), (nat.BOW_VALUES, -1), (7, 0)):
        assert lib.lislam_bow_download(db.h, what, idx, nat.ptr(out), 100, ctypes.byref(cnt)) == nat.ERR_ARG and err()
    assert lib.lislam_bow_download(db.h, nat.BOW_VALUES, 0, nat.ptr(out), 3, ctypes.byref(cnt)) == nat.ERR_CAPACITY
    assert cnt.value == len(RB.bow_vector(BC.restated("k10L3"), sets["random65"]))
    # batches: another context's, and one whose ORB front end has not run (or not that far)
    other = pkg.Context(n_scans=16, width=256)
    ob = pkg.Batch(other, 1)
    assert lib.lislam_bow_add_batch(db.h, ob.h, 0, 1) == nat.ERR_ARG and "another context" in err()
    ob.close()
    other.close()
    fresh = pkg.Batch(ctx, 2)
    assert lib.lislam_bow_add_batch(db.h, fresh.h, 0, 1) == nat.ERR_STATE and "intensity_odometry" in err()
    assert lib.lislam_bow_add_batch(db.h, fresh.h, 1, 2) == nat.ERR_ARG and "range" in err()
    fresh.close()
    with pytest.raises(nat.LislamError):
        db.add([sets["random1"], sets["random1"]])
    assert len(db) == 2 and _dump(db) == before
    db.add([sets["random64"]])
    assert len(db) == 3
    _vector_equals(db, 2, RB.bow_vector(BC.restated("k10L3"), sets["random64"]))
    assert list(db.detect().loop_id) == [-1, -1, -1]
    db.close()
