"""CPU checks of the bag-of-words restatement (tests/restate_bow.py) and of the cases the GPU
tests rest on (tests/bow_cases.py): the literal stateful Database and the closed form agree, the
scripted database takes every branch of detectLoop, and no query has tied scores where the GPU
comparison needs a unique order."""
import numpy as np
import pytest

import bow_cases as BC
import restate_bow as RB

SETTINGS = [(5, 4), (50, 4), (3, 16)]  # (gap, max_results); every gap >= 2 meets k - gap = -2, -1 and 0


@pytest.fixture(scope="module")
def script():
    voc = BC.restated("script")
    frames = BC.scripted_keyframes()
    return voc, frames, RB.run_stateful(voc, frames, BC.SCRIPT_CFG)


@pytest.fixture(scope="module")
def random_db():
    voc = BC.restated("k10L3")
    frames = BC.random_keyframes()
    vectors = [RB.bow_vector(voc, f) for f in frames]
    return voc, frames, vectors


def _same(ret_a, ret_b):
    return [r[0] for r in ret_a] == [r[0] for r in ret_b] and [r[1] for r in ret_a] == [r[1] for r in ret_b]


@pytest.mark.parametrize("gap,max_results", SETTINGS)
def test_forms_agree_on_the_scripted_database(script, gap, max_results):
    voc, frames, (_, _, _, db0) = script
    cfg = dict(BC.SCRIPT_CFG, min_loop_search_gap=gap, max_results=max_results)
    loops, rets, events, db = RB.run_stateful(voc, frames, cfg)
    assert db.n == BC.N_SCRIPT
    for k in range(BC.N_SCRIPT):
        loop, ret, ev = RB.closed_form_detect(db.vectors, k, cfg)
        assert loop == loops[k] and ev == events[k] and _same(ret, rets[k]), k
    for d in (-2, -1, 0):
        assert RB.query_limit(gap + d, gap) == (gap - 1 if d == -1 else 0)


@pytest.mark.parametrize("gap,max_results", SETTINGS)
def test_forms_agree_on_random_keyframes(random_db, gap, max_results):
    voc, frames, vectors = random_db
    cfg = dict(RB.DEFAULTS, min_loop_search_gap=gap, max_results=max_results)
    db = RB.Database(voc)
    for k, v in enumerate(vectors):
        ret = db.query_vector(v, max_results, k - gap)
        db.add_vector(v)
        loop, ev = RB.decide(ret, k, cfg)
        loop2, ret2, ev2 = RB.closed_form_detect(vectors, k, cfg)
        assert loop == loop2 and ev == ev2 and _same(ret, ret2), k
        if k == gap - 1:
            assert len(ret) == min(max_results, sum(1 for x in vectors[:k] if x)) > 0  # max_id == -1: unrestricted
        if k in (gap - 2, gap):
            assert ret == []
        for e, s in ret:
            assert 0.0 <= s <= 1.0


def test_scripted_database_takes_every_branch(script):
    """Every branch of detectLoop under gap 5, th 0.013.  `i <= 5`: with a gap of 5 a keyframe with
    i <= 5 never holds a result when detectLoop reaches `find && i > 5` (i - gap <= 0 leaves the query
    nothing), so that branch shows as keyframes 0..5 returning -1, keyframe 4 (i - gap == -1, the
    unrestricted query) with two results above th among them."""
    voc, frames, (loops, rets, events, db) = script
    th = BC.SCRIPT_CFG["min_loop_bow_threshold"]
    seen = set().union(*events)
    assert {"empty", "ret0_low", "only_ret0", "i_small", "beyond_bound", "takeover", "refused", "loop", "before_gap"} <= seen
    assert loops[:6] == [-1] * 6 and all("i_small" in events[k] for k in range(6))
    assert [r[0] for r in rets[4]] == [0, 1] and all(r[1] > th for r in rets[4]) and loops[4] == -1
    assert rets[3] == [] and rets[5] == []  # max_id -2 and 0
    # an empty result after the gap, a result at or below th, only ret[0] above th
    assert "empty" in events[6] and "ret0_low" in events[8] and "only_ret0" in events[10] and "only_ret0" in events[40]
    assert "beyond_bound" in events[20] and loops[20] == -1 and "beyond_bound" in events[45]
    assert "takeover" in events[22] and loops[22] == 1
    assert "refused" in events[25] and loops[25] == 4
    refused = [r for r in rets[25] if r[0] == 2][0]
    assert th < refused[1] <= BC.SCRIPT_CFG["index_score_threshold"]
    assert loops[30] == 0 and loops[35] == 5 and loops[49] == 0 and loops[60] == 1
    assert sum(1 for x in loops if x >= 0) >= 3
    assert [k for k, x in enumerate(loops) if x >= 0] == [22, 25, 30, 35, 49, 60]
    # the keyframe without descriptors and the one on weight-0 words hold empty vectors and still took an id
    assert db.vectors[BC.SCRIPT_EMPTY] == {} and db.vectors[BC.SCRIPT_WEIGHT0] == {} and len(frames[BC.SCRIPT_WEIGHT0]) == 20
    assert rets[BC.SCRIPT_EMPTY] == [] and rets[BC.SCRIPT_WEIGHT0] == []


def test_scores(script, random_db):
    """score(a, a): the sum of the entry's own values.  It is exactly 1.0 where that sum is exact (one
    word; two or four words of one weight: powers of two); for any entry it is within n ulps of 1,
    each of its n quotients and n - 1 additions rounding once (|error| <= (2 n - 1) 2^-53 <= n 2^-52)."""
    voc = BC.restated("k10L3")
    sets = BC.descriptor_sets("k10L3")
    one = RB.bow_vector(voc, sets["repeat1000"])
    assert len(one) == 1 and list(one.values()) == [1.0] and RB.l1_score(one, one) == 1.0
    same_weight = RB.Vocabulary(voc.parent, voc.descriptor, np.where(voc.weight > 0, 1.5, 0.0))
    words = same_weight.transform(sets["random1000"])
    pick, seen = [], set()
    for d, wid, w in zip(sets["random1000"], words[0].tolist(), words[1].tolist()):
        if w > 0 and wid not in seen and len(pick) < 4:
            seen.add(wid)
            pick.append(d)
    for n in (2, 4):
        v = RB.bow_vector(same_weight, np.array(pick[:n]))
        assert len(v) == n and RB.l1_score(v, v) == 1.0
    _, _, vectors = random_db
    _, _, (_, _, _, db) = script
    for v in list(vectors) + db.vectors:
        if v:
            assert abs(RB.l1_score(v, v) - 1.0) <= len(v) * 2.0 ** -52
    rng = np.random.default_rng(5)
    for a, b in rng.integers(0, len(vectors), (300, 2)):
        s = RB.l1_score(vectors[a], vectors[b])
        assert 0.0 <= s <= 1.0
        if not vectors[a] or not vectors[b]:
            assert s == 0.0


def _no_ties(vectors, cfg):
    wide = dict(cfg, max_results=0)  # every result
    db = RB.Database(None)
    for k, v in enumerate(vectors):
        ret = db.query_vector(v, 0, k - wide["min_loop_search_gap"])
        db.add_vector(v)
        head = [s for _, s in ret[:cfg["max_results"] + 1]]
        assert len(set(head)) == len(head), (k, head)


@pytest.mark.parametrize("gap,max_results", SETTINGS + [(50, 4)])
def test_no_tied_scores_where_the_order_is_compared(script, random_db, gap, max_results):
    """No query of the GPU tests' sequences has two equal scores among its first max_results + 1
    (the dedicated tie case of test_gpu_bow.py aside), so the order of the results is unique."""
    _, _, (_, _, _, db) = script
    _, _, vectors = random_db
    cfg = dict(RB.DEFAULTS, min_loop_search_gap=gap, max_results=max_results)
    _no_ties(db.vectors, cfg)
    _no_ties(vectors, cfg)


def test_descent(random_db):
    """The level-by-level transform equals the literal descent, ties included; word ids follow the
    leaves in ascending node id."""
    for name in BC.VOCABULARIES:
        voc = BC.restated(name)
        sets = BC.descriptor_sets(name)
        sample = np.concatenate([sets["mixed"], sets["nodes"][:60], sets["zeros_ones"]])
        words, weights = voc.transform(sample)
        for d, wid, w in zip(sample, words, weights):
            assert voc.transform_one(d) == (wid, w)
        assert list(voc.word_of[voc.leaf_node]) == list(range(len(voc.leaf_node)))
        assert np.all(np.diff(voc.leaf_node) > 0)
    voc = BC.restated("unbalanced")
    assert voc.transform_one(voc.descriptor[8]) == (int(voc.word_of[7]), float(voc.weight[7]))  # identical siblings: the first
    assert len(BC.descriptor_sets("k10L3")["equidistant"]) == 8
    for name in BC.VOCABULARIES:
        s = BC.descriptor_sets(name)
        assert len(s["weight0"]) >= 10 and RB.bow_vector(BC.restated(name), s["weight0"]) == {}
        assert [len(s[f"random{c}"]) for c in BC.COUNTS] == list(BC.COUNTS)


def test_binding_matches_the_header(pkg):
    import ctypes

    n = pkg.native
    assert ctypes.sizeof(n.BowConfig) == 32
    c = n.BowConfig()
    assert {k: getattr(c, k) for k, _ in n.BowConfig._fields_} == RB.DEFAULTS  # detectLoop's constants
    assert pkg.BowDatabase is pkg.bow.BowDatabase
    data = open(n.LIB_PATH, "rb").read()
    for k in n.BOW_KERNELS:
        assert k.encode() in data, k


def test_null_arguments(pkg):
    import ctypes

    lib, E = pkg.native.load(), pkg.native.ERR_ARG
    h, n = ctypes.c_void_p(), ctypes.c_int32()
    assert lib.lislam_bow_create(None, 0, None, None, None, None, 1, 1, ctypes.byref(h)) == E
    assert lib.lislam_bow_destroy(None) == E
    assert lib.lislam_bow_size(None, ctypes.byref(n)) == E
    assert lib.lislam_bow_add(None, None, None, 0) == E
    assert lib.lislam_bow_add_batch(None, None, 0, 0) == E
    assert lib.lislam_bow_detect(None, 0, 0, None, None, None, None) == E
    assert lib.lislam_bow_score(None, None, None, 0, None) == E
    assert lib.lislam_bow_transform(None, None, 0, None, None) == E
    assert lib.lislam_bow_download(None, 0, 0, None, 0, ctypes.byref(n)) == E
