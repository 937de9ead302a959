"""GPU check of backend.LoopBackend: one 16-scan 64x1024 batch stepped as [0, 8) then [8, 16) must give,
bit for bit, what the same sequence written out by hand from the public calls gives (step_batch, the
four add_batch_scans, detect, close_loops, optimize): both sides run the same kernels in the same order.

The detector is a bag-of-words database over a small vocabulary with a permissive configuration, so
that the restatement of detectLoop (tests/restate_bow.py) on the downloaded descriptors of the selected
scans reports loop candidates; that is asserted first, a run without a candidate would test nothing."""
import numpy as np
import pytest

import bow_cases as BC
import restate_bow as RB
import restate_keysel as RK

pytestmark = pytest.mark.gpu

N = 16
STEPS = ((0, 8), (8, 8))
TIMES = 20.0 + 0.1037 * np.arange(N)
INTERVALS = (0.15, 0.0)  # the time gate passes every second frame at the earliest; any motion passes the other
VOC = "k10L3"
BOW = dict(min_loop_search_gap=1, min_loop_bow_threshold=0.0, index_score_threshold=0.0, min_frame_index=0,
           loop_index_bound=1 << 20)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(pkg, synth, ctx):
    b = pkg.Batch(ctx, N)
    b.upload(synth.make_sequence(N, 64, 1024))
    b.extract(N)
    b.odometry(N, N - 1)
    b.intensity_odometry(N, 1000)
    yield b
    b.close()


def _objects(pkg, ctx):
    return (pkg.KeyframeSelector(ctx, *INTERVALS), pkg.KeyframePool(ctx, N, N * 64 * 1024),
            pkg.BowDatabase(ctx, *BC.vocabulary(VOC), capacity=N, max_features=1000, **BOW),
            pkg.PoseGraph(ctx, node_capacity=N, edge_capacity=4 * N))


def _icp(pkg):
    return pkg.loop.IcpConfig(max_iterations=10)


def _by_hand(pkg, ctx, b):
    """loopClosureThread / factorGraphThread for the two ranges, from the public calls."""
    sel, pool, db, g = _objects(pkg, ctx)
    out = []
    for first, n in STEPS:
        k0 = len(pool)
        ids, T, nodes = sel.step_batch(b, first, n, TIMES[first:first + n])
        scans = (first + np.flatnonzero(ids >= 0)).astype(np.int32)
        pool.add_batch_scans(b, scans)
        db.add_batch_scans(b, scans)
        g.add_batch_scans(b, scans)
        if k0 == 0:
            g.set_prior(0, g.poses(0, 1)[0])
        det = db.detect(k0, scans.shape[0])
        cur = np.arange(k0, k0 + scans.shape[0], dtype=np.int32)
        verified = pkg.close_loops(pool, g, cur, det.loop_id, _icp(pkg), False)
        summary = g.optimize() if np.any(verified[3][:, 0] == pkg.loop.ACCEPTED) else None
        out.append((ids, T, nodes, scans, det, verified, summary))
    return out, (sel, pool, db, g)


def _bytes(x):
    return np.ascontiguousarray(x).tobytes()


def test_backend_equals_the_sequence_by_hand(pkg, ctx, batch):
    nat, b = pkg.native, batch
    # the selection, restated on the downloaded rows, and the candidates, restated on the selected scans' descriptors
    T = np.array([b.download(nat.OUT_ORB_T, k) for k in range(N)]).reshape(N, 7)
    good = np.array([b.download(nat.OUT_ORB_STATS, k)[0] == 1 for k in range(N)], np.int32)
    r = RK.Selector(*INTERVALS)
    ref_ids, _, ref_nodes = r.step(T, good, TIMES)
    n_key = ref_nodes.shape[0]
    selected = np.flatnonzero(ref_ids >= 0)
    print("good", list(good), "selected", list(selected), "margins", r.margins())
    assert n_key >= 4 and min(r.margins()) > 1e-9
    assert (selected < 8).any() and (selected >= 8).any()
    desc = [b.download(nat.OUT_ORB_DESCRIPTORS, int(s)) for s in selected]
    loops, _, _, _ = RB.run_stateful(BC.restated(VOC), desc, dict(RB.DEFAULTS, **BOW))
    print("restated loop ids", loops)
    assert any(v >= 0 for v in loops)

    hand, hand_objs = _by_hand(pkg, ctx, b)
    sel, pool, db, g = _objects(pkg, ctx)
    be = pkg.LoopBackend(ctx, sel, pool, db, g, icp_cfg=_icp(pkg), robust=False)
    got = [be.step(b, first, n, TIMES[first:first + n]) for first, n in STEPS]

    assert np.array_equal(np.concatenate([s.keyframe_id for s in got]), ref_ids)
    assert [int(v) for s in got for v in s.detection.loop_id] == loops
    for s, (ids, T_s2m, nodes, scans, det, verified, summary) in zip(got, hand):
        assert _bytes(s.keyframe_id) == _bytes(ids) and _bytes(s.T_s2m) == _bytes(T_s2m) and _bytes(s.nodes) == _bytes(nodes)
        assert s.scans.dtype == np.int32 and _bytes(s.scans) == _bytes(scans)
        assert _bytes(s.detection.loop_id) == _bytes(det.loop_id)
        assert len(s.detection.ids) == len(det.ids)
        assert all(_bytes(a) == _bytes(c) for a, c in zip(s.detection.ids, det.ids))
        assert all(_bytes(a) == _bytes(c) for a, c in zip(s.detection.scores, det.scores))
        for a, c in zip((s.T_icp, s.T_cur2map, s.fitness, s.info), verified):
            assert a.shape == c.shape and _bytes(a) == _bytes(c)
        print("info[:, 0]", list(s.info[:, 0]), "fitness", list(s.fitness), "summary", summary)
        assert (s.summary is None) == (summary is None)
        assert (s.summary is not None) == bool(np.any(s.info[:, 0] == pkg.loop.ACCEPTED))
        if summary is not None:
            assert s.summary[:7] == summary[:7] and _bytes(s.summary.stats) == _bytes(summary.stats)
    hg = hand_objs[3]
    assert g.size() == hg.size() and g.size()[0] == n_key and g.size()[1] >= n_key - 1
    assert all(_bytes(a) == _bytes(c) for a, c in zip(g.edges(), hg.edges()))
    assert _bytes(g.poses()) == _bytes(hg.poses())
    frm, to = g.edges()[:2]
    assert sorted(frm[to == frm + 1]) == list(range(n_key - 1))  # the odometry chain runs keyframe to keyframe
    assert np.all(frm[to != frm + 1] > to[to != frm + 1])        # every other edge is a loop factor (cur, loop)
    assert len(pool) == len(db) == len(g) == n_key and sel.state()[0] == n_key
    for o in (sel, pool, db, g) + hand_objs:
        o.close()


def test_backend_step_without_a_keyframe(pkg, ctx, batch):
    """A range in which nothing is selected (the first scan alone is never good) adds nothing anywhere."""
    sel, pool, db, g = _objects(pkg, ctx)
    be = pkg.LoopBackend(ctx, sel, pool, db, g)
    s = be.step(batch, 0, 1, TIMES[:1])
    assert list(s.keyframe_id) == [-1] and s.scans.shape == (0,) and s.detection is None and s.summary is None
    assert s.info.shape == (0, 8) and len(pool) == len(db) == len(g) == 0
    for o in (sel, pool, db, g):
        o.close()
