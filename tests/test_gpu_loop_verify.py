"""GPU tests of the device keyframe pool (lislam_keyframes_*) and of the batched loop verification
(lislam_loop_verify): every candidate of a call equals the single path (lislam_loop_icp) and the
CPU oracle on its submap, bit for bit -- the batch performs the same floating-point operations per
candidate, so every comparison is equality.  The cases and what they cover: loop_verify_cases.py,
test_loop_verify_cases_cpu.py."""
import ctypes

import numpy as np
import pytest

import loop_verify_cases as C

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(pkg, synth, ctx):
    p = pkg.KeyframePool(ctx, capacity=C.POOL_SIZE, point_capacity=1 << 17)
    p.add_clouds(C.pool_clouds(synth))
    yield p
    p.close()


def _same_row(got, k, ref):
    Ti, Tc2m, fit, info = got
    rTi, rTc2m, rfit, rinfo = ref
    assert list(info[k]) == list(rinfo), k
    assert np.array_equal(Ti[k], rTi), k
    assert np.array_equal(Tc2m[k], rTc2m), k
    assert fit[k] == rfit, k


def test_pool_round_trip(pkg, synth, ctx):
    import torch

    clouds = C.pool_clouds(synth)
    total = sum(c.shape[0] for c in clouds)
    p = pkg.KeyframePool(ctx, capacity=2 * C.POOL_SIZE + 3, point_capacity=2 * total + 3 * 65536)
    p.add_clouds(clouds)                                   # host arrays
    counts = [c.shape[0] for c in clouds]
    dev = torch.from_numpy(np.concatenate(clouds)).cuda()  # one device tensor
    p.add_clouds(dev, counts)
    assert p.size() == (2 * C.POOL_SIZE, 2 * total)
    for i, c in enumerate(clouds):
        for j in (i, C.POOL_SIZE + i):
            got = p.cloud(j)
            assert got.shape == c.shape and got.tobytes() == c.tobytes(), j
    # cloud_track of an extracted 64 x 1024 batch, device to device
    b = pkg.Batch(ctx, 3)
    b.upload(synth.make_sequence(3, 64, 1024))
    b.extract(3)
    p.add_batch(b, 0, 2)
    p.add_batch(b, 2, 1)  # a range that starts inside the batch
    assert p.size() == (2 * C.POOL_SIZE + 3, 2 * total + 3 * 65536)
    for k in range(3):
        track = b.download(pkg.native.OUT_CLOUD_TRACK, k)
        assert p.cloud(2 * C.POOL_SIZE + k).tobytes() == np.ascontiguousarray(track, np.float32).tobytes()
    b.close()
    p.close()


def test_pool_errors(pkg, synth, ctx):
    n, lib = pkg.native, ctx.lib
    err = lambda: (lib.lislam_last_error(ctx.h) or b"").decode()
    clouds = C.pool_clouds(synth)
    p = pkg.KeyframePool(ctx, capacity=3, point_capacity=4096 + 65536)
    p.add_clouds(clouds[:1])
    b = pkg.Batch(ctx, 2)
    b.upload(synth.make_sequence(2, 64, 1024))
    b.extract(2)
    two = np.zeros((80000, 4), np.float32)
    cnt2 = np.array([40000, 40000], np.int32)
    # over the point capacity, then over the keyframe capacity: nothing is added
    assert lib.lislam_keyframes_add_clouds(p.h, n.ptr(two), n.ptr(cnt2), 2) == n.ERR_CAPACITY and "points" in err()
    assert lib.lislam_keyframes_add_batch(p.h, b.h, 0, 2) == n.ERR_CAPACITY and "points" in err()
    zeros = np.zeros(3, np.int32)
    assert lib.lislam_keyframes_add_clouds(p.h, None, n.ptr(zeros), 3) == n.ERR_CAPACITY and "keyframes" in err()
    assert p.size() == (1, 4096)
    # preconditions of add_batch, as lislam_place_add_batch
    assert lib.lislam_keyframes_add_batch(p.h, b.h, 1, 2) == n.ERR_ARG and "range" in err()
    assert lib.lislam_keyframes_add_batch(p.h, b.h, -1, 1) == n.ERR_ARG
    bad = np.array([5, -1], np.int32)
    assert lib.lislam_keyframes_add_clouds(p.h, n.ptr(two), n.ptr(bad), 2) == n.ERR_ARG
    other = pkg.Context(n_scans=16, width=256)
    ob = pkg.Batch(other, 1)
    ob.upload(synth.make_sequence(1, 16, 256))
    ob.extract(1)
    assert lib.lislam_keyframes_add_batch(p.h, ob.h, 0, 1) == n.ERR_ARG and "another context" in err()
    ob.close()
    other.close()
    fresh = pkg.Batch(ctx, 2)
    assert lib.lislam_keyframes_add_batch(p.h, fresh.h, 0, 1) == n.ERR_STATE
    fresh.close()
    bare = pkg.Context(n_scans=16, width=256, want_images=False)
    bp, bb = pkg.KeyframePool(bare, capacity=1, point_capacity=4096), pkg.Batch(bare, 1)
    assert lib.lislam_keyframes_add_batch(bp.h, bb.h, 0, 1) == n.ERR_STATE
    for o in (bp, bb, bare):
        o.close()
    # download: index and capacity
    out = np.zeros((4096, 4), np.float32)
    cnt = ctypes.c_int32()
    assert lib.lislam_keyframes_download(p.h, 1, n.ptr(out), 4096, ctypes.byref(cnt)) == n.ERR_ARG and "range" in err()
    assert lib.lislam_keyframes_download(p.h, 0, n.ptr(out), 100, ctypes.byref(cnt)) == n.ERR_CAPACITY and cnt.value == 4096
    h = ctypes.c_void_p()
    assert lib.lislam_keyframes_create(ctx.h, 0, 10, ctypes.byref(h)) == n.ERR_ARG
    assert lib.lislam_keyframes_create(ctx.h, 1, -1, ctypes.byref(h)) == n.ERR_ARG
    # it still takes what fits: a batch scan fills it to the last point, then an empty keyframe
    p.add_batch(b, 1, 1)
    p.add_clouds([np.zeros((0, 4), np.float32)])
    assert p.size() == (3, 4096 + 65536) and p.cloud(2).shape == (0, 4)
    assert p.cloud(0).tobytes() == clouds[0].tobytes()
    b.close()
    p.close()


@pytest.mark.parametrize("name", [c[0] for c in C.CONFIGS] + ["mixed_overflow"])
def test_verify_equals_the_single_path(pkg, oracle, synth, ctx, pool, name):
    """Every case list in ONE verify_loops call: each row equals oracle.loop_icp and the GPU's
    lislam_loop_icp on the candidate's submap; loop_id < 0 rows come back as -3."""
    _, kw, w, cands = next(c for c in C.all_configs(synth) if c[0] == name)
    clouds, T = C.pool_clouds(synth), C.keyframe_poses(synth)
    ref = C.cached_oracle_rows(oracle, synth, name)
    cfg = pkg.loop.IcpConfig(**kw)
    got = pool.verify_loops([c[0] for c in cands], [c[1] for c in cands], T, cfg, submap_window=w)
    for k, (cur, loop) in enumerate(cands):
        if loop < 0:
            assert list(got[3][k]) == [-3, 0, 0, 0, 0, 0, 0, 0]
            assert np.array_equal(got[0][k], np.eye(4)) and np.array_equal(got[1][k], T[cur]) and got[2][k] == DBL_MAX
            continue
        _same_row(got, k, ref[k])
        ids = C.submap_ids(cur, loop, w)
        single = pkg.loop.loop_closure_icp(ctx, clouds[cur], T[cur], [clouds[i] for i in ids], [T[i] for i in ids], cfg)
        _same_row(got, k, single)


def test_batching_does_not_matter(pkg, synth, ctx, pool):
    """Any order of the candidates, and one call per candidate, give the same rows; T_kf may lie on
    the device; n_loops = 0 touches nothing."""
    import torch

    T = C.keyframe_poses(synth)
    cands = C.DEFAULT_CANDIDATES
    cur, loop = np.array([c[0] for c in cands]), np.array([c[1] for c in cands])
    base = pool.verify_loops(cur, loop, T)
    assert [int(v) for v in base[3][:, 0]] == [1, 1, 1, 1]
    for perm in ([3, 2, 1, 0], [2, 0, 3, 1], [1, 3, 0, 2]):
        got = pool.verify_loops(cur[perm], loop[perm], T)
        assert all(np.array_equal(b[perm], g) for b, g in zip(base, got)), perm
    for k in range(4):
        one = pool.verify_loops(cur[k:k + 1], loop[k:k + 1], T)
        assert all(np.array_equal(o[0], b[k]) for o, b in zip(one, base)), k
    dT = torch.from_numpy(T).cuda()
    torch.cuda.synchronize()
    assert all(np.array_equal(g, o) for g, o in zip(pool.verify_loops(cur, loop, dT), base))
    out = [np.full(16, 7.0), np.full(16, 7.0), np.full(1, 7.0), np.full(8, 7, np.int32)]
    n, cfg = pkg.native, pkg.loop.IcpConfig()
    T16 = np.ascontiguousarray(T.reshape(-1, 16))
    assert ctx.lib.lislam_loop_verify(pool.h, ctypes.byref(cfg), 1, None, None, 0, n.ptr(T16), *(n.ptr(o) for o in out)) == n.OK
    assert all((o == 7).all() for o in out)
    empty = pool.verify_loops([], [], T)
    assert empty[0].shape == (0, 4, 4) and empty[3].shape == (0, 8)


def test_argument_errors(pkg, synth, ctx, pool):
    n, lib = pkg.native, ctx.lib
    err = lambda: (lib.lislam_last_error(ctx.h) or b"").decode()
    T16 = np.ascontiguousarray(C.keyframe_poses(synth).reshape(-1, 16))
    cfg = pkg.loop.IcpConfig()
    for cur, loop, w, word in (([11, C.POOL_SIZE], [0, 3], 1, "cur_id"), ([11, -1], [0, -1], 1, "cur_id"),
                               ([11, 5], [0, 6], 1, "loop_id"), ([11, 16], [0, C.POOL_SIZE], 1, "loop_id"),
                               ([11, 10], [0, 3], 5, "submap_window"), ([11, 10], [0, 3], -1, "submap_window")):
        out = [np.full(32, 7.0), np.full(32, 7.0), np.full(2, 7.0), np.full(16, 7, np.int32)]
        c, l = np.array(cur, np.int32), np.array(loop, np.int32)
        rc = lib.lislam_loop_verify(pool.h, ctypes.byref(cfg), w, n.ptr(c), n.ptr(l), 2, n.ptr(T16), *(n.ptr(o) for o in out))
        assert rc == n.ERR_ARG and word in err(), (cur, loop, w, err())
        assert all((o == 7).all() for o in out)
    bad = pkg.loop.IcpConfig(voxel_size=0.0)
    c, l = np.array([11], np.int32), np.array([0], np.int32)
    assert lib.lislam_loop_verify(pool.h, ctypes.byref(bad), 1, n.ptr(c), n.ptr(l), 1, n.ptr(T16), None, None, None, None) == n.ERR_ARG
    with pytest.raises(n.LislamError):
        pool.verify_loops([11], [12], T16)
    # the pool still verifies
    assert pool.verify_loops([11], [0], T16)[3][0, 0] == 1


def test_close_loops(pkg, synth, ctx):
    """close_loops adds the edges that add_loop adds from the single-path results: the accepted
    candidates only, in candidate order."""
    from loop_cases import pose_T

    clouds = C.pool_clouds(synth)[:C.N_CORRIDOR]
    poses = np.stack([pkg.posegraph.matrix_to_pose(pose_T(synth.ground_truth_pose(k))) for k in range(C.N_CORRIDOR)])
    p = pkg.KeyframePool(ctx, capacity=C.N_CORRIDOR, point_capacity=C.N_CORRIDOR * 4096)
    p.add_clouds(clouds)
    cands = [(11, 0), (8, -1), (10, 3), (9, 5), (11, 7)]
    ga, gb = pkg.PoseGraph(ctx, 16, 16), pkg.PoseGraph(ctx, 16, 16)
    ga.add_nodes(poses)
    gb.add_nodes(poses)
    T = np.stack([pkg.loop.get_transform_matrix(*(float(v) for v in q)) for q in gb.key_poses_6d()])
    single = [pkg.loop.loop_closure_icp(ctx, clouds[cur], T[cur], [clouds[i] for i in C.submap_ids(cur, loop)],
                                        [T[i] for i in C.submap_ids(cur, loop)]) for cur, loop in cands if loop >= 0]
    fits = sorted(s[2] for s in single)
    assert fits[0] < fits[-1]
    cfg = pkg.loop.IcpConfig(fitness_threshold=0.5 * (fits[0] + fits[-1]))  # some are accepted, some are not
    it = iter(single)
    expect = []
    for cur, loop in cands:
        if loop < 0:
            continue
        Ti, Tc2m, fit, info = next(it)
        if info[1] and fit <= cfg.fitness_threshold:
            gb.add_loop(cur, loop, Tc2m, T[loop], fit, True)
            expect.append((cur, loop))
    assert 0 < len(expect) < len(single)
    out = pkg.close_loops(p, ga, [c[0] for c in cands], [c[1] for c in cands], cfg, robust=True)
    assert [tuple(c) for c, i in zip(cands, out[3]) if i[0] == 1] == expect and out[3][1, 0] == -3
    ea, eb = ga.edges(), gb.edges()
    assert ga.size() == gb.size() == (C.N_CORRIDOR, len(expect))
    assert list(zip(ea[0], ea[1])) == expect
    for a, b in zip(ea, eb):
        assert np.array_equal(a, b)
    assert (ea[4] == 1).all()
    for o in (ga, gb, p):
        o.close()
