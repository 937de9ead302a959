"""GPU parity of the vocabulary training (lislam_bow_trainer_*, lislam_bow_train: k_bowt_seed,
k_bowt_assign, k_bowt_means, k_bowt_majority, the partition kernels, k_bowt_ni) against the literal
recursive restatement of DBoW3's Vocabulary::create (tests/restate_bow_train.py).

Everything is compared by equality of bytes: parent, descriptor, weight, and the iteration and node
counts of the statistics.  The training is integer arithmetic up to the host's log(N / Ni), which
the restatement takes with the same libm, so nothing needs a tolerance."""
import ctypes

import numpy as np
import pytest

import bow_train_cases as TC
import restate_bow as RB
import restate_bow_train as RT

pytestmark = pytest.mark.gpu

# the sizes the kernels change path at (lislam_bow.hip, namespace bowt)
K_THREADS = 256    # k_bowt_seed's narrow workgroup (four wave ranges), the flat kernels' workgroup
K_STAGE = 512      # the rows k_bowt_means stages in LDS at a time
K_TILE = 2048      # positions per tile of k_bowt_means and of the partition; wider nodes count globally
K_SEED_WIDE = 16384  # above it k_bowt_seed runs 1,024 threads
K_SLOT_PASS = 32   # slots k_bowt_means counts per pass


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


def _trainer(pkg, ctx, desc, counts, spare=0):
    tr = pkg.BowTrainer(ctx, len(counts) + spare + 1, desc.shape[0] + 1)
    tr.add(TC.images(desc, counts))
    assert tr.size() == (len(counts), desc.shape[0])
    return tr


def _equals(voc, stats, ref: RT.Trained):
    assert voc.parent.tobytes() == ref.parent.tobytes()
    assert voc.descriptor.tobytes() == ref.descriptor.tobytes()
    assert voc.weight.tobytes() == ref.weight.tobytes()
    leaves = np.setdiff1d(np.arange(ref.parent.shape[0]), ref.parent[1:])
    assert stats.n_nodes == ref.parent.shape[0]
    if stats.n_nodes > 1:
        assert stats.n_words == leaves.shape[0] and stats.n_zero_words == int(np.sum(ref.weight[leaves] == 0))
    m = len(stats.level_steps)
    for key in ("level_steps", "level_clustered", "level_iterations", "level_capped"):
        assert getattr(stats, key) == ref.stats[key][:m], key
        assert not any(ref.stats[key][m:]), key


def _check(pkg, ctx, desc, counts, k, L, max_iterations=100, seed=0, ref=None):
    tr = _trainer(pkg, ctx, desc, counts)
    voc = tr.train(k, L, max_iterations, seed)
    ref = ref or RT.train_recursive(desc, counts, k, L, max_iterations, seed)
    _equals(voc, tr.stats, ref)
    tr.close()
    return voc, ref


@pytest.mark.parametrize("k,L", TC.KL)
@pytest.mark.parametrize("name", ["random", "clustered"])
def test_five_thousand_rows(pkg, ctx, name, k, L):
    """5,000 rows in 40 images.  k = 17 and k = 64 take the one-wave-per-descriptor descent for the
    weights; (64, 1) is one node wider than a tile with two slot passes."""
    _, ref = _check(pkg, ctx, *TC.case(name), k, L, ref=TC.recursive(name, k, L))
    assert sum(ref.stats["level_capped"]) == 0


@pytest.mark.parametrize("name,k,L", [("duplicates", 3, 4), ("duplicates", 10, 3), ("duplicates", 64, 1), ("identical", 2, 1),
                                      ("identical", 3, 4), ("identical", 10, 3), ("gaps", 3, 4), ("gaps", 10, 3)])
def test_duplicates_identical_rows_and_empty_images(pkg, ctx, name, k, L):
    """7 distinct rows x 40 end the seeding at S == 0 with 7 centres; identical rows seed one centre
    per level; images without descriptors first, in between and last."""
    _, ref = _check(pkg, ctx, *TC.case(name), k, L, ref=TC.recursive(name, k, L))
    if name == "duplicates" and k >= 10:
        assert ref.events["s_zero"] >= 1


@pytest.mark.parametrize("n", [0, 1, 2, 9, 10, 11])
def test_descriptor_counts_around_k(pkg, ctx, n):
    """k = 10: no descriptor (the root alone, which lislam_bow_create rejects), one, k - 1, k (each
    its own child), k + 1 (the smallest k-means; its children hold <= k and split again at L = 2)."""
    rng = np.random.default_rng(40 + n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    tr = _trainer(pkg, ctx, desc, [n, 0] if n < 2 else [n - 2, 2])
    voc = tr.train(10, 2)
    _equals(voc, tr.stats, RT.train_recursive(desc, [n, 0] if n < 2 else [n - 2, 2], 10, 2))
    if n == 0:
        assert voc.parent.tolist() == [-1] and tr.stats.level_steps == []
        with pytest.raises(pkg.native.LislamError):
            tr.database(4)
    elif n <= 10:
        assert voc.parent.tolist() == [-1] + [0] * n and voc.descriptor[1:].tobytes() == desc.tobytes()
    tr.close()


@pytest.mark.parametrize("n", [K_THREADS - 1, K_THREADS, K_THREADS + 1, K_STAGE - 1, K_STAGE, K_STAGE + 1, K_TILE - 1, K_TILE,
                               K_TILE + 1])
def test_one_node_around_the_workgroup_and_tile_sizes(pkg, ctx, n):
    """The root's segment one below, at and one above 256, 512 and 2,048; L = 2 partitions it across
    the tiles and clusters the three children again."""
    rng = np.random.default_rng(n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    _check(pkg, ctx, desc, [n], 3, 2)


@pytest.mark.parametrize("n", [K_SEED_WIDE - 1, K_SEED_WIDE, K_SEED_WIDE + 1])
def test_one_node_around_the_wide_seeding(pkg, ctx, n):
    rng = np.random.default_rng(n)
    proto = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    desc = TC.flip(proto[rng.integers(0, 12, n)], 0.05, rng)
    _check(pkg, ctx, desc, [n - 100, 0, 100], 4, 1)


@pytest.mark.parametrize("k,n", [(K_SLOT_PASS, 400), (K_SLOT_PASS + 1, 400), (40, K_TILE + 500)])
def test_slot_passes(pkg, ctx, k, n):
    """32 slots are one pass of k_bowt_means, 33 are two, inside one tile and across tiles."""
    rng = np.random.default_rng(k + n)
    proto = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    desc = TC.flip(proto[rng.integers(0, 60, n)], 0.04, rng)
    _check(pkg, ctx, desc, TC.split(n, 7, rng), k, 2)


def test_an_empty_image_changes_every_weight(pkg, ctx):
    desc, counts = TC.case("gaps")
    a, ra = _check(pkg, ctx, desc, counts, 3, 4, ref=TC.recursive("gaps", 3, 4))
    b, _ = _check(pkg, ctx, desc, counts + [0], 3, 4)
    assert a.parent.tobytes() == b.parent.tobytes() and a.descriptor.tobytes() == b.descriptor.tobytes()
    words = a.weight > 0
    assert words.any() and np.all(b.weight[words] > a.weight[words])


@pytest.mark.parametrize("cap", [1, 2])
def test_the_iteration_cap(pkg, ctx, cap):
    _, ref = _check(pkg, ctx, *TC.case("random"), 10, 3, max_iterations=cap, ref=TC.recursive("random", 10, 3, cap))
    assert ref.stats["level_iterations"] == [cap] * 3 and ref.stats["level_capped"][:2] == [1, 10]


def test_seeds_and_repeats(pkg, ctx):
    """Two seeds give different trees; the same seed again, after another configuration, and on a
    fresh trainer gives the same bytes."""
    desc, counts = TC.case("clustered")
    tr = _trainer(pkg, ctx, desc, counts)
    first = tr.train(10, 3, seed=0)
    _equals(first, tr.stats, TC.recursive("clustered", 10, 3))
    other = tr.train(10, 3, seed=1)
    _equals(other, tr.stats, TC.recursive("clustered", 10, 3, 100, 1))
    assert other.descriptor.tobytes() != first.descriptor.tobytes()
    _equals(tr.train(17, 2), tr.stats, TC.recursive("clustered", 17, 2))
    again = tr.train(10, 3, seed=0)
    fresh = _trainer(pkg, ctx, desc, counts)
    new = fresh.train(10, 3, seed=0)
    for v in (again, new):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(v, first))
    tr.close()
    fresh.close()


def test_add_in_one_call_in_three_and_after_a_training(pkg, ctx):
    desc, counts = TC.case("gaps")
    images = TC.images(desc, counts)
    ref = TC.recursive("gaps", 10, 3)
    tr = pkg.BowTrainer(ctx, len(images), desc.shape[0])  # exactly full at the end
    tr.add(images[:1])
    tr.add(images[1:6])
    part = tr.train(10, 3)  # a training in between: the next one sees every image
    _equals(part, tr.stats, RT.train_recursive(np.concatenate(images[:6]), counts[:6], 10, 3))
    tr.add(images[6:])
    assert tr.size() == (len(images), desc.shape[0])
    _equals(tr.train(10, 3), tr.stats, ref)
    tr.close()


def test_add_from_a_device_pointer(pkg, ctx):
    import torch

    desc, counts = TC.case("gaps")
    rows = torch.from_numpy(desc).cuda()
    cnt = np.array(counts, np.int32)
    torch.cuda.synchronize()
    tr = pkg.BowTrainer(ctx, len(counts), desc.shape[0])
    assert ctx.lib.lislam_bow_trainer_add(tr.h, ctypes.c_void_p(rows.data_ptr()), pkg.native.ptr(cnt), len(counts)) == 0
    _equals(tr.train(10, 3), tr.stats, TC.recursive("gaps", 10, 3))
    tr.close()


def test_add_batch_reads_the_orb_descriptors_on_the_device(pkg, synth, ctx):
    """add_batch over 8 scans of 64 x 1024 is byte-equal to add of the downloaded
    OUT_ORB_DESCRIPTORS, in one range or two; LISLAM_ERR_STATE before the ORB front end has run."""
    nat = pkg.native
    b = pkg.Batch(ctx, 8)
    b.upload(synth.make_sequence(8, 64, 1024))
    b.extract(8)
    dev, two, host = (pkg.BowTrainer(ctx, 8, 8000) for _ in range(3))
    assert ctx.lib.lislam_bow_trainer_add_batch(dev.h, b.h, 0, 8) == nat.ERR_STATE and ctx.lib.lislam_last_error(ctx.h)
    assert dev.size() == (0, 0)
    b.intensity_odometry(8, 1000)
    dev.add_batch(b, 0, 8)
    two.add_batch(b, 0, 3)
    two.add_batch(b, 3, 5)
    desc = [b.download(nat.OUT_ORB_DESCRIPTORS, k) for k in range(8)]
    assert all(0 < d.shape[0] <= 1000 for d in desc)
    host.add(desc)
    assert dev.size() == two.size() == host.size() == (8, sum(d.shape[0] for d in desc))
    vh = host.train(10, 2)
    for t in (dev, two):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(t.train(10, 2), vh))
    assert vh.parent.shape[0] > 11 and host.stats.level_clustered[0] == 1
    _equals(vh, host.stats, RT.train_recursive(np.concatenate(desc), [d.shape[0] for d in desc], 10, 2))
    # no room for a ninth scan
    assert ctx.lib.lislam_bow_trainer_add_batch(dev.h, b.h, 0, 1) == nat.ERR_CAPACITY and dev.size() == host.size()
    for o in (dev, two, host, b):
        o.close()


def test_database_over_the_trained_vocabulary(pkg, ctx):
    """End to end: the trained tree as a BowDatabase over a sequence that revisits earlier images;
    transform, the BoW vectors and detect equal the stateful restatement over the same arrays."""
    desc, counts = TC.case("clustered")
    images = TC.images(desc, counts)
    tr = _trainer(pkg, ctx, desc, counts)
    voc = tr.train(10, 3)
    ref = TC.recursive("clustered", 10, 3)
    _equals(voc, tr.stats, ref)
    frames = images[:30] + [images[3], images[17], images[8][: len(images[8]) // 2], images[0]] + images[30:]
    kw = dict(min_loop_search_gap=5, loop_index_bound=1000)
    rvoc = RB.Vocabulary(ref.parent, ref.descriptor, ref.weight)
    loops, rets, _, rdb = RB.run_stateful(rvoc, frames, dict(RB.DEFAULTS, **kw))
    db = tr.database(len(frames), max_features=max(counts), **kw)
    words, weights = db.transform(desc[:700])
    rw, rwt = rvoc.transform(desc[:700])
    assert np.array_equal(words, rw) and weights.tobytes() == rwt.tobytes()
    db.add(frames)
    for i in range(len(frames)):
        w, v = db.bow_vector(i)
        ew, ev = RB.vector_arrays(rdb.vectors[i])
        assert w.tobytes() == ew.tobytes() and v.tobytes() == ev.tobytes(), i
    got = db.detect()
    assert list(got.loop_id) == loops
    for k, (ids, scores) in enumerate(zip(got.ids, got.scores)):
        assert list(ids) == [r[0] for r in rets[k]] and scores.tobytes() == np.array([r[1] for r in rets[k]]).tobytes(), k
    assert got.ids[30][0] == 3 and got.ids[31][0] == 17 and got.ids[33][0] == 0  # the revisits find their images
    db.close()
    tr.close()


def test_errors_add_nothing_and_set_the_message(pkg, ctx):
    nat, lib = pkg.native, ctx.lib

    def err():
        return lib.lislam_last_error(ctx.h).decode()

    h = ctypes.c_void_p()
    assert lib.lislam_bow_trainer_create(ctx.h, 0, 10, ctypes.byref(h)) == nat.ERR_ARG and err()
    assert lib.lislam_bow_trainer_create(ctx.h, 4, nat.BOW_TRAIN_MAX_DESCRIPTORS + 1, ctypes.byref(h)) == nat.ERR_CAPACITY
    desc, counts = TC.case("identical")
    tr = pkg.BowTrainer(ctx, len(counts) + 1, desc.shape[0] + 5)
    out = np.zeros(8, np.int32)
    assert lib.lislam_bow_trainer_vocabulary(tr.h, 8, nat.ptr(out), None, None) == nat.ERR_STATE and "lislam_bow_train" in err()
    tr.add(TC.images(desc, counts))
    n = ctypes.c_int32()
    for kw in (dict(k=1), dict(k=65), dict(L=0), dict(L=11), dict(max_iterations=0)):
        cfg = nat.BowTrainConfig(**kw)
        assert lib.lislam_bow_train(tr.h, ctypes.byref(cfg), ctypes.byref(n), None) == nat.ERR_ARG and "lislam_bow_train" in err(), kw
    rows = np.zeros((6, 32), np.uint8)
    six, two, neg = np.array([6], np.int32), np.array([1, 1], np.int32), np.array([-1], np.int32)
    assert lib.lislam_bow_trainer_add(tr.h, nat.ptr(rows), nat.ptr(six), 1) == nat.ERR_CAPACITY and "descriptors" in err()
    assert lib.lislam_bow_trainer_add(tr.h, nat.ptr(rows), nat.ptr(two), 2) == nat.ERR_CAPACITY and "images" in err()
    assert lib.lislam_bow_trainer_add(tr.h, nat.ptr(rows), nat.ptr(neg), 1) == nat.ERR_ARG and "counts[0]" in err()
    assert lib.lislam_bow_trainer_add(tr.h, None, nat.ptr(six), 1) == nat.ERR_ARG and "null" in err()
    other = pkg.Context(n_scans=16, width=256)
    ob = pkg.Batch(other, 1)
    assert lib.lislam_bow_trainer_add_batch(tr.h, ob.h, 0, 1) == nat.ERR_ARG and "another context" in err()
    ob.close()
    other.close()
    fresh = pkg.Batch(ctx, 2)
    assert lib.lislam_bow_trainer_add_batch(tr.h, fresh.h, 0, 1) == nat.ERR_STATE and "intensity_odometry" in err()
    assert lib.lislam_bow_trainer_add_batch(tr.h, fresh.h, 1, 2) == nat.ERR_ARG and "range" in err()
    fresh.close()
    assert tr.size() == (len(counts), desc.shape[0])
    voc = tr.train(3, 4)
    _equals(voc, tr.stats, TC.recursive("identical", 3, 4))
    assert lib.lislam_bow_trainer_vocabulary(tr.h, 4, nat.ptr(out), None, None) == nat.ERR_CAPACITY and "capacity" in err()
    tr.close()
