"""Engine pairing (include/lislam.h, lislam_set_engine_pairing): at depth > 1 the library's dispatcher (a
host thread per device) may run the chains of two batches as ONE split-engine launch (k_odom_roles2 + k_odom_items2), one
chain's solve beside the other's association.  Which launch runs a chain must not change what it
computes.  Every case checks every pair's para, pose, correspondence counts and LM iterations against
the oracle's chain over the same scans (the tolerances of test_gpu_chain.check_chain).  The oracle's
chain reports no LM terminations (oracle.odometry_chain returns six stats per scan), so every case
also compares its outputs, the terminations (stats 6, 7) included, array for array with an unpaired
launch of the same batch: it is the same arithmetic in the same order per chain."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # BASELINE.json north_star: <= 1e-4 m / <= 1e-4 rad (test_gpu_chain.check_chain)


@pytest.fixture(scope="module")
def refs(oracle, synth):
    """(scans, pose, rel, stats) of corridor stretches, computed once: key = (start, n_scans)."""
    cache = {}

    def get(start, n):
        if (start, n) not in cache:
            scans = synth.make_sequence(n, start=start)
            feats = [oracle.scan_registration(s) for s in scans]
            cache[(start, n)] = (scans,) + tuple(oracle.odometry_chain(feats))
        return cache[(start, n)]

    return get


def snapshot(pkg, b, n):
    nat = pkg.native
    return {name: [b.download(what, k) for k in range(n)]
            for name, what in (("para", nat.OUT_PARA), ("pose", nat.OUT_POSE), ("stats", nat.OUT_STATS))}


def check_against_oracle(snap, ref):
    _, pose, rel, st = ref
    for j in range(1, len(pose)):
        d = max(np.max(np.abs(snap["para"][j] - rel[j])), np.max(np.abs(snap["pose"][j] - pose[j])))
        assert d < POSE_TOL, (j, snap["para"][j], rel[j], snap["pose"][j], pose[j])
        assert np.array_equal(snap["stats"][j][:6], st[j][:6]), (j, snap["stats"][j], st[j])  # correspondences + LM iterations


def check_identical(snap, ref_snap):
    """Array for array (para, pose and all eight stats: the LM terminations too)."""
    for name in ("para", "pose", "stats"):
        assert len(snap[name]) == len(ref_snap[name])
        for k, (x, y) in enumerate(zip(snap[name], ref_snap[name])):
            assert np.array_equal(x, y), (name, k, x, y)


def run_two(pkg, specs, pairing, qpw=None, steps=1):
    """One context per spec (engine shape (qpw[i], 5), the given pairing mode), one batch each over
    specs[i] = (scans, ...), each context queued from its own host thread for `steps` steps.
    Returns per batch the snapshot of every step, the paired flag of every step, and the status."""
    ctxs = [pkg.Context(n_scans=64, width=1024) for _ in specs]
    bats = []
    out = [{"snaps": [], "paired": [], "status": None, "engine": None} for _ in specs]
    errors = []
    try:
        for c, q in zip(ctxs, qpw or (3,) * len(specs)):
            c.set_engine_shape(q, 5)
            c.set_engine_pairing(pairing)
            c.set_odometry_schedule(c.ENGINE_ON)
        bats = [pkg.Batch(c, len(s[0])) for c, s in zip(ctxs, specs)]
        for b, s in zip(bats, specs):
            b.upload(s[0])

        def worker(i):
            try:
                n = len(specs[i][0])
                for _ in range(steps):
                    bats[i].extract(n)
                    bats[i].odometry(n, n - 1)
                    out[i]["paired"].append(bats[i].odometry_paired())
                    out[i]["snaps"].append(snapshot(pkg, bats[i], n))
                out[i]["engine"] = bats[i].odometry_engine()
                out[i]["status"] = bats[i].odometry_status()
            except BaseException as e:  # re-raised on the calling thread
                errors.append(e)

        ths = [threading.Thread(target=worker, args=(i,)) for i in range(len(specs))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errors:
            raise errors[0]
    finally:
        for b in bats:
            b.close()
        for c in ctxs:
            c.close()
    return out


@pytest.fixture(scope="module")
def unpaired(pkg, refs):
    """The outputs of an unpaired engine launch (pairing off) of a stretch, computed once per key."""
    cache = {}

    def get(*keys):
        missing = [k for k in keys if k not in cache]
        if missing:
            out = run_two(pkg, [refs(*k) for k in missing], pkg.Context.PAIRING_OFF)
            for k, o in zip(missing, out):
                assert o["paired"] == [0] and o["status"] == 0 and o["engine"] == 2, (k, o["paired"], o["status"])
                cache[k] = o["snaps"][0]
        return [cache[k] for k in keys]

    return get


@pytest.fixture(scope="module")
def required_pair(pkg, refs):
    """Case 1's run (pairing required, two 6-scan batches), shared with the pairing-off case."""
    specs = [refs(100, 6), refs(700, 6)]
    return specs, run_two(pkg, specs, pkg.Context.PAIRING_REQUIRE)


def test_paired_launch_equal_lengths(required_pair, unpaired):
    specs, out = required_pair
    for o, ref, un in zip(out, specs, unpaired((100, 6), (700, 6))):
        assert o["paired"] == [1] and o["status"] == 0 and o["engine"] == 2, o["paired"]
        check_against_oracle(o["snaps"][0], ref)
        check_identical(o["snaps"][0], un)


def test_paired_launch_unequal_lengths(pkg, refs, unpaired):
    """5 and 8 scans: the shorter chain ends first, the launch goes on for the longer one."""
    specs = [refs(250, 5), refs(1000, 8)]
    out = run_two(pkg, specs, pkg.Context.PAIRING_REQUIRE)
    for o, ref, un in zip(out, specs, unpaired((250, 5), (1000, 8))):
        assert o["paired"] == [1] and o["status"] == 0, o["paired"]
        check_against_oracle(o["snaps"][0], ref)
        check_identical(o["snaps"][0], un)


def test_second_step_on_the_same_batches(pkg, refs, unpaired):
    """The control words, records and shares of a paired launch are reused by the next one."""
    specs = [refs(100, 6), refs(700, 6)]
    out = run_two(pkg, specs, pkg.Context.PAIRING_REQUIRE, steps=2)
    for o, ref, un in zip(out, specs, unpaired((100, 6), (700, 6))):
        assert o["paired"] == [1, 1] and o["status"] == 0, o["paired"]
        for snap in o["snaps"]:
            check_against_oracle(snap, ref)
            check_identical(snap, un)


def test_incompatible_requests_are_not_paired(pkg, refs, unpaired):
    """Three queries per wavefront and one: two item builds, never one launch."""
    specs = [refs(100, 6), refs(700, 6)]
    out = run_two(pkg, specs, pkg.Context.PAIRING_AUTO, qpw=(3, 1))
    for o, ref in zip(out, specs):
        assert o["paired"] == [0] and o["status"] == 0, o["paired"]
        check_against_oracle(o["snaps"][0], ref)
    check_identical(out[0]["snaps"][0], unpaired((100, 6))[0])  # (the qpw-3 batch: qpw-1 items sum in another order)


def test_pairing_off_is_the_same_arithmetic(pkg, required_pair):
    """Unpaired launches of the same batches: identical outputs, array for array."""
    specs, paired = required_pair
    out = run_two(pkg, specs, pkg.Context.PAIRING_OFF)
    for o, p in zip(out, paired):
        assert o["paired"] == [0] and o["status"] == 0, o["paired"]
        check_identical(o["snaps"][0], p["snaps"][0])


BENCH_STARTS = (100, 400, 700, 1000)


def bench_schedule_run(pkg, specs, steps=8):
    """bench.pipeline over one context per spec at the throughput shape, pairing auto (the default).
    Returns the paired flag of every step's launch, per batch the status and abort code, and every
    batch's last outputs.  A step's flag is read where its batch's next call would settle the launch
    anyway: right before the batch's next extraction (through bench.pipeline's `call` hook), and
    after the last step; so reading it does not change the schedule."""
    import bench

    k, S = len(specs), len(specs[0][0])
    ctxs = [pkg.Context(n_scans=64, width=1024) for _ in range(k)]
    for c in ctxs:
        c.set_engine_shape(*c.SHAPE_THROUGHPUT)
    bats = [pkg.Batch(c, S) for c in ctxs]
    flags = {}

    def call(name, st, f, *a):
        if name == "extract" and st >= k:
            flags[st - k] = f.__self__.odometry_paired()
        return f(*a)

    try:
        for b, s in zip(bats, specs):
            b.upload(s[0])
        bench.pipeline(bats, S, steps, S - 1, k, (1000, pkg.intensity.set_mask(64, 1024)), call)
        for c in ctxs:
            c.synchronize()
        queues = ctxs[0].masked_queues()
        for st in range(max(0, steps - k), steps):
            flags[st] = bats[st % k].odometry_paired()
        status = [(b.odometry_status(), b.odometry_abort_code()) for b in bats]
        snaps = [snapshot(pkg, b, S) for b in bats]
    finally:
        for b in bats:
            b.close()
        for c in ctxs:
            c.close()
    return [flags[st] for st in range(steps)], status, snaps, queues


def test_pairs_under_the_bench_schedule(pkg, refs, unpaired):
    """bench.pipeline over 4 contexts x 8 steps of 61 scans at the throughput shape, pairing auto
    (the default): no launch gave up, every context's last step is the oracle's and, array for
    array, an unpaired launch's, and some launch was shared.

    Whether two requests meet under pairing auto depends on when each context's extraction ends, so
    one run of the schedule need not pair anything in a given launch: over 13 runs on an MI355X
    every run shared 2 to 6 of its 8 launches, 5 runs none of the first four and 1 run none of the
    last four (each batch's last launch, all that lislam_batch_odometry_paired reports at the end).
    So every step's flag counts, and the schedule is run again, at most three times in all, each
    run checked in full, until a launch was shared: from those frequencies a run without any shared
    launch is a few per cent, three in a row below 1e-4."""
    keys = [(start, 61) for start in BENCH_STARTS]
    specs = [refs(*k) for k in keys]
    shared = 0
    for run in range(3):
        flags, status, snaps, queues = bench_schedule_run(pkg, specs)
        print("run", run, "paired flag per step:", flags, "status:", status)
        assert queues <= len(specs) + 10, queues
        for st, code in status:
            assert st == 0, hex(code)
        for snap, ref, un in zip(snaps, specs, unpaired(*keys)):
            check_against_oracle(snap, ref)
            check_identical(snap, un)
        shared += sum(flags)
        if shared:
            break
    assert shared >= 1, shared
