"""Engine segments (include/lislam.h, lislam_set_engine_segment): at depth > 1 the dispatcher runs a
one-chain odometry call as engine launches of L scan pairs each, every one starting from the state
the previous one left, and chooses the chain's partner anew for every launch.  Where a chain is cut,
and with whom it shares a launch, must not change what it computes: every case checks every pair
against the oracle's chain (the tolerances of test_gpu_chain.check_chain, correspondence counts and
LM iterations equal) and, array for array (para, pose, all eight stats), against the same batch run
as one unpaired launch (segment 0, pairing off)."""
import os
import subprocess
import sys
import threading

import pytest

from test_gpu_engine_pairs import (BENCH_STARTS, bench_schedule_run, check_against_oracle, check_identical, refs,  # noqa: F401
                                   snapshot)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_batches(pkg, specs, pairing, segment, steps=1):
    """One context per spec at engine shape (3, 5) with the given pairing mode and segment, one batch
    each over specs[i] = (scans, ...), each context queued from its own host thread; the threads meet
    at a barrier before every step's odometry call, so under PAIRING_REQUIRE both requests of a step
    are fresh together.  Returns per batch every step's snapshot and paired flag, and the status."""
    ctxs = [pkg.Context(n_scans=64, width=1024) for _ in specs]
    bats = []
    out = [{"snaps": [], "paired": [], "status": None, "engine": None} for _ in specs]
    errors = []
    gate = threading.Barrier(len(specs))
    try:
        for c in ctxs:
            c.set_engine_shape(3, 5)
            c.set_engine_pairing(pairing)
            c.set_engine_segment(segment)
            c.set_odometry_schedule(c.ENGINE_ON)
        bats = [pkg.Batch(c, len(s[0])) for c, s in zip(ctxs, specs)]
        for b, s in zip(bats, specs):
            b.upload(s[0])

        def worker(i):
            try:
                n = len(specs[i][0])
                for _ in range(steps):
                    bats[i].extract(n)
                    gate.wait(timeout=60)
                    bats[i].odometry(n, n - 1)
                    out[i]["paired"].append(bats[i].odometry_paired())
                    out[i]["snaps"].append(snapshot(pkg, bats[i], n))
                out[i]["engine"] = bats[i].odometry_engine()
                out[i]["status"] = bats[i].odometry_status()
            except BaseException as e:  # re-raised on the calling thread
                gate.abort()
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
def whole(pkg, refs):
    """The outputs of one unpaired launch of the whole chain (segment 0, pairing off) of a stretch,
    computed once per key."""
    cache = {}

    def get(*keys):
        missing = [k for k in keys if k not in cache]
        if missing:
            out = run_batches(pkg, [refs(*k) for k in missing], pkg.Context.PAIRING_OFF, 0)
            for k, o in zip(missing, out):
                assert o["paired"] == [0] and o["status"] == 0 and o["engine"] == 2, (k, o["paired"], o["status"])
                cache[k] = o["snaps"][0]
        return [cache[k] for k in keys]

    return get


@pytest.mark.parametrize("segment", [3, 1, 8])
def test_one_chain_in_segments(pkg, refs, whole, segment):
    """A 9-scan batch (8 pairs), pairing off: segments of 3 + 3 + 2 (an uneven tail), of 1 (a
    boundary after every pair) and of 8 (a single segment)."""
    key = (550, 9)
    (o,) = run_batches(pkg, [refs(*key)], pkg.Context.PAIRING_OFF, segment)
    assert o["paired"] == [0] and o["status"] == 0 and o["engine"] == 2, (o["paired"], o["status"])
    check_against_oracle(o["snaps"][0], refs(*key))
    check_identical(o["snaps"][0], whole(key)[0])


@pytest.fixture(scope="module")
def two_steps(pkg, refs):
    """5 and 8 scans (4 and 7 pairs), pairing required, segment 2, two steps: the chains share the
    launches of rounds 0-1 and 2-3, then the longer one goes on alone (2 + 1 rounds)."""
    specs = [refs(250, 5), refs(1000, 8)]
    return specs, run_batches(pkg, specs, pkg.Context.PAIRING_REQUIRE, 2, steps=2)


def test_partners_change_mid_chain(two_steps, whole):
    specs, out = two_steps
    for o, ref, un in zip(out, specs, whole((250, 5), (1000, 8))):
        assert o["paired"][0] == 1 and o["status"] == 0 and o["engine"] == 2, (o["paired"], o["status"])
        check_against_oracle(o["snaps"][0], ref)
        check_identical(o["snaps"][0], un)


def test_second_step_on_the_same_batches(two_steps, whole):
    """The control words, records, shares and the resume state are reused by the next step's segments."""
    specs, out = two_steps
    for o, ref, un in zip(out, specs, whole((250, 5), (1000, 8))):
        assert o["paired"] == [1, 1] and o["status"] == 0, (o["paired"], o["status"])
        check_against_oracle(o["snaps"][1], ref)
        check_identical(o["snaps"][1], un)


def test_segments_under_the_bench_schedule(pkg, refs, whole):
    """bench.pipeline over 4 contexts x 8 steps of 61 scans at the throughput shape with the default
    segment and pairing auto: no launch gave up, every context's last step is the oracle's and, array
    for array, one unpaired launch's, and the masked queues stay within the pairs test's bound.

    The paired share is not asserted: whether two requests meet under pairing auto depends on when
    each context's extraction ends (test_gpu_engine_pairs.test_pairs_under_the_bench_schedule saw
    runs with none of four launches shared), and the flags are printed instead."""
    keys = [(start, 61) for start in BENCH_STARTS]
    specs = [refs(*k) for k in keys]
    flags, status, snaps, queues = bench_schedule_run(pkg, specs)
    print("paired flag per step:", flags, "status:", status)
    assert queues <= len(specs) + 10, queues
    for st, code in status:
        assert st == 0, hex(code)
    for snap, ref, un in zip(snaps, specs, whole(*keys)):
        check_against_oracle(snap, ref)
        check_identical(snap, un)


def test_give_up_under_the_dispatcher():
    """Two batches pending on the dispatcher at shape (3, 5), segment 2, with the library's bounded
    device waits cut to 1 us (LISLAM_ENGINE_WAIT_US=1: every wait expires at once and the kernels
    return): each chain ends at its first segment, is re-run on the per-round schedule, and its
    outputs equal that schedule's.  In a child process, so the variable does not leak."""
    env = dict(os.environ, LISLAM_ENGINE_WAIT_US="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "engine_segment_giveup.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "give-up recovered" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
