"""Scan-to-scan odometry on blank, sparse and tiny clouds (tests/odom_cases.py) under every schedule,
against the CPU oracle computed at run time: para and pose within POSE_TOL, stats[:6] (correspondence
counts and LM iterations of both passes) equal, no engine give-up.  The LM terminations (stats 6, 7)
have no oracle counterpart and are compared between schedules only, with para and pose to 1e-9.
tests/test_odom_cases_cpu.py shows on the oracle alone that the cases are sound: which give exactly
zero correspondences, that the others give some, and that all are stable under one-ulp nudges.

The contract these pin (odometry): a blank or featureless frame yields zero correspondences
and zero iterations, para is carried, the pose accumulates it, and no schedule gives up.

What each group guards (csrc/lislam_odometry.hip unless noted):

a. Node cases (LaserOdometry.step, per-round launches and the engine's solo items at 16 x 256).
   targets_k: target_index_body's `n == 0` return after the target chunk boxes, the P = 1024 padding,
   nch / nsu of one chunk, one super-chunk and their first multiples (15 / 16 / 17, 31 / 33, 200), the
   `u * kSuper < n` guards of the register path; nn16 / nn_wave / ls16 / line_search on a cloud of one
   partial chunk.  queries_k: k_odom_assoc16's qblocks and the engine's live items (eng_live_items,
   pass_shape) at 0, one partial wave and one item; evaluate2 / eng_solve_pass with ns = nf = 0 and with
   one to three blocks of each kind (rank-deficient J^T J through lislam_lm.hpp); the role's turn on a
   pass without queries (eng_solve_role, the assoc_done / lm_gen hand-over).  one_line, every_4th_line,
   identical_targets: the second / third neighbour must lie on another line within 2.5 (ls16_need,
   ls_need, the label ranges of chunk_boxes' w), else no correspondence; identical_targets also the
   `ext = max(..., 1e-6f)` cell size of coincident points.  lines_0_1, every_2nd_line: the same searches
   at the lowest lines and at a line distance of 2.  shift_0.4 / shift_6: the 25 m^2 gate on the 1-NN
   seed from feat_loff and on the box lower bounds (box_lb).  all_empty: every kernel at n = 0.
   Capacity: put_frame (lislam_abi.cpp) refuses n_sharp = cap_sharp + 1.
b. A node that lives on: copy_slot (lislam_abi.cpp) of a slot without targets, whose sorted / nn_chunk
   arrays still hold the previous frame's index, then of a one-query frame; nothing stale may reach
   the next pair.
c. Large targets (64 x 1024): k_target_index<8, 32> / k_target_index_all's `in_regs` switch at
   P > 64 kK kW = 16384 keys (wg_bitonic in registers up to 16384 points, global_bitonic plus the second
   chunk_boxes pass from 16385), with P = 32768 and 65536 beyond it, and the P = 1024 floor at
   1023 / 1024 / 1025 points.
d. Batch chains (Batch.extract + odometry): the same blank / thin / all-near scans extracted on the
   device (k_scan_*, compared bit-exact first), through k_target_index_all and then the per-round
   launches (k_odom_assoc16, k_odom_lm2), the split engine (k_odom_roles with k_odom_items_solo at one
   query per wave, k_odom_items<3> and <4>), and the single-launch engine (k_odom_chain); chains that
   start and end on the blank scan (k_odom_init, pair_of) and the gated chain (eng_live_items' gate).
e. Paired launch: k_odom_roles2 / k_odom_items2 with one chain whose passes have no items beside an
   ordinary chain (TwoBatches::of, the shared ticket queue)."""
import ctypes
import os
import threading

import numpy as np
import pytest

import odom_cases as C
from test_gpu_chain import check_chain
from test_gpu_engine_pairs import check_against_oracle, check_identical, snapshot
from test_gpu_parity import assert_features_equal
from test_odom_cases_cpu import UNSTABLE

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4       # BASELINE.json north_star: <= 1e-4 m / <= 1e-4 rad
SCHEDULE_TOL = 1e-9   # between schedules (test_gpu_chain.test_schedules_agree)
NODE_SCHEDULES = ("off", "engine")
NODE_NAMES = tuple(f"targets_{k}" for k in C.TARGETS_K) + tuple(f"queries_{k}" for k in C.QUERIES_K) + (
    "one_line", "lines_0_1", "every_2nd_line", "every_4th_line", "identical_targets", "shift_0.4", "shift_6", "all_empty")
LARGE_NAMES = tuple(f"large_{n}" for n in C.LARGE_POOLED + C.LARGE_SINGLE)


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


@pytest.fixture(scope="module")
def node(oracle, synth):
    cases = C.node_cases(oracle, synth)
    assert tuple(cases) == NODE_NAMES
    return cases


@pytest.fixture(scope="module")
def large(oracle, synth):
    return C.large_target_cases(oracle, synth)


@pytest.fixture(scope="module")
def references(oracle):
    """The oracle's chain over a list of frames, computed once per key."""
    cache = {}

    def get(key, frames):
        if key not in cache:
            cache[key] = oracle.odometry_chain(list(frames))
        return cache[key]

    return get


def mode_of(ctx, schedule):
    return ctx.ENGINE_OFF if schedule == "off" else ctx.ENGINE_ON


def run_node(pkg, ctx, schedule, frames):
    """A fresh node over `frames` under one schedule: [(para, pose, stats)] per frame, and the
    give-ups the node's engine launches counted."""
    ctx.set_odometry_schedule(mode_of(ctx, schedule))
    try:
        odo = pkg.LaserOdometry(ctx)
        try:
            out = [odo.step(f) for f in frames]
            gave_up = odo.status()
        finally:
            odo.close()
    finally:
        ctx.set_odometry_schedule(ctx.ENGINE_AUTO)
    return out, gave_up


@pytest.fixture(scope="module")
def node_runs(pkg):
    """run_node once per (context, schedule, key): the schedule comparison reuses the oracle tests' runs."""
    cache = {}

    def get(ctx, schedule, key, frames):
        k = (id(ctx), schedule, key)
        if k not in cache:
            cache[k] = run_node(pkg, ctx, schedule, frames)
        return cache[k]

    return get


def check_node(name, out, gave_up, ref):
    pose, rel, st = ref
    assert gave_up == 0, (name, gave_up)  # a give-up on a blank pair is a failure, not a recovery
    for k, (para, pw, gst) in enumerate(out):
        assert np.all(np.isfinite(para)) and np.all(np.isfinite(pw)), (name, k, para, pw)
        assert np.all(gst >= 0), (name, k, gst)
        assert np.array_equal(gst[:2], st[k][:2]), (name, k, gst, st[k])  # pass 1's correspondences
        if name in UNSTABLE:  # (test_odom_cases_cpu's stability cap: counts and finiteness only)
            continue
        d = max(np.max(np.abs(para - rel[k])), np.max(np.abs(pw - pose[k])))
        assert d < POSE_TOL, (name, k, para, rel[k], pw, pose[k])
        assert np.array_equal(gst[:6], st[k][:6]), (name, k, gst, st[k])  # ... and LM iterations


def check_schedules_agree(name, a, b):
    for k, ((p0, w0, s0), (p1, w1, s1)) in enumerate(zip(a, b)):
        assert np.max(np.abs(p0 - p1)) < SCHEDULE_TOL, (name, k, p0, p1)
        assert np.max(np.abs(w0 - w1)) < SCHEDULE_TOL, (name, k, w0, w1)
        assert np.array_equal(s0, s1), (name, k, s0, s1)  # all eight: the terminations too


# ------------------------------------------------------------------ a. node cases
@pytest.mark.parametrize("name", NODE_NAMES)
@pytest.mark.parametrize("schedule", NODE_SCHEDULES)  # the slower index: every case per-round first
def test_node_case(pkg, ctx16, node, references, node_runs, schedule, name):
    out, gave_up = node_runs(ctx16, schedule, name, node[name])
    check_node(name, out, gave_up, references(name, node[name]))


@pytest.mark.parametrize("name", NODE_NAMES)
def test_node_case_schedules_agree(ctx16, node, node_runs, name):
    check_schedules_agree(name, node_runs(ctx16, "off", name, node[name])[0], node_runs(ctx16, "engine", name, node[name])[0])


def test_node_refuses_a_cloud_above_its_capacity(pkg, ctx16, node):
    """put_frame checks the counts before anything reaches the device; the node goes on afterwards."""
    nat = pkg.native
    f0, f1 = node["shift_0.4"]
    cap_sharp = 12 * ctx16.n_scans
    big = np.zeros((cap_sharp + 1, 4), np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    arrs = [big] + [np.ascontiguousarray(a, np.float32) for a in (f0.less_sharp, f0.flat, f0.less_flat)]
    fr = nat.Frame(fp(arrs[0]), arrs[0].shape[0], fp(arrs[1]), arrs[1].shape[0], fp(arrs[2]), arrs[2].shape[0],
                   fp(arrs[3]), arrs[3].shape[0])
    odo = pkg.LaserOdometry(ctx16)
    try:
        assert ctx16.lib.lislam_odom_step(odo.h, ctypes.byref(fr), None, None, None) == nat.ERR_CAPACITY
        odo.step(f0)
        para, _, st = odo.step(f1)
        assert np.all(np.isfinite(para)) and st[0] > 0
    finally:
        odo.close()


# ------------------------------------------------------------------ b. a node that lives on
@pytest.fixture(scope="module")
def living(oracle, synth):
    return C.living_node_frames(oracle, synth)


@pytest.mark.parametrize("schedule", NODE_SCHEDULES)
def test_node_lives_on(pkg, ctx16, living, references, node_runs, schedule):
    out, gave_up = node_runs(ctx16, schedule, "living", living)
    check_node("living", out, gave_up, references("living", living))


def test_node_lives_on_schedules_agree(ctx16, living, node_runs):
    check_schedules_agree("living", node_runs(ctx16, "off", "living", living)[0],
                          node_runs(ctx16, "engine", "living", living)[0])


# ------------------------------------------------------------------ c. large targets
@pytest.mark.parametrize("name", LARGE_NAMES)
@pytest.mark.parametrize("schedule", NODE_SCHEDULES)
def test_large_targets(pkg, ctx64, large, references, node_runs, schedule, name):
    out, gave_up = node_runs(ctx64, schedule, name, large[name])
    check_node(name, out, gave_up, references(name, large[name]))


@pytest.mark.parametrize("schedule", NODE_SCHEDULES)
def test_large_targets_both_sides_of_the_sort_boundary(ctx64, large, references, node_runs, schedule):
    """Every schedule has run a target at the last in-register size and one at the first global one."""
    below, above = f"large_{C.SORT_BOUNDARY}", f"large_{C.SORT_BOUNDARY + 1}"
    assert large[below][0].less_flat.shape[0] == C.SORT_BOUNDARY and large[above][0].less_flat.shape[0] == C.SORT_BOUNDARY + 1
    for name in (below, above):
        out, gave_up = node_runs(ctx64, schedule, name, large[name])
        check_node(name, out, gave_up, references(name, large[name]))


@pytest.mark.parametrize("name", LARGE_NAMES)
def test_large_targets_schedules_agree(ctx64, large, node_runs, name):
    check_schedules_agree(name, node_runs(ctx64, "off", name, large[name])[0], node_runs(ctx64, "engine", name, large[name])[0])


# ------------------------------------------------------------------ d. batch chains
CHAIN_SCHEDULES = ("off", "engine", "single", "qpw1", "qpw3", "qpw4")


@pytest.fixture(scope="module")
def chains(oracle, synth):
    """variant -> (scans, feats), extracted by the oracle once."""
    cache = {}

    def get(variant):
        if variant not in cache:
            scans = C.chain_scans(synth, variant)
            cache[variant] = (scans, [oracle.scan_registration(s) for s in scans])
        return cache[variant]

    return get


def run_chain(pkg, ctx, scans, schedule, chain_len=None, use_aloam=None):
    """A batch over `scans` after extract + odometry under one schedule (the caller closes it)."""
    S = len(scans)
    ctx.set_odometry_schedule(mode_of(ctx, schedule))
    if schedule == "single":  # as test_gpu_chain.test_continuous_chain_60_pairs_single_launch_engine
        os.environ["LISLAM_ENGINE_SINGLE"] = "1"
    if schedule.startswith("qpw"):
        ctx.set_engine_shape(int(schedule[3:]), 0)
    b = pkg.Batch(ctx, S)
    try:
        b.upload(scans)
        b.extract(S)
        b.odometry(S, chain_len or S - 1, use_aloam=use_aloam)  # the batch's first engine launch reads the variable
        ctx.synchronize()
    except BaseException:
        b.close()
        raise
    finally:
        if schedule == "single":
            del os.environ["LISLAM_ENGINE_SINGLE"]
        ctx.set_engine_shape(1, 0)
        ctx.set_odometry_schedule(ctx.ENGINE_AUTO)
    eng = b.odometry_engine()  # 0 per-round launches, 1 the single-launch engine, 2 the split engine
    assert (eng == 0) == (schedule == "off") and (schedule != "single" or eng == 1), (schedule, eng)
    return b


@pytest.fixture(scope="module")
def chain_runs(pkg, ctx16, chains, references):
    """(variant, schedule) -> the outputs of the continuous chain, run and checked against the oracle
    (test_gpu_chain.check_chain: no give-up, POSE_TOL, stats[:6]) once."""
    cache = {}

    def get(variant, schedule):
        if (variant, schedule) not in cache:
            scans, feats = chains(variant)
            pose, rel, st = references(("chain", variant), feats)
            b = run_chain(pkg, ctx16, scans, schedule)
            try:
                check_chain(pkg, b, feats, pose, rel, st)
                cache[(variant, schedule)] = snapshot(pkg, b, len(scans))
            finally:
                b.close()
        return cache[(variant, schedule)]

    return get


def test_altered_scans_extract_bit_exact(pkg, ctx16, chains):
    """The blank, thin and all-near scans through the device's extraction: a later failure is the
    odometry's."""
    scans, feats = chains("default")
    b = pkg.Batch(ctx16, len(scans))
    try:
        b.upload(scans)
        b.extract(len(scans))
        for k in (3, 5, 7):
            assert_features_equal(pkg, b, k, feats[k])
    finally:
        b.close()


@pytest.mark.parametrize("variant", C.CHAIN_VARIANTS)
@pytest.mark.parametrize("schedule", CHAIN_SCHEDULES)
def test_chain(chain_runs, schedule, variant):
    snap = chain_runs(variant, schedule)
    S = len(snap["para"])
    for k in range(S):
        assert np.all(np.isfinite(snap["para"][k])) and np.all(np.isfinite(snap["pose"][k])) and np.all(snap["stats"][k] >= 0)
    if schedule != "off":
        first = chain_runs(variant, "off")
        check_schedules_agree((variant, schedule), [(first["para"][k], first["pose"][k], first["stats"][k]) for k in range(S)],
                              [(snap["para"][k], snap["pose"][k], snap["stats"][k]) for k in range(S)])


@pytest.mark.parametrize("schedule", ("off", "engine"))
def test_chains_of_three_pairs(pkg, oracle, ctx16, chains, schedule):
    """chain_len = 3: the second chain starts on the blank scan, the first ends on it."""
    scans, feats = chains("default")
    S, L = len(scans), 3
    b = run_chain(pkg, ctx16, scans, schedule, chain_len=L)
    try:
        for c0 in range(0, S - 1, L):
            chain = feats[c0:c0 + L + 1]
            pose, rel, st = oracle.odometry_chain(chain)
            check_chain(pkg, b, chain, pose, rel, st, k0=c0)
    finally:
        b.close()


@pytest.mark.parametrize("schedule", ("off", "engine"))
def test_gated_chain(pkg, oracle, ctx16, chains, schedule):
    scans, feats = chains("default")
    use = np.array(C.USE_ALOAM, np.int32)
    pose, rel, st = oracle.odometry_chain(feats, use_aloam=use)
    b = run_chain(pkg, ctx16, scans, schedule, use_aloam=use)
    try:
        check_chain(pkg, b, feats, pose, rel, st)
    finally:
        b.close()


# ------------------------------------------------------------------ e. paired launch
def run_two_16(pkg, specs, pairing):
    """test_gpu_engine_pairs.run_two's arrangement (engine shape (3, 5), one context and host thread
    per batch, one step) on 16 x 256 contexts, the shape of the degenerate stream."""
    ctxs = [pkg.Context(n_scans=16, width=256) for _ in specs]
    bats = []
    out = [{"snap": None, "paired": None, "status": None, "engine": None} for _ in specs]
    errors = []
    try:
        for c in ctxs:
            c.set_engine_shape(3, 5)
            c.set_engine_pairing(pairing)
            c.set_odometry_schedule(c.ENGINE_ON)
        bats = [pkg.Batch(c, len(s)) for c, s in zip(ctxs, specs)]
        for b, s in zip(bats, specs):
            b.upload(s)

        def worker(i):
            try:
                n = len(specs[i])
                bats[i].extract(n)
                bats[i].odometry(n, n - 1)
                out[i]["paired"] = bats[i].odometry_paired()
                out[i]["snap"] = snapshot(pkg, bats[i], n)
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


def test_paired_with_an_ordinary_chain(pkg, oracle, synth, chains):
    """One ordinary 9-scan batch and the degenerate stream as one launch: both equal their unpaired
    outputs array for array (terminations included) and the oracle, and both report the shared launch."""
    ordinary = synth.make_sequence(9, 16, 256, start=100)
    degenerate, dfeats = chains("default")
    specs = [ordinary, degenerate]
    refs = [(ordinary,) + tuple(oracle.odometry_chain([oracle.scan_registration(s) for s in ordinary])),
            (degenerate,) + tuple(oracle.odometry_chain(dfeats))]
    alone = run_two_16(pkg, specs, pkg.Context.PAIRING_OFF)
    paired = run_two_16(pkg, specs, pkg.Context.PAIRING_REQUIRE)
    for o, p, ref in zip(alone, paired, refs):
        assert o["paired"] == 0 and o["status"] == 0 and o["engine"] == 2, o
        assert p["paired"] == 1 and p["status"] == 0 and p["engine"] == 2, (p["paired"], p["status"], p["engine"])
        check_against_oracle(o["snap"], ref)
        check_against_oracle(p["snap"], ref)
        check_identical(p["snap"], o["snap"])
