"""lislam_set_distortion on the GPU (the DISTORTION 1 instantiations of k_odom_assoc16 and k_odom_lm2,
k_odom_to_end, k_target_index_round) against the CPU restatement of the reference's DISTORTION switch (tests/restate_deskew.py, pinned by
test_deskew_restate_cpu.py), on the 16 x 256 frames of tests/odom_cases.py:

i.   LaserOdometry.step over the living node's five frames (with the negative-relTime quirk: queries with
     s > 1, s near 10 and s < 0), where mode 2's targets are the previous step's to-end clouds;
ii.  Batch.odometry over the nine chain scans, chain_len 8 and 3, plain and gated, every variant;
iii. the node's degenerate pairs (0 / 1 / 17 targets, 0 / 1 / 16 queries, one line, all empty);
iv.  every batch case under LISLAM_ENGINE_OFF, AUTO and ON: bit-identical outputs, per-round launches.

stats equal; para and pose within 1e-4 m / 1e-4 rad (the measured maxima are printed: about 1e-12 is
expected, the two sides differ in sin / acos (ocml, glibc) and in the solve's factorization); in mode 2
every coordinate of outputs 22-24 within one float32 ulp and every intensity equal.  The batch's
reference consumes the feature clouds the device extracted, so only the odometry is under test here.
Mode 0 after set_distortion(OFF) is bit-equal to a context that never called it."""
import numpy as np
import pytest

import deskew_cases as D
import odom_cases as C
import restate_deskew as R

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # BASELINE.json north_star: <= 1e-4 m / <= 1e-4 rad
MAXIMA = {}      # mode -> largest |para / pose difference| seen, printed by the last test


@pytest.fixture(scope="module")
def ctx16(pkg):
    c = pkg.Context(n_scans=16, width=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batches(pkg, ctx16, synth):
    """variant -> (batch with the nine scans extracted, their feature clouds as the device extracted them)."""
    out = {}
    for variant in C.CHAIN_VARIANTS:
        b = pkg.Batch(ctx16, 9)
        b.upload(C.chain_scans(synth, variant))
        b.extract(9)
        out[variant] = (b, [b.features(k) for k in range(9)])
    yield out
    for b, _ in out.values():
        b.close()


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    return get


def ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def note(mode, d):
    MAXIMA[mode] = max(MAXIMA.get(mode, 0.0), float(d))


def check_pose(what, mode, para, pose, stats, ref, k):
    assert np.all(np.isfinite(para)) and np.all(np.isfinite(pose)), (what, k)
    assert np.array_equal(stats[:6], ref.stats[k]), (what, k, stats, ref.stats[k])
    d = max(np.max(np.abs(para - ref.para[k])), np.max(np.abs(pose - ref.pose[k])))
    note(mode, d)
    assert d < POSE_TOL, (what, k, d, para, ref.para[k])


def check_to_end(what, got, want, tally):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.shape[0] == 0:
        return
    assert np.array_equal(got[:, 3], want[:, 3]), what  # int(intensity): exactly
    ulps = np.abs(ordered(got[:, :3]) - ordered(want[:, :3]))
    tally[0] += int(np.count_nonzero(ulps))
    tally[1] += ulps.size
    assert ulps.max() <= 1, (what, int(ulps.max()), got[np.argmax(ulps.max(axis=1))], want[np.argmax(ulps.max(axis=1))])


def run_node(pkg, ctx, mode, frames):
    ctx.set_distortion(mode)
    try:
        odo = pkg.LaserOdometry(ctx)
        try:
            return [odo.step(f) for f in frames]
        finally:
            odo.close()
    finally:
        ctx.set_distortion(ctx.DISTORTION_OFF)


# ------------------------------------------------------------------ i. the living node
@pytest.mark.parametrize("mode", D.MODES)
def test_living_node(pkg, ctx16, oracle, synth, references, mode):
    frames = references("living", lambda: D.living_frames(oracle, synth))
    ref = references(("living", mode), lambda: R.odometry_chain(frames, mode))
    assert ref.stats[1][0] > 0 and ref.stats[4][0] > 0
    for k, (para, pose, st) in enumerate(run_node(pkg, ctx16, mode, frames)):
        check_pose("living", mode, para, pose, st, ref, k)
    if mode == 2:  # the steps did search the previous step's to-end clouds: mode 1 gives another pose
        m1 = references(("living", 1), lambda: R.odometry_chain(frames, 1))
        assert np.max(np.abs(m1.para[4] - ref.para[4])) > 1e-6


# ------------------------------------------------------------------ iii. the node's degenerate pairs
@pytest.mark.parametrize("name", D.NODE_NAMES)
@pytest.mark.parametrize("mode", D.MODES)
def test_node_case(pkg, ctx16, oracle, synth, references, mode, name):
    pairs = references("pairs", lambda: D.node_pairs(oracle, synth))
    ref = references((name, mode), lambda: R.odometry_chain(list(pairs[name]), mode))
    for k, (para, pose, st) in enumerate(run_node(pkg, ctx16, mode, pairs[name])):
        check_pose(name, mode, para, pose, st, ref, k)


# ------------------------------------------------------------------ ii. + iv. batch chains, every schedule
def run_batch(pkg, ctx, b, mode, schedule, chain_len, gate):
    nat = pkg.native
    ctx.set_distortion(mode)
    ctx.set_odometry_schedule(schedule)
    try:
        b.odometry(9, chain_len, gate)
        ctx.synchronize()
        engine = b.odometry_engine()
        out = {"para": np.stack([b.download(nat.OUT_PARA, k) for k in range(9)]),
               "pose": np.stack([b.download(nat.OUT_POSE, k) for k in range(9)]),
               "stats": np.stack([b.download(nat.OUT_STATS, k) for k in range(9)])}
        if mode == 2:
            for name, what in (("corner", nat.OUT_CORNER_LAST), ("surf", nat.OUT_SURF_LAST), ("full", nat.OUT_FULL_RES_END)):
                out[name] = [b.download(what, k) for k in range(9)]
        return engine, out
    finally:
        ctx.set_odometry_schedule(ctx.ENGINE_AUTO)
        ctx.set_distortion(ctx.DISTORTION_OFF)


TALLY = [0, 0]  # coordinates of outputs 22-24 that differ at all / compared


@pytest.mark.parametrize("gated", (False, True), ids=("plain", "gated"))
@pytest.mark.parametrize("chain_len", (8, 3))
@pytest.mark.parametrize("variant", C.CHAIN_VARIANTS)
@pytest.mark.parametrize("mode", D.MODES)
def test_batch_chains(pkg, ctx16, batches, references, mode, variant, chain_len, gated):
    b, feats = batches[variant]
    gate = C.USE_ALOAM if gated else None
    ref = references((variant, mode, chain_len, gated), lambda: R.batch_chains(feats, mode, chain_len, gate))
    runs = {}
    for schedule in (ctx16.ENGINE_OFF, ctx16.ENGINE_AUTO, ctx16.ENGINE_ON):
        engine, runs[schedule] = run_batch(pkg, ctx16, b, mode, schedule, chain_len, gate)
        assert engine == 0, (schedule, engine)  # modes 1 / 2 resolve to the per-round launches
    out = runs[ctx16.ENGINE_OFF]
    what = (variant, mode, chain_len, gated)
    for k in range(9):
        check_pose(what, mode, out["para"][k], out["pose"][k], out["stats"][k], ref, k)
    if mode == 2:
        for k in range(9):
            check_to_end(what + ("corner", k), out["corner"][k], ref.corner_last[k], TALLY)
            check_to_end(what + ("surf", k), out["surf"][k], ref.surf_last[k], TALLY)
            check_to_end(what + ("full", k), out["full"][k], ref.full_end[k], TALLY)
    for schedule in (ctx16.ENGINE_AUTO, ctx16.ENGINE_ON):  # the schedule setting changes nothing: bit for bit
        for key, v in out.items():
            w = runs[schedule][key]
            same = all(np.array_equal(x, y) for x, y in zip(v, w)) if isinstance(v, list) else np.array_equal(v, w)
            assert same, (what, schedule, key)


def test_solved_pairs_exist(batches, references):
    """The batch cases above compare real solves: most pairs of the default chain have correspondences."""
    _, feats = batches["default"]
    for mode in D.MODES:
        ref = references(("default", mode, 8, False), lambda: R.batch_chains(feats, mode, 8, None))
        assert np.count_nonzero(ref.stats[:, 0] + ref.stats[:, 1]) >= 4


# ------------------------------------------------------------------ mode 0 and the outputs' life
def test_mode_off_is_untouched(pkg, ctx16, batches):
    nat = pkg.native
    b, _ = batches["default"]
    with pkg.Context(n_scans=16, width=256) as fresh:  # never calls set_distortion
        fb = pkg.Batch(fresh, 9)
        try:
            fb.upload(C.chain_scans(pkg.synth, "default"))
            fb.extract(9)
            fresh.set_odometry_schedule(fresh.ENGINE_OFF)
            fb.odometry(9, 3)
            fresh.synchronize()
            want = [np.stack([fb.download(w, k) for k in range(9)]) for w in (nat.OUT_PARA, nat.OUT_POSE, nat.OUT_STATS)]
            with pytest.raises(nat.LislamError, match="LISLAM_DISTORTION_TO_END"):
                fb.download(nat.OUT_CORNER_LAST, 0)
        finally:
            fb.close()
    run_batch(pkg, ctx16, b, 2, ctx16.ENGINE_OFF, 3, None)  # leaves the context in DISTORTION_OFF
    ctx16.set_distortion(ctx16.DISTORTION_OFF)
    ctx16.set_odometry_schedule(ctx16.ENGINE_OFF)
    try:
        b.odometry(9, 3)
        ctx16.synchronize()
        got = [np.stack([b.download(w, k) for k in range(9)]) for w in (nat.OUT_PARA, nat.OUT_POSE, nat.OUT_STATS)]
        for what in (nat.OUT_CORNER_LAST, nat.OUT_SURF_LAST, nat.OUT_FULL_RES_END):
            with pytest.raises(nat.LislamError, match="LISLAM_DISTORTION_TO_END"):  # the mode-2 call's clouds are gone
                b.download(what, 0)
            with pytest.raises(nat.LislamError):
                b.download_cloud(what, 0)
    finally:
        ctx16.set_odometry_schedule(ctx16.ENGINE_AUTO)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    with pytest.raises(nat.LislamError):
        ctx16.set_distortion(3)


def test_to_end_clouds_pack_like_the_others(pkg, ctx16, batches):
    nat = pkg.native
    b, _ = batches["default"]
    ctx16.set_distortion(ctx16.DISTORTION_TO_END)
    try:
        b.odometry(9, 8)
        for what in (nat.OUT_CORNER_LAST, nat.OUT_SURF_LAST, nat.OUT_FULL_RES_END):
            pts = b.download(what, 2)
            raw = np.frombuffer(b.download_cloud(what, 2), np.float32).reshape(-1, 8)  # PCL PointXYZI: x y z . i . . .
            assert raw.shape[0] == pts.shape[0] > 0
            assert np.array_equal(raw[:, :3], pts[:, :3]) and np.array_equal(raw[:, 4], pts[:, 3])
        # outputs 3, 8, 10 stay as extraction left them
        assert np.any(b.download(nat.OUT_LESS_FLAT, 2)[:, 3] != b.download(nat.OUT_SURF_LAST, 2)[:, 3])
        with pytest.raises(nat.LislamError):  # only the scans of the call
            b.odometry(5, 8)
            b.download(nat.OUT_SURF_LAST, 7)
    finally:
        ctx16.set_distortion(ctx16.DISTORTION_OFF)


def test_zz_report_measured_maxima():
    """Prints what the tests above measured (DESIGN.md section 2 quotes it)."""
    print("\ndeskew parity: max |para / pose difference| per mode:", {m: f"{v:.3e}" for m, v in sorted(MAXIMA.items())})
    if TALLY[1]:
        print(f"deskew parity: outputs 22-24: {TALLY[0]} of {TALLY[1]} coordinates differ at all "
              f"({100.0 * TALLY[0] / TALLY[1]:.5f} %), none by more than one float32 ulp")
    assert set(MAXIMA) == set(D.MODES)
