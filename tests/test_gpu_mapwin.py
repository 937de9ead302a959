"""GPU parity of mapOptimization's ORB keyframe sliding window (lislam_mapwin_*,
lislam_mapopt_step_window, lislam_orb_detect_map, lislam_batch_mapopt_window) against the CPU
restatement (tests/restate_mapwin.py) on the constructed cases of tests/mapwin_cases.py, whose
properties tests/test_mapwin_cpu.py asserts.

Integer outputs (matches, info, pairs, summaries, map sizes) are exact; record source columns are
float-to-double copies and exact; record destination columns are a handful of fp64 roundings at
|coordinate| <= 250 m and agree within 1e-12 m; poses and states within the suite's POSE_TOL.
"""
import numpy as np
import pytest

import mapwin_cases as C
import restate_mapwin as R

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # BASELINE.json north_star
REC_TOL = 1e-12


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(n_scans=64, width=1024)
    yield c
    c.close()


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _points(n, seed=0):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = np.random.default_rng(seed).uniform(-5, 5, (n, 3))
    return p


IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _fill(win, kfs):
    for d, p, x in kfs:
        win.push(d, p, x)


def _check_records(win, cur, kfs):
    """lislam_mapwin_records of `cur` against the window holding `kfs` (oldest first) vs the restatement."""
    rec, info, pairs = win.records(*cur)
    rrec, rinfo, rpairs, _ = R.window_records([R.Keyframe(*k) for k in kfs], *cur)
    assert np.array_equal(info, rinfo), (info, rinfo)
    assert np.array_equal(pairs, rpairs)
    assert rec.shape == rrec.shape
    assert np.array_equal(rec[:, :3], rrec[:, :3]) and np.array_equal(rec[:, 6:], rrec[:, 6:])
    assert np.max(np.abs(rec[:, 3:6] - rrec[:, 3:6]), initial=0.0) <= REC_TOL
    return rec, info, pairs


@pytest.mark.parametrize("nts", C.MATCH_WINDOWS)
@pytest.mark.parametrize("nq", C.MATCH_NQ)
def test_match(pkg, ctx, nq, nts):
    """Three keyframes of different sizes in one call: train index (the first of equal sums) and the
    exact integer sum per query; -1 against an empty keyframe."""
    q, trains = C.match_case(nq, nts)
    win = pkg.mapping.SlidingWindow(ctx, 3, 512)
    _fill(win, [(t, _points(len(t)), IDENT) for t in trains])
    m = win.match(q)
    assert m.shape == (3, nq, 2)
    for w, t in enumerate(reversed(trains)):  # newest first
        idx, s = R.l2_match_fast(q, t)
        if len(t) == 0:
            assert np.all(m[w] == -1)
        else:
            assert np.array_equal(m[w, :, 0], idx), (w, len(t))
            assert np.array_equal(m[w, :, 1], s), (w, len(t))
        if len(t) >= 8:
            assert m[w, 0, 0] == 2 and m[w, 0, 1] == 0  # rows 2, 5 and nt - 1 are query 0: the first wins
    win.close()


def test_match_extremes(pkg, ctx):
    q, (a, b) = C.extreme_case()
    win = pkg.mapping.SlidingWindow(ctx, 2, 16)
    _fill(win, [(a, _points(1), IDENT), (b, _points(4), IDENT)])
    m = win.match(q)
    assert m[1].tolist() == [[0, C.MAX_SUM], [0, 0]]  # against a: the maximum sum
    assert m[0].tolist() == [[1, 0], [0, 0]]          # against b: the first of the duplicated rows
    win.close()


@pytest.mark.parametrize("nq,nt", C.SELECT_CASES)
def test_selection_boundaries(pkg, ctx, nq, nt):
    """M > 100 and G > 50 (nq = 100, 101, 250: not used; 251: used; M > 100 alone never makes a
    keyframe used, G > 50 implies it), nt == nq not used; a run of equal sums straddles the G-th place,
    so the stable tie rule decides which matches are kept."""
    cur, kf = C.select_case(nq, nt)
    win = pkg.mapping.SlidingWindow(ctx, 1, 512)
    _fill(win, [kf])
    rec, info, pairs = _check_records(win, cur, [kf])
    used = nq > 250 and nt != nq
    assert info[0].tolist()[:4] == [nt, nq, R.good_count(nq), int(used)]
    assert len(rec) == (R.good_count(nq) if used else 0)
    win.close()


def test_records(pkg, ctx):
    """Landmarks seen from two poses with centimetre noise, planted outliers on both sides of the
    gate, three window keyframes (one with nt == nq): info, pairs and rec against the restatement."""
    cur, kfs = C.records_case()
    win = pkg.mapping.SlidingWindow(ctx, 3, 400)
    _fill(win, kfs)
    rec, info, pairs = _check_records(win, cur, kfs)
    assert info[:, 3].tolist() == [1, 0, 1] and 0 < info[0, 4] < info[0, 2]
    # the same call again, and a window that has popped its oldest keyframe
    _check_records(win, cur, kfs)
    win.push(*kfs[1])
    _check_records(win, cur, kfs[1:] + [kfs[1]])
    win.close()


@pytest.mark.parametrize("W", [0, 1, 3])
def test_window_push_pop(pkg, ctx, W):
    """emplace_back / pop_front over 2 W + 1 pushes; lislam_mapwin_keyframe returns what was pushed;
    capacity and argument errors leave the window unchanged."""
    rng = np.random.default_rng(7 + W)
    win = pkg.mapping.SlidingWindow(ctx, W, 64)
    pushed = []

    def same():
        assert len(win) == min(len(pushed), W)
        for i, (d, p, x) in enumerate(pushed[len(pushed) - len(win):]):
            gd, gp, gx = win.keyframe(i)
            assert np.array_equal(gd, d) and np.array_equal(gp, p) and np.array_equal(gx, x), i

    for k in range(2 * W + 1):
        n = int(rng.integers(0, 65))
        kf = (C.random_desc(rng, n), _points(n, k), rng.normal(size=7))
        win.push(*kf)
        pushed.append(kf)
        same()
        with pytest.raises(pkg.native.LislamError, match="status -3"):  # LISLAM_ERR_CAPACITY
            win.push(C.random_desc(rng, 65), _points(65), IDENT)
        with pytest.raises(pkg.native.LislamError, match="status -3"):
            win.records(C.random_desc(rng, 65), _points(65), IDENT)
        with pytest.raises(pkg.native.LislamError, match="status -1"):  # LISLAM_ERR_ARG
            win.keyframe(len(win))
        same()
    win.close()
    for bad in ((-1, 64), (17, 64), (3, 0), (3, 4097)):
        with pytest.raises(pkg.native.LislamError, match="status -1"):
            pkg.mapping.SlidingWindow(ctx, *bad)


def test_step_drive(pkg, oracle, ctx, synth):
    """A 6-frame drive with W = 3 against the restated step, frame by frame: pose, state, summary,
    map size and every window keyframe's stored pose.  Frame DRIVE_BAD_FRAME's odometry is so far off
    that the solve does not converge: that keyframe keeps its initial guess."""
    frames = C.drive_case(synth)
    go = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, sliding_window_size=C.DRIVE_WINDOW, feature_capacity=1024)
    ro = R.MapOptimization(oracle, C.DRIVE_WINDOW)
    worst = 0.0
    for k, (g, od, f) in enumerate(frames):
        x0 = R.compose(go.state, od)  # the device's own initial guess (:112)
        pg, sg = go.callback(g, od, features=f)
        pr, sr = ro.callback(g, od, None, f)
        dp, ds = np.max(np.abs(pg - pr)), np.max(np.abs(go.state - ro.state))
        worst = max(worst, dp, ds)
        print(f"frame {k}: summary {list(sg)} |pose - restated| {dp:.3e} |state - restated| {ds:.3e}")
        assert dp < POSE_TOL and ds < POSE_TOL, (k, pg, pr)
        assert list(sg) == list(sr), (k, sg, sr)
        assert go.map.size() == ro.map.size(), k
        assert len(go.window) == len(ro.window), k
        for i, kf in enumerate(ro.window):
            d, p, x = go.window.keyframe(i)
            assert np.array_equal(d, kf.desc) and np.array_equal(p, kf.p3d), (k, i)
            assert np.max(np.abs(x - kf.pose)) < POSE_TOL, (k, i)
        if k == C.DRIVE_BAD_FRAME:
            assert sg[2] == 0
            x = go.window.keyframe(len(go.window) - 1)[2]
            assert np.max(np.abs(x - x0)) < 1e-12 and np.max(np.abs(x - pg)) > 1e-3  # the initial guess, not the solve's end
    print(f"largest difference over the drive {worst:.3e}")
    go.close()


def _drive_inputs(oracle, synth, n=4):
    out = []
    for k in range(n):
        scan = synth.make_scan(20 + k)
        flat = scan.reshape(-1, 4)
        ground = _f32(flat[np.abs(flat[:, :3]).sum(1) > 0])
        corner = oracle.scan_registration(scan).less_sharp
        q, t = synth.ground_truth_pose(20 + k).as_qt()
        out.append((ground, corner, synth.perturb_pose(q, t, 0.02, 0.2, seed=40 + k)))
    return out


@pytest.mark.parametrize("mode", ["null", "size0"])
def test_no_window_is_step_corner(pkg, oracle, ctx, synth, mode):
    """win = NULL and window_size = 0: outputs byte-equal to lislam_mapopt_step_corner on the same
    inputs (features given and ignored)."""
    import ctypes

    nat = pkg.native
    a = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, corner=True)
    b = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, corner=True)
    win = pkg.mapping.SlidingWindow(ctx, 0, 512) if mode == "size0" else None
    rng = np.random.default_rng(5)
    for k, (ground, corner, odom) in enumerate(_drive_inputs(oracle, synth)):
        pa, sa = a.callback(ground, odom, corner)
        d, p = C.random_desc(rng, 300), _points(300, k)
        pb, sb = np.zeros(7), np.full(5, 99, np.int32)
        nat.check(ctx.lib.lislam_mapopt_step_window(b.map.h, b.corner_map.h, win.h if win else None, nat.ptr(ground),
                                                    ground.shape[0], nat.ptr(corner), corner.shape[0], nat.ptr(d), nat.ptr(p),
                                                    300, nat.ptr(odom), nat.ptr(b.state), nat.ptr(pb), nat.ptr(sb)),
                  ctx.h, "lislam_mapopt_step_window")
        assert pa.tobytes() == pb.tobytes() and a.state.tobytes() == b.state.tobytes(), k
        assert list(sb) == list(sa) + [0, 0], k
        assert a.map.points().tobytes() == b.map.points().tobytes(), k
        assert a.corner_map.points().tobytes() == b.corner_map.points().tobytes(), k
        if win:
            assert len(win) == 0
    # MapOptimization's defaults take the windowless path
    assert pkg.mapping.MapOptimization(ctx).window is None
    a.close()
    b.close()
    if win:
        win.close()


def test_orb_detect_map(pkg, oracle, ctx, synth):
    """mapOptimization's three-axis zero filter: with points planted under keypoints that have
    |x| < 0.01 but |y| or |z| >= 0.01 (kept) or all three below (dropped), keypoints and descriptors
    equal oracle.orb_detect on a copy of the track whose x is 1 wherever the three-axis test keeps the
    point, the points gathered from the original track; lislam_orb_detect is unchanged."""
    f = oracle.scan_registration(synth.make_scan(23))
    img, track = f.img_intensity, np.array(f.cloud_track, np.float32).reshape(-1, 4)
    mask = oracle.hand_held_mask()
    kp0, _, _ = oracle.orb_detect(img, track, 1000, mask)
    pix = np.rint(kp0[:, 1]).astype(int) * 1024 + np.rint(kp0[:, 0]).astype(int)
    track[pix[0::7], 0] = 0.001          # x alone near zero: mapOptimization keeps these
    track[pix[1::7], :3] = (0.001, 0.02, 0.0)
    track[pix[2::7], :3] = (-0.002, 0.0, -5.0)
    track[pix[3::7], :3] = (0.009, -0.009, 0.009)  # all three near zero: dropped by both
    keep = R.keeps_point(track)
    rkp, rde, _ = oracle.orb_detect(img, C.map_filter_track(track, keep), 1000, mask)
    kp, de, p3 = pkg.intensity.orb_detect(ctx, img, track, 1000, mask, map_filter=True)
    assert kp.shape == rkp.shape and np.array_equal(kp, rkp) and np.array_equal(de, rde)
    rpix = np.rint(rkp[:, 1]).astype(int) * 1024 + np.rint(rkp[:, 0]).astype(int)
    assert np.array_equal(p3[:, :3], track[rpix, :3]) and np.all(p3[:, 3] == 0)
    assert np.all(keep[rpix]) and (np.abs(p3[:, 0]) < 0.01).sum() >= 100
    # the feature tracker's entry point on the same input: unchanged, and fewer keypoints
    tkp, tde, tp3 = pkg.intensity.orb_detect(ctx, img, track, 1000, mask)
    okp, ode, op3 = oracle.orb_detect(img, track, 1000, mask)
    assert np.array_equal(tkp, okp) and np.array_equal(tde, ode) and np.array_equal(tp3[:, :3], op3)
    assert len(tkp) < len(kp)


def test_batch_path(pkg, oracle, ctx, synth):
    """callback_batch over 4 synthetic 64 x 1024 scans with W = 2 (features detected on the device)
    equals callback fed the features orb_detect(map_filter=True) returns for those scans, and the
    restated step.  The scans (make_sequence(4, start=40)) give feature blocks in frames 2 and 3."""
    S, NF = 4, 2000
    nat = pkg.native
    scans = synth.make_sequence(S, start=40)
    b = pkg.Batch(ctx, S)
    b.upload(scans)
    b.extract(S)
    b.ground(S)
    gb = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, corner=True, sliding_window_size=2, feature_capacity=4096)
    gc = pkg.mapping.MapOptimization(ctx, 0.4, 0.2, corner=True, sliding_window_size=2, feature_capacity=4096)
    ro = R.MapOptimization(oracle, 2)
    blocks = 0
    for k in range(S):
        f = oracle.scan_registration(scans[k])
        g_ref, _, _ = oracle.ground_extract(scans[k])
        merged = np.concatenate([g_ref, f.less_flat]).astype(np.float32)
        q, t = synth.ground_truth_pose(40 + k).as_qt()
        odom = synth.perturb_pose(q, t, 0.02, 0.2, seed=60 + k)
        # callback's inputs are the batch's own clouds and images (downloaded), the restated step's the oracle's
        bf = b.features(k)
        bmerged = np.concatenate([b.ground_result(k)[0], bf.less_flat]).astype(np.float32)
        bimg = b.download(nat.OUT_IMAGE_INTENSITY, k).reshape(64, 1024)
        btrack = b.download(nat.OUT_CLOUD_TRACK, k)
        _, de, p3 = pkg.intensity.orb_detect(ctx, bimg, btrack, NF, None, map_filter=True)
        keep = R.keeps_point(f.cloud_track)
        rkp, rde, _ = oracle.orb_detect(f.img_intensity, C.map_filter_track(f.cloud_track, keep), NF, None)
        rp3 = np.zeros((len(rkp), 4), np.float32)
        rp3[:, :3] = f.cloud_track.reshape(-1, 4)[np.rint(rkp[:, 1]).astype(int) * 1024 + np.rint(rkp[:, 0]).astype(int), :3]
        assert np.array_equal(de, rde) and np.array_equal(p3, rp3), k
        pb, sb = gb.callback_batch(b, k, odom, nfeatures=NF)
        pc, sc = gc.callback(bmerged, odom, bf.less_sharp, features=(de, p3))
        pr, sr = ro.callback(merged, odom, f.less_sharp, (rde, rp3))
        assert pb.tobytes() == pc.tobytes() and gb.state.tobytes() == gc.state.tobytes(), k
        assert list(sb) == list(sc) == list(sr), (k, sb, sc, sr)
        assert np.max(np.abs(pb - pr)) < POSE_TOL and np.max(np.abs(gb.state - ro.state)) < POSE_TOL, k
        assert gb.map.size() == gc.map.size() == ro.map.size(), k
        assert gb.corner_map.size() == gc.corner_map.size() == ro.corner_map.size(), k
        for i in range(len(gb.window)):
            db, p_b, xb = gb.window.keyframe(i)
            dc, p_c, xc = gc.window.keyframe(i)
            assert np.array_equal(db, dc) and np.array_equal(p_b, p_c) and xb.tobytes() == xc.tobytes(), (k, i)
        blocks += sb[3]
    assert blocks > 0
    gb.close()
    gc.close()
    b.close()
