"""The CPU restatement of mapOptimization's ORB keyframe sliding window (tests/restate_mapwin.py)
against the oracle and against independent statements of its pieces, and the properties of the
constructed cases (tests/mapwin_cases.py) that the GPU tests rely on.  No GPU."""
import numpy as np
import pytest

import mapwin_cases as C
import restate_mapwin as R


def test_empty_window_is_the_oracle_step(oracle, synth):
    """With sliding_window_size 0 (and with a window that has nothing to offer) the restated step is
    oracle.mapopt_step_corner bit for bit over the 5-frame drive of test_mapopt_corner_map."""
    mo = R.MapOptimization(oracle, 0)
    mo3 = R.MapOptimization(oracle, 3)  # features never given: empty keyframes, M = 0
    om, ocm = oracle.IkdMap(0.4), oracle.IkdMap(0.8)
    ostate = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    for k in range(5):
        scan = synth.make_scan(20 + k)
        flat = scan.reshape(-1, 4)
        ground = np.ascontiguousarray(flat[np.abs(flat[:, :3]).sum(1) > 0], np.float32)
        corner = oracle.scan_registration(scan).less_sharp
        q, t = synth.ground_truth_pose(20 + k).as_qt()
        odom = synth.perturb_pose(q, t, 0.02, 0.2, seed=40 + k)
        po, ostate, so = oracle.mapopt_step_corner(om, ocm, ground, corner, odom, ostate)
        for m in (mo, mo3):
            p, s = m.callback(ground, odom, corner)
            assert np.array_equal(p, po), k
            assert np.array_equal(m.state, ostate), k
            assert list(s[:3]) == list(so) and list(s[3:]) == [0, 0], (k, s, so)
            assert m.map.size() == om.size() and m.corner_map.size() == ocm.size(), k
            assert np.array_equal(m.corner_map.points(), ocm.points()), k
    assert len(mo.window) == 0 and len(mo3.window) == 3


@pytest.mark.parametrize("nts", C.MATCH_WINDOWS)
def test_l2_argmin(nts):
    """The literal argmin loop, the numpy form the other tests use and an independent np.argmin over
    sqrt(float32) distances (cv::BFMatcher's DMatch::distance) agree."""
    for nq in C.MATCH_NQ:
        q, trains = C.match_case(nq, nts)
        for t in trains + C.extreme_case()[1]:
            idx, s = R.l2_match(q, t)
            fidx, fs = R.l2_match_fast(q, t)
            assert np.array_equal(idx, fidx) and np.array_equal(s, fs)
            if len(t):
                d = np.sqrt(((q[:, None, :].astype(np.float32) - t[None, :, :].astype(np.float32)) ** 2).sum(2).astype(np.float32))
                assert np.array_equal(np.argmin(d, axis=1), idx)
                assert np.array_equal(np.sqrt(s.astype(np.float32)), d[np.arange(nq), idx])
            else:
                assert len(idx) == 0
    q, (a, b) = C.extreme_case()
    assert list(R.l2_match(q, a)[1]) == [C.MAX_SUM, 0]
    assert list(R.l2_match(q, b)[0]) == [1, 0]


def test_good_count_is_the_literal_loop():
    """G for M = 0..4096: for (i = 0; i < M * 0.2; ++i) evaluated in double."""
    for M in range(4097):
        lim = np.float64(M) * np.float64(0.2)
        G = int(np.ceil(lim))
        assert R.good_count(M) == G, M
        assert (G == 0 or np.float64(G - 1) < lim) and not np.float64(G) < lim, M
    assert R.good_count(250) == 50 and R.good_count(251) == 51 and R.good_count(4096) == 820


def _window(kfs):
    return [R.Keyframe(*k) for k in kfs]


def test_condition_boundaries_are_hit():
    """Every condition of :309 / :327 is met from both sides by the selection cases, and equal sums
    straddle the G-th place wherever a keyframe is used."""
    seen = set()
    for nq, nt in C.SELECT_CASES:
        cur, kf = C.select_case(nq, nt)
        rec, info, pairs, _ = R.window_records(_window([kf]), *cur)
        nt_, M, G, used, kept, off = info[0]
        assert (nt_, M) == (nt, nq)
        seen.add((M > 100, G > 50, nt != nq, bool(used)))
        assert used == (M > 100 and G > 50 and G != M and nt != nq)
        idx, s = R.l2_match(cur[0], kf[0])
        assert np.all(idx == 0)
        srt = np.sort(s)
        assert srt[G - 1] == srt[G], (nq, nt)  # a run of equal sums straddles the G-th place
        if used:
            # the stable order keeps the lowest query indices of that run
            assert kept == G and list(pairs[:, 1]) == sorted(range(nq), key=lambda i: s[i])[:G]
    # M > 100 fails (100), holds with G <= 50 (101, 250), G > 50 holds (251), nt == nq (300, 300)
    assert (False, False, True, False) in seen and (True, False, True, False) in seen
    assert (True, True, True, True) in seen and (True, True, False, False) in seen
    info = {c: R.window_records(_window([C.select_case(*c)[1]]), *C.select_case(*c)[0])[1][0] for c in C.SELECT_CASES}
    assert info[(250, 300)][2] == 50 and not info[(250, 300)][3]
    assert info[(251, 300)][2] == 51 and info[(251, 300)][3]
    assert not info[(100, 150)][3] and not info[(300, 300)][3] and info[(299, 300)][3]


def test_records_case_properties():
    """Planted outliers fall on both sides of the gate, none within 1e-6 m of it, and the keyframe
    with nt == nq is skipped."""
    cur, win = C.records_case()
    rec, info, pairs, d = R.window_records(_window(win), *cur)
    d = np.array(d)
    assert np.min(np.abs(d - 0.3)) > 1e-6
    assert (d > 0.3).sum() >= 10 and ((d > 0.15) & (d < 0.3)).sum() >= 10 and (d < 0.05).sum() >= 50
    assert list(info[:, 3]) == [1, 0, 1] and info[1, 0] == info[1, 1]
    assert len(rec) == info[:, 4].sum() and 0 < info[0, 4] < info[0, 2]
    assert list(info[:, 5]) == [0, info[0, 4], info[0, 4]]


def test_drive_case_properties(oracle, synth):
    """The drive yields feature blocks in at least 3 frames, its far-off frame does not converge (so
    that keyframe keeps its initial guess), and no gate distance lies within 1e-6 m of 0.3."""
    frames = C.drive_case(synth)
    mo = R.MapOptimization(oracle, C.DRIVE_WINDOW)
    with_blocks = 0
    for k, (g, od, f) in enumerate(frames):
        x0 = R.compose(mo.state, od)
        if k > 0:
            d = np.array(R.window_records(list(mo.window), f[0], f[1], x0)[3])
            assert len(d) == 0 or np.min(np.abs(d - 0.3)) > 1e-6, k
        p, s = mo.callback(g, od, None, f)
        with_blocks += s[3] > 0
        if k == C.DRIVE_BAD_FRAME:
            assert s[2] == 0, s  # NO_CONVERGENCE
            assert np.array_equal(mo.window[-1].pose, x0) and not np.array_equal(p, x0)
        elif k > 0:
            assert s[2] == 1, (k, s)
            assert np.array_equal(mo.window[-1].pose, p)
    assert with_blocks >= 3
    assert len(mo.window) == C.DRIVE_WINDOW
