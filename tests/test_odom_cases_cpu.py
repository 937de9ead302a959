"""The degenerate-odometry cases (tests/odom_cases.py) are sound, checked on the CPU oracle alone: the
GPU test (test_gpu_odom_degenerate.py) compares the kernels with the oracle on these inputs, so the
inputs must neither make that comparison vacuous nor fail it for the oracle's own reasons.

Stability cap: every x, y, z of the current frame moved by one float ulp (np.nextafter towards +inf,
then towards -inf) may move the oracle's para by at most CAP = 1e-5 (a tenth of the GPU test's
POSE_TOL) and may not change a correspondence count.  A case beyond the cap would be listed in
UNSTABLE with its measured value and lose the GPU pose comparison (at most MAX_UNSTABLE cases).
Measured: none; the largest move is 9.8e-7 (queries_16), 8.9e-7 for the large targets and 1.3e-7 for
the chains (where every frame of the stream is nudged, and the world poses are held to the cap too)."""
import numpy as np
import pytest

import odom_cases as C

CAP = 1e-5
MAX_UNSTABLE = 2
UNSTABLE = {}  # case name -> measured move of para; the GPU test skips the pose comparison for these


@pytest.fixture(scope="module")
def node(oracle, synth):
    return C.node_cases(oracle, synth)


@pytest.fixture(scope="module")
def large(oracle, synth):
    return C.large_target_cases(oracle, synth)


def pair_result(oracle, pair):
    pose, rel, st = oracle.odometry_chain(list(pair))
    return pose, rel, st


def assert_finite_unit(pose, rel, st):
    assert np.all(np.isfinite(pose)) and np.all(np.isfinite(rel)) and np.all(np.isfinite(st))
    for q in (pose[:, :4], rel[:, :4]):
        assert np.max(np.abs(np.linalg.norm(q, axis=1) - 1.0)) <= 1e-12


def is_identity(x):
    return np.array_equal(x, [0, 0, 0, 1, 0, 0, 0])


def test_case_lists_are_complete(node, large):
    assert [n for n in node if n.startswith("targets_")] == [f"targets_{k}" for k in C.TARGETS_K]
    assert [n for n in node if n.startswith("queries_")] == [f"queries_{k}" for k in C.QUERIES_K]
    assert set(C.ZERO_NODE_CASES) <= set(node)
    assert {f"large_{n}" for n in C.LARGE_POOLED + C.LARGE_SINGLE} == set(large)
    for n in C.LARGE_POOLED + C.LARGE_SINGLE:
        assert large[f"large_{n}"][0].less_flat.shape == (n, 4)
    assert min(C.LARGE_POOLED) < C.SORT_BOUNDARY < max(C.LARGE_POOLED)
    # every cloud of every case is ordered by scan line and within the 16- / 64-line capacities
    for cases, H in ((node, 16), (large, 64)):
        for name, pair in cases.items():
            for f in pair:
                for cl, cap in zip(C.CLOUDS, (12 * H, 120 * H, 24 * H, H * (256 if H == 16 else 1024))):
                    line = C.line_of(getattr(f, cl))
                    assert np.all(np.diff(line) >= 0), (name, cl)
                    assert line.shape[0] <= cap, (name, cl)


def test_sub_keeps_order_and_the_original(node, oracle, synth):
    f0, _ = C.base_pair(oracle, synth)
    n = f0.less_flat.shape[0]
    g = C.sub(f0, less_flat=17, sharp=np.array([3, 1]))
    assert np.array_equal(g.less_flat, f0.less_flat[np.linspace(0, n - 1, 17).astype(int)])
    assert np.array_equal(g.sharp, f0.sharp[[3, 1]]) and g.flat is f0.flat
    assert f0.less_flat.shape[0] == n and C.sub(f0, flat=0).flat.shape == (0, 4)
    assert np.array_equal(C.sub(f0, flat=1).flat, f0.flat[:1])


@pytest.mark.parametrize("name", C.ZERO_NODE_CASES)
def test_zero_node_cases(oracle, node, name):
    """No correspondence in either pass, the identity para of a fresh node, 0 / 0 iterations."""
    pose, rel, st = pair_result(oracle, node[name])
    assert_finite_unit(pose, rel, st)
    assert not st.any(), st
    assert is_identity(rel[1]) and is_identity(pose[1])


def test_nonzero_cases_are_nonzero_and_stable(oracle, node, large):
    """Every other case has corner and plane correspondences in pass 1, finite unit outputs, and
    stays within the stability cap (or is listed in UNSTABLE)."""
    worst = {}
    for cases in (node, large):
        for name, (fl, fc) in cases.items():
            if name in C.ZERO_NODE_CASES:
                continue
            pose, rel, st = pair_result(oracle, (fl, fc))
            assert_finite_unit(pose, rel, st)
            assert st[1][0] > 0 and st[1][1] > 0, (name, st[1])
            move = 0.0
            for towards in (np.inf, -np.inf):
                _, rel2, st2 = pair_result(oracle, (fl, C.nudged(fc, towards)))
                move = max(move, float(np.max(np.abs(rel2[1] - rel[1]))))
                if not np.array_equal(st2[1][:4], st[1][:4]):
                    move = np.inf  # a count changed: as unstable as it gets
            worst[name] = move
    over = {n: m for n, m in worst.items() if m > CAP}
    print(f"stability: largest move of para {max(worst.values()):.3g} ({max(worst, key=worst.get)}); "
          f"cases demoted by the stability cap: {len(UNSTABLE)}")
    assert set(over) <= set(UNSTABLE), over
    assert len(UNSTABLE) <= MAX_UNSTABLE


@pytest.mark.parametrize("k", [k for k in C.QUERIES_K if k])
def test_queries_k_find_exactly_k(oracle, node, k):
    """Every one of the k sharp and k flat queries finds its correspondence in both passes (measured
    on these scans; a change of the synthetic data that breaks it should be noticed here)."""
    _, _, st = pair_result(oracle, node[f"queries_{k}"])
    assert list(st[1][:4]) == [k, k, k, k], st[1]


def test_living_node_frames(oracle, synth):
    """Pair 2 (no targets) carries pair 1's para; the pairs around it are solved."""
    frames = C.living_node_frames(oracle, synth)
    pose, rel, st = oracle.odometry_chain(frames)
    assert_finite_unit(pose, rel, st)
    assert not st[2].any() and np.array_equal(rel[2], rel[1]) and not np.array_equal(pose[2], pose[1])
    assert list(st[3][:4]) == [1, 1, 1, 1]
    for k in (1, 4):
        assert st[k][0] > 0 and st[k][1] > 0, (k, st[k])
    for towards in (np.inf, -np.inf):
        pose2, rel2, st2 = oracle.odometry_chain([C.nudged(f, towards) for f in frames])
        assert np.array_equal(st2[:, :4], st[:, :4])
        assert max(np.max(np.abs(rel2 - rel)), np.max(np.abs(pose2 - pose))) <= CAP


@pytest.mark.parametrize("variant", C.CHAIN_VARIANTS)
def test_chain_cases(oracle, synth, variant):
    """The altered scans lose what they should in extraction; blank pairs carry para with zero
    correspondences and iterations while the pose goes on accumulating; the other pairs are solved."""
    scans = C.chain_scans(synth, variant)
    feats = [oracle.scan_registration(s) for s in scans]
    counts = [[getattr(f, c).shape[0] for c in C.CLOUDS] for f in feats]
    blank_scans = [k for k in range(9) if counts[k] == [0, 0, 0, 0]]
    assert blank_scans == sorted({3, 7} | ({0} if variant == "blank_first" else set())
                                 | ({8} if variant == "blank_last" else set()))
    assert 0 < counts[5][2] < 32 and 0 < counts[5][0] < counts[4][0]  # the thin scan
    pose, rel, st = oracle.odometry_chain(feats)
    assert_finite_unit(pose, rel, st)
    blank = C.chain_blank_pairs(variant)
    for k in range(1, 9):
        if k in blank:
            assert not st[k].any(), (k, st[k])
            assert np.array_equal(rel[k], rel[k - 1]), k  # carried
            if not is_identity(rel[k]):
                assert not np.array_equal(pose[k], pose[k - 1]), k  # ... and accumulated
        else:
            assert st[k][0] > 0 and st[k][1] > 0, (k, st[k])
    if variant == "default":
        assert blank == [3, 4, 7, 8]
        assert list(st[5][:2]) == [97, 15] and list(st[6][:2]) == [85, 236]
    for towards in (np.inf, -np.inf):
        pose2, rel2, st2 = oracle.odometry_chain([C.nudged(f, towards) for f in feats])
        assert np.array_equal(st2[:, :4], st[:, :4])
        assert max(np.max(np.abs(rel2 - rel)), np.max(np.abs(pose2 - pose))) <= CAP
    # the gated run and the three-pair chains of the GPU test see the same blank pairs
    _, relg, stg = oracle.odometry_chain(feats, use_aloam=np.array(C.USE_ALOAM, np.int32))
    assert np.all(np.isfinite(relg)) and not stg[4].any()
