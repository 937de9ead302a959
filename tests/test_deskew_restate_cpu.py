"""The CPU restatement of the odometry's distortion modes (tests/cpp/deskew_restate.cpp through
tests/restate_deskew.py) is what test_gpu_deskew.py holds the GPU against, so it is pinned here first,
without a GPU:

a. mode 0 reproduces the oracle (oracle_odom.cpp, the same headers and 1-NN tie rule) exactly: para,
   pose and stats with max |delta| = 0, plain and gated, on the default chain and the living node;
b. mode 2 under the identity para (a chain's first frame) leaves xyz bit-identical and intensity int();
c. the frames the GPU tests use hold queries with s > 1 and with s < 0 (the negative-relTime quirk);
d. modes 1 and 2 change the result on the default chain, and mode 2 changes it against mode 1."""
import numpy as np
import pytest

import deskew_cases as D
import odom_cases as C
import restate_deskew as R


@pytest.fixture(scope="module")
def default_chain(oracle, synth):
    return D.chain_features(oracle, synth, "default")


@pytest.fixture(scope="module")
def living(oracle, synth):
    return D.living_frames(oracle, synth)


def assert_same_as_oracle(ref, got):
    pose, rel, st = ref
    assert np.max(np.abs(got.para - rel)) == 0.0
    assert np.max(np.abs(got.pose - pose)) == 0.0
    assert np.array_equal(got.stats, st)


@pytest.mark.parametrize("gated", (False, True))
def test_mode0_is_the_oracle_on_the_default_chain(oracle, default_chain, gated):
    gate = C.USE_ALOAM if gated else None
    ref = oracle.odometry_chain(default_chain, gate)
    assert np.any(ref[2][:, :2] > 0)  # the chain has solved pairs
    assert_same_as_oracle(ref, R.odometry_chain(default_chain, R.OFF, gate))


@pytest.mark.parametrize("gated", (False, True))
def test_mode0_is_the_oracle_on_the_living_node(oracle, synth, living, gated):
    gate = (1, 0, 1, 1, 1) if gated else None
    for frames in (C.living_node_frames(oracle, synth), living):
        assert_same_as_oracle(oracle.odometry_chain(frames, gate), R.odometry_chain(frames, R.OFF, gate))


def test_mode0_chains_of_a_batch(oracle, default_chain):
    """batch_chains (chain_len 3: chains over scans 0-3, 3-6, 6-8) against one oracle node per chain."""
    got = R.batch_chains(default_chain, R.OFF, 3)
    for c0, c1 in ((0, 3), (3, 6), (6, 8)):
        pose, rel, st = oracle.odometry_chain(default_chain[c0: c1 + 1])
        lo = 0 if c0 == 0 else 1
        assert np.array_equal(got.para[c0 + lo: c1 + 1], rel[lo:])
        assert np.array_equal(got.pose[c0 + lo: c1 + 1], pose[lo:])
        assert np.array_equal(got.stats[c0 + lo: c1 + 1], st[lo:])


def test_to_end_under_the_identity_keeps_xyz(default_chain, living):
    for frames in (default_chain, living):
        r = R.odometry_chain(frames[:1], R.TO_END)
        assert np.array_equal(r.para[0], [0, 0, 0, 1, 0, 0, 0])
        for got, src in ((r.corner_last[0], frames[0].less_sharp), (r.surf_last[0], frames[0].less_flat),
                         (r.full_end[0], frames[0].laser_cloud)):
            assert got.shape == src.shape and got.shape[0] > 0
            assert np.array_equal(got[:, :3].view(np.uint32), np.ascontiguousarray(src[:, :3]).view(np.uint32))
            assert np.array_equal(got[:, 3], np.trunc(src[:, 3]))
            assert np.any(got[:, 3] != src[:, 3])  # the inputs do carry a relative time


def test_to_end_moves_a_solved_frame(default_chain):
    r = R.odometry_chain(default_chain[:2], R.TO_END)
    assert r.stats[1][0] > 0 and r.stats[1][1] > 0
    assert not np.array_equal(r.surf_last[1][:, :3], default_chain[1].less_flat[:, :3])
    assert np.array_equal(r.surf_last[1][:, 3], np.trunc(default_chain[1].less_flat[:, 3]))


def queries_s(frames):
    return np.concatenate([R.rel_s(np.concatenate([f.sharp, f.flat])) for f in frames if f.sharp.shape[0] + f.flat.shape[0]])


def test_fixtures_cover_the_quirk_branches(oracle, synth, default_chain, living):
    # the batch path extracts its features on the device, so its scans go unedited: s > 1 is there
    for variant in C.CHAIN_VARIANTS:
        s = queries_s(D.chain_features(oracle, synth, variant))
        assert np.any(s > 1.0) and np.all(np.isfinite(s)), variant
    # the node path takes edited frames: both signs, and the line-below case (s near 10)
    s = queries_s(living)
    assert np.any(s > 1.0) and np.any(s < 0.0) and np.any(s > 9.0)
    # ... and they reach residual blocks: the quirky frames are solved with about as many correspondences
    plain = R.odometry_chain(C.living_node_frames(oracle, synth), R.QUERIES)
    quirk = R.odometry_chain(living, R.QUERIES)
    for k in (1, 4):
        assert quirk.stats[k][0] > 0 and quirk.stats[k][1] > 0
        assert not np.array_equal(quirk.para[k], plain.para[k])
    s = queries_s([f for pair in D.node_pairs(oracle, synth).values() for f in pair])
    assert np.any(s > 1.0)


def test_modes_differ_on_the_default_chain(default_chain):
    r0 = R.odometry_chain(default_chain, R.OFF)
    r1 = R.odometry_chain(default_chain, R.QUERIES)
    r2 = R.odometry_chain(default_chain, R.TO_END)
    assert not np.array_equal(r1.para[1], r0.para[1])  # the first solved pair already
    assert np.array_equal(r2.para[1], r1.para[1])      # pair 1's targets are a first frame: the same xyz
    assert not np.array_equal(r2.para[2], r1.para[2])  # pair 2 searches de-skewed targets
    assert np.max(np.abs(r1.para - r0.para)) > 1e-4 and np.max(np.abs(r2.para - r1.para)) > 1e-4


def test_the_public_interface_names_the_modes(pkg):
    nat = pkg.native
    assert (nat.DISTORTION_OFF, nat.DISTORTION_QUERIES, nat.DISTORTION_TO_END) == (R.OFF, R.QUERIES, R.TO_END)
    assert (nat.OUT_CORNER_LAST, nat.OUT_SURF_LAST, nat.OUT_FULL_RES_END) == (22, 23, 24)
    assert "lislam_set_distortion" in nat.EXPORTED_SYMBOLS
    assert nat.KERNELS[-2:] == ("k_odom_to_end", "k_target_index_round")
