"""The cases of loop_verify_cases.py on the CPU oracle alone: they must cover the ground the GPU test
(test_gpu_loop_verify.py) is meant to cover -- every outcome code, every convergence state that
the corridor reaches, candidates that leave the iteration loop at different times, clipped submap
windows, both VoxelGrid paths in one call -- so that the GPU test cannot pass vacuously.

T_kf has one row per keyframe, so a current keyframe that lies inside its own submap (cur <= loop +
window) is there under its drifted pose too: (9, 8) and (11, 10) then converge in 2 iterations (with
the history at undrifted poses, which no single T_kf can express, the oracle takes 6)."""
import numpy as np

import loop_verify_cases as C


def _info(oracle, synth, name):
    cfg = next(c for c in C.all_configs(synth) if c[0] == name)
    rows = C.cached_oracle_rows(oracle, synth, name)
    return cfg, {cand: (None if r is None else [int(v) for v in r[3]]) for cand, r in zip(cfg[3], rows)}, rows


def test_submap_ids_restates_the_reference():
    assert C.submap_ids(11, 0) == [0, 1]            # clipped at 0
    assert C.submap_ids(11, 10) == [9, 10, 11]
    assert C.submap_ids(10, 10) == [9, 10]          # clipped at cur
    assert C.submap_ids(10, 3, 0) == [3]
    assert C.submap_ids(10, 3, 2) == [1, 2, 3, 4, 5]
    assert C.submap_ids(9, 1, 2) == [0, 1, 2, 3]


def test_package_submap_ids_agrees(pkg):
    for cur in range(12):
        for loop in range(cur + 1):
            for w in range(5):
                assert pkg.keyframes.submap_ids(cur, loop, w) == C.submap_ids(cur, loop, w)


def test_pool_is_what_the_cases_say(synth):
    cl = C.pool_clouds(synth)
    assert len(cl) == C.POOL_SIZE and all(c.shape == (4096, 4) for c in cl[:12])
    assert cl[C.EMPTY].shape == (0, 4) and cl[C.TINY].shape == (8, 4)
    assert np.isnan(cl[C.NAN_X][:, 0]).all() and np.isfinite(cl[C.NAN_X][:, 1:]).all()
    cube = cl[C.CUBE]
    assert np.array_equal(cube[0::2], cube[1::2]) and np.ptp(cube[:, :3], axis=0).max() < 1.0


def test_default_candidates(oracle, synth):
    cfg, info, _ = _info(oracle, synth, "default")
    assert all(c in cfg[3] for c in C.DEFAULT_CANDIDATES)
    for cand in C.DEFAULT_CANDIDATES:
        assert info[cand][0] == 1 and info[cand][1] == 1 and info[cand][2] == 2  # accepted, transform
    # candidates leave the loop at different times (and in different 6-iteration chunks)
    assert [info[c][3] for c in C.DEFAULT_CANDIDATES] == [24, 31, 2, 2]
    assert len(C.submap_ids(11, 0)) == 2 and C.submap_ids(11, 10)[-1] == 11
    assert sum(1 for c in cfg[3] if c[1] < 0) == 2 and cfg[3].count((10, 3)) == 2  # -3 rows, a repeated candidate
    assert len({c[0] for c in cfg[3] if c[1] >= 0}) < len([c for c in cfg[3] if c[1] >= 0])  # a keyframe in several


def test_config_cases(oracle, synth):
    _, info, _ = _info(oracle, synth, "max_iterations")
    assert all(i[1] == 1 and i[2] == 1 and i[3] == 3 for i in info.values())      # state 1: iterations
    _, info, _ = _info(oracle, synth, "max_distance")
    assert info[(11, 0)][:3] == [0, 0, 5] and info[(11, 0)][6] < 3                 # state 5, not converged
    _, info, rows = _info(oracle, synth, "fitness")
    assert all(i[0] == 0 and i[1] == 1 for i in info.values()) and all(r[2] > 1e-4 for r in rows)
    _, info, _ = _info(oracle, synth, "no_downsample")
    assert info[(10, 3)][3:6] == [48, 4096, 12288] and info[(9, 8)][4:6] == [4096, 12288]
    _, info, _ = _info(oracle, synth, "crop")
    _, full, _ = _info(oracle, synth, "default")
    assert all(0 < info[c][4] < full[c][4] and info[c][0] == 1 for c in info)      # the crop box removes points


def test_window_cases(oracle, synth):
    cfg0, info0, _ = _info(oracle, synth, "window0")
    cfg2, info2, _ = _info(oracle, synth, "window2")
    assert cfg0[2] == 0 and all(len(C.submap_ids(*c, 0)) == 1 for c in cfg0[3])
    assert cfg2[2] == 2 and len(C.submap_ids(10, 3, 2)) == 5
    assert len(C.submap_ids(11, 10, 2)) == 4 and len(C.submap_ids(9, 1, 2)) == 4   # clipped at cur, at 0
    _, info1, _ = _info(oracle, synth, "default")
    assert info0[(10, 3)][5] < info1[(10, 3)][5] < info2[(10, 3)][5]               # the target grows with the window
    assert all(i[1] == 1 for i in list(info0.values()) + list(info2.values()))


def test_degenerate_cases(oracle, synth):
    cfg, info, _ = _info(oracle, synth, "degenerate")
    assert cfg[2] == 0
    assert info[(C.ROOM, C.EMPTY)] == [-1, 0, 0, 0, 0, 0, 0, 0]                    # empty submap
    assert info[(C.ROOM, C.NAN_X)][0] == -2 and info[(C.ROOM, C.NAN_X)][4] > 10 and info[(C.ROOM, C.NAN_X)][5] == 0
    assert info[(C.TINY, 3)][0] == -2 and 0 < info[(C.TINY, 3)][4] <= 8 and info[(C.TINY, 3)][5] > 10
    assert info[(C.NAN_X, 3)][0] == -2 and info[(C.NAN_X, 3)][4] == 0
    assert info[(11, 0)][1] == 1 and info[(C.ROOM, C.ROOM)][0] == 1               # healthy ones in between
    assert info[(C.CUBE, -1)] is None


def test_mixed_overflow_case(oracle, synth):
    cfg, info, _ = _info(oracle, synth, "mixed_overflow")
    v = cfg[1]["voxel_size"]
    cl = C.pool_clouds(synth)
    assert not C.voxel_overflows(cl[C.CUBE], v) and C.voxel_overflows(cl[8], v)
    assert info[(C.CUBE, C.CUBE)][4] == cl[C.CUBE].shape[0] // 2 == info[(C.CUBE, C.CUBE)][5]  # VoxelGrid ran
    assert info[(8, 8)][4] == cl[8].shape[0] == info[(8, 8)][5]                                # it passed unchanged
    assert info[(8, 7)][4] == cl[8].shape[0] and info[(8, 7)][5] == cl[7].shape[0] and info[(8, 7)][3] > 1
    assert all(i[1] == 1 for i in info.values())
