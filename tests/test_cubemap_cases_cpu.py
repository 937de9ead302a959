"""CPU pin of the cube-map edge cases (tests/cubemap_cases.py): on every case the oracle
(oracle_lmap_step) and the independent Python bookkeeping (tests/restate_cubemap.py) agree on the
local-map sizes, the points per cube and every point, and the case produces what it was built for —
the shift, drop, merge, gate and overflow facts below are asserted on the oracle's run, so a case cannot
go hollow unnoticed.  No GPU."""
import numpy as np
import pytest

import cubemap_cases as CC
from restate_cubemap import DIMS, H, PyCubeMap, W, _cube, _qrot


def run_case(oracle, case):
    """Oracle and PyCubeMap side by side (the pose is the oracle's); per frame a record of the
    oracle's outputs and PyCubeMap's facts."""
    om = oracle.LaserMap(case.line_res, case.plane_res)
    pm = PyCubeMap(oracle, case.line_res, case.plane_res)
    log = []
    for k, (c, s, od) in enumerate(case.frames):
        state0 = om.state.copy()
        x, stats = om.step(c, s, od)
        # the centre cube follows t_w_curr = q_wmap_wodom t_wodom + t_wmap_wodom before the optimization
        t_curr = _qrot(state0[:4], od[4:].astype(np.float64)) + state0[4:]
        stacks = [oracle.voxel_grid(c.reshape(-1, 4), case.line_res), oracle.voxel_grid(s.reshape(-1, 4), case.plane_res)]
        local = pm.frame(stacks, x, t_curr)
        assert (stats[0], stats[1]) == (local[0].shape[0], local[1].shape[0]), k  # local maps before insertion
        assert (stats[2], stats[3]) == (stacks[0].shape[0], stacks[1].shape[0]), k
        counts = om.counts()
        for w in (0, 1):
            py = np.array([a.shape[0] for a in pm.arr[w]])
            assert np.array_equal(counts[w], py), (k, w)
            assert np.array_equal(om.points(w), np.concatenate(pm.arr[w])), (k, w)
        world = [np.array([(_qrot(x[:4], p[:3].astype(np.float64)) + x[4:]).astype(np.float32) for p in st]).reshape(-1, 3)
                 for st in stacks]
        log.append(dict(stats=stats.copy(), pose=x.copy(), t_curr=t_curr, facts=pm.facts(), cen=tuple(pm.cen),
                        counts=[c_.copy() for c_ in counts], world=world, state=om.state.copy()))
    return log, pm


def check_opt(case, log):
    for k, (want, rec) in enumerate(zip(case.opt, log)):
        o = rec["stats"][4:]
        if want == "none":
            assert np.all(o == -1), (k, o)
        elif want == "zero":
            assert np.all(o == 0), (k, o)
        else:
            assert o[0] + o[1] > 0 and o[2] + o[3] > 0 and np.all(o >= 0), (k, o)


def _bookkeeping(oracle, name):
    case = CC.BOOKKEEPING[name]
    log, pm = run_case(oracle, case)
    check_opt(case, log)
    for k, rec in enumerate(log):  # the optimization never ran: the pose is the odometry
        assert rec["stats"][0] <= 10 or rec["stats"][1] <= 50, k
        assert np.array_equal(rec["pose"][4:], rec["t_curr"]), k
    return case, log, pm


def at(i, j, k):
    return i + W * j + W * H * k


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("sign", (1, -1))
def test_axes(oracle, axis, sign):
    """Re-centring on each axis in each direction by 1, 2 and 3 cubes, alone and with another axis: the
    shifts are the intended ones, each shift keeps part of the pool and drops part, and each frame near
    the edge drops part of the new points and keeps part."""
    case, log, pm = _bookkeeping(oracle, f"axes{'+' if sign > 0 else '-'}{'xyz'[axis]}")
    assert [r["facts"]["shift"] for r in log] == case.expect["shifts"]
    other = (axis + 1) % 3
    assert log[5]["facts"]["shift"][axis] == -sign and log[5]["facts"]["shift"][other] == sign
    cen = [10, 10, 5]
    cen[axis] -= sign * 7
    cen[other] += sign
    assert log[-1]["cen"] == tuple(cen)
    for k in range(1, 6):
        f = log[k]["facts"]
        for w in (0, 1):
            assert 0 < f["dropped"][w] < f["stack"][w], (k, w)
            assert f["nonvalid"][w] > 0, (k, w)
            if k >= 2:
                assert 0 < f["kept"][w] <= f["pool_before"][w], (k, w)
    for w in (0, 1):  # and the far side of the array left it on the way
        assert sum(log[k]["facts"]["pool_before"][w] - log[k]["facts"]["kept"][w] for k in range(2, 6)) > 0, w


def test_far_jump(oracle):
    """A jump of more than the array on every axis: the shift empties both pools (kept == 0 of a
    non-empty pool), the frame after it meets an empty map and fills it, and the jump back does the same."""
    case, log, pm = _bookkeeping(oracle, "far_jump")
    for k, s in ((1, -1), (3, 1)):
        f = log[k]["facts"]
        assert all(abs(f["shift"][a]) > DIMS[a] and np.sign(f["shift"][a]) == s * (1, -1, 1)[a] for a in range(3))
        assert min(f["pool_before"]) > 0 and f["kept"] == [0, 0] and f["local"] == [0, 0]
        assert all(0 < f["stack"][w] - f["dropped"][w] == log[k]["counts"][w].sum() for w in (0, 1))
    f = log[2]["facts"]
    assert f["shift"] == (0, 0, 0) and min(f["local"]) > 0
    assert log[3]["cen"] != (10, 10, 5)


@pytest.mark.parametrize("rich", (0, 1))
@pytest.mark.parametrize("rotated", (False, True))
def test_merge(oracle, rotated, rich):
    """Old centroids and new points average into one voxel, new points do among themselves, points go
    into valid cubes around a cen that never moved, and one voxel of the grid holds a centroid on either
    side of a cube face (the cubes are voxelized apart)."""
    case, log, pm = _bookkeeping(oracle, f"merge_{'rot' if rotated else 'id'}_{'surf' if rich else 'corner'}")
    for k, rec in enumerate(log):
        f = rec["facts"]
        assert f["dropped"] == [0, 0] and f["nonvalid"] == [0, 0], k
        assert (f["old_new"][rich] > 0) == (k > 0), k
        assert len(f["touched"][rich]) >= 12, k  # 2 + 4 + 2 + 8 + 2 + 1 cubes at the least when each cluster straddles
    # the stack is voxelized in the sensor frame: two of its centroids share a voxel of the map only where the grids differ
    assert sum(rec["facts"]["new_new"][rich] for rec in log) > 0
    leaf = (case.line_res, case.plane_res)[rich]
    a, b = pm.arr[rich][at(10, 10, 5)], pm.arr[rich][at(11, 10, 5)]  # either side of the face x = 25
    va = {tuple(v) for v in np.floor(a[:, :3] / np.float32(leaf)).astype(int)}
    vb = {tuple(v) for v in np.floor(b[:, :3] / np.float32(leaf)).astype(int)}
    assert va & vb


def test_boundary(oracle):
    """World coordinates exactly on a cube boundary and one ulp either side, before and after a shift,
    and sensors with t + 25 exactly -50.0 and 0.0: truncate-then-decrement puts -75 and -25 one cube below
    floor()."""
    case, log, pm = _bookkeeping(oracle, "boundary")
    assert log[1]["cen"] == log[2]["cen"] == case.expect["cen_after_shift"] and log[0]["cen"] == (10, 10, 5)
    assert log[2]["facts"]["shift"] == (0, 0, 0)
    assert _cube(-75.0, 10) == 8 == int(np.floor((-75.0 + 25.0) / 50.0)) + 10 - 1 and _cube(25.0, 10) == 11
    for k in (0, 2, 3, 4):
        for w in (0, 1):
            world, hits = log[k]["world"][w], case.expect["hits"][k][w]
            assert len(hits) == world.shape[0]
            for a, v in hits:  # every point is a voxel of its own: the stack holds it unchanged
                assert np.any(world[:, a] == np.float32(v)), (k, w, a, v)
            values = {(a, v) for a, v in hits}
            for a in (0, 1, 2) if w == 0 else (2,):
                for b in CC.BOUNDS:
                    assert (a, b) in values, (k, w, a, b)
                    if k in (0, 2):  # identity pose: both neighbours are expressible
                        assert (a, float(np.nextafter(np.float32(b), np.float32(np.inf)))) in values
                        assert (a, float(np.nextafter(np.float32(b), np.float32(-np.inf)))) in values
    # at cen (10, 10, 5) x == -75 goes to cube 8 with its lower neighbour (floor() puts it in 9 with the upper one)
    f = log[0]["facts"]
    hits, world = case.expect["hits"][0][0], log[0]["world"][0]
    cubes = {}
    for a, v in hits:
        (p,) = world[world[:, a] == np.float32(v)]
        cubes[(a, v)] = tuple(_cube(float(p[e]), 10 if e < 2 else 5) for e in range(3))
    lo = float(np.nextafter(np.float32(-75.0), np.float32(-np.inf)))
    hi = float(np.nextafter(np.float32(-75.0), np.float32(np.inf)))
    assert (cubes[(0, lo)][0], cubes[(0, -75.0)][0], cubes[(0, hi)][0]) == (8, 8, 9)
    assert all(at(*c) in f["touched"][0] for c in cubes.values())
    assert f["nonvalid"][0] > 0 and f["nonvalid"][1] > 0  # z = -75 and z = 75 lie outside the valid block
    # the centre cube of a sensor at t + 25 == -50.0 (one below floor) and == 0.0
    cen = log[2]["cen"]
    assert log[3]["facts"]["centre"][0] == _cube(-75.0, cen[0]) == cen[0] - 2
    assert log[3]["facts"]["centre"][1] == _cube(-25.0, cen[1]) == cen[1]
    assert log[4]["facts"]["centre"][0] == log[4]["cen"][0]


def test_nonvalid(oracle):
    """Points into cubes of the array outside the valid block pass un-voxelized: those cubes grow by
    their full input every frame, pairs within one voxel included, while the valid cubes stay as the first
    frame left them."""
    case, log, pm = _bookkeeping(oracle, "nonvalid")
    for w in (0, 1):
        first = log[0]["counts"][w]
        f = log[0]["facts"]
        valid = np.zeros(first.shape[0], bool)
        c = f["centre"]
        for i in range(c[0] - 2, c[0] + 3):
            for j in range(c[1] - 2, c[1] + 3):
                for k in range(c[2] - 1, c[2] + 2):
                    valid[at(i, j, k)] = True
        assert f["nonvalid"][w] >= 60 and f["dropped"][w] == 0 and first[valid].sum() > 0
        assert first[~valid].sum() == f["nonvalid"][w]
        assert first[~valid].max() >= 2
        for k in (1, 2):
            assert log[k]["facts"]["old_new"][w] > 0
            assert np.array_equal(log[k]["counts"][w][~valid], (k + 1) * first[~valid])
            assert np.array_equal(log[k]["counts"][w][valid], first[valid])
    # a pair 1 cm apart survived in a non-valid corner cube (the 0.4 m VoxelGrid would have merged it)
    pts = pm.arr[0]
    assert any(a.shape[0] >= 6 and np.min(np.linalg.norm(a[1:, :3] - a[0, :3], axis=1)) < 0.05 for a in pts)


def test_empties(oracle):
    """nc == 0, ns == 0, both, the first frame, an empty frame over a filled map, and a frame whose
    points all fall outside the array."""
    case, log, pm = _bookkeeping(oracle, "empties")
    sizes = [tuple(int(x.shape[0] > 0) for x in fr[:2]) for fr in case.frames]
    assert sizes[:5] == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 0)]
    assert log[0]["counts"][0].sum() == log[0]["counts"][1].sum() == 0
    k = case.expect["empty_after_points"]
    assert min(log[k]["stats"][:2]) > 0 and tuple(log[k]["stats"][2:4]) == (0, 0)
    for w in (0, 1):
        assert np.array_equal(log[k]["counts"][w], log[k - 1]["counts"][w])
    k = case.expect["all_dropped"]
    f = log[k]["facts"]
    assert f["dropped"] == f["stack"] and min(f["stack"]) > 0
    for w in (0, 1):
        assert np.array_equal(log[k]["counts"][w], log[k - 1]["counts"][w])
    assert log[6]["counts"][0].sum() > log[5]["counts"][0].sum()


@pytest.mark.parametrize("nc", (10, 11))
@pytest.mark.parametrize("ns", (50, 51))
def test_gate(oracle, nc, ns):
    """The optimization runs only past 10 corner and 50 surf map points; on lattices too sparse for
    any association it finds none and leaves the pose alone."""
    case = CC.BOOKKEEPING[f"gate_{nc}_{ns}"]
    log, pm = run_case(oracle, case)
    check_opt(case, log)
    assert tuple(log[1]["stats"][:4]) == (nc, ns, nc, ns)
    assert np.array_equal(log[1]["pose"], case.frames[1][2])
    assert np.all(log[1]["stats"][4:] == (0 if nc == 11 and ns == 51 else -1))


def test_tiny_leaf(oracle):
    """A leaf so small that one cube's index space passes 2^31: that cube keeps every point it is
    given, its neighbour under the limit is voxelized as usual."""
    case, log, pm = _bookkeeping(oracle, "tiny_leaf")
    wide, near = at(*case.expect["wide_cube"]), at(*case.expect["near_cube"])
    n = case.expect["n_wide"]
    for k, rec in enumerate(log):
        assert rec["facts"]["overflow"][0] == 1, k
        assert rec["counts"][0][wide] == (k + 1) * n, k
        assert rec["counts"][0][near] == log[0]["counts"][0][near], k
    assert 0 < log[0]["counts"][0][near] < case.frames[0][0].shape[0] - n  # pairs merged on the first frame
    assert log[0]["facts"]["new_new"][0] > 0 and log[1]["facts"]["old_new"][0] > 0


@pytest.fixture(scope="module")
def back(oracle, synth):
    case = CC.there_and_back(oracle, synth)
    return (case,) + run_case(oracle, case)


def test_there_and_back(back):
    """The optimization over a pool that went through the shift, and insertion into translated cubes:
    the out-bound frames meet an empty local map, the second frame out there and every frame that comes
    back optimize with associations, at a cen that is not the initial one.  One leg of (-340, 380, 130)
    shifts y and z but not x (_cube(-340, 10) is 3, the last cube that stays), so the first two return
    frames run at cen (10, 9, 4); cubes translated on x as well are met by the last return frame only,
    after the second leg, at cen (17, 3, 3)."""
    case, log, pm = back
    check_opt(case, log)
    for k in case.expect["outbound"]:
        f = log[k]["facts"]
        assert f["shift"] != (0, 0, 0) and f["local"] == [0, 0] and min(f["kept"]) > 0, k
    assert log[3]["facts"]["shift"] == (0, 0, 0) and np.all(log[3]["stats"][4:] > 0)
    for k in case.expect["returns"]:
        f = log[k]["facts"]
        assert log[k]["cen"] != (10, 10, 5) and np.all(log[k]["stats"][4:] > 0), k
        assert f["old_new"][0] > 0 and f["old_new"][1] > 0, k  # new points merged into cubes that were translated
        assert min(f["kept"]) > 0
    assert all(log[7]["cen"][a] != (10, 10, 5)[a] for a in range(3))
