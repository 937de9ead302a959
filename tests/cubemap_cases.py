"""Edge cases of laserMapping's cube map (lislam_lmap_*, oracle_lmap_*): fixed-seed numpy generators for
tests/test_cubemap_cases_cpu.py (oracle against tests/restate_cubemap.py, and the coverage each case
is built for); a GPU test of the library takes the same cases and `opt` patterns.

A case is a list of frames (corner_last, surf_last, odom7), the two leaf sizes, the expected
optimization pattern per frame (`opt`: "none" = stats[4:] all -1, "zero" = all 0, "some" = both
passes found associations) and `expect`, the facts the CPU test asserts.  The cube geometry the
inputs are placed by: cube c of an axis covers [-25 + 50 (c - cen), 25 + 50 (c - cen)), cen starts at
(10, 10, 5), the centre cube is kept within [3, dim - 3) by re-centring, the valid block is the centre
cube +-2, +-2, +-1.

All cases but `there_and_back` keep the corner local map <= 10 points or the surf local map <= 50, so
the optimization never runs and the pose is host arithmetic alone.  No GPU, no file is read."""
from dataclasses import dataclass, field

import numpy as np

ID = (0.0, 0.0, 0.0, 1.0)
EMPTY = np.zeros((0, 4), np.float32)
BOUNDS = (-75.0, -25.0, 25.0, 75.0)


@dataclass
class Case:
    name: str
    frames: list
    opt: list
    line_res: float = 0.4
    plane_res: float = 0.8
    expect: dict = field(default_factory=dict)


def _odom(t, q=ID):
    return np.array([*q, *t], np.float64)


def _xyzi(rng, xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.concatenate([xyz, rng.uniform(0, 1, (xyz.shape[0], 1))], 1).astype(np.float32)


def _box(rng, n, half, centre=(0, 0, 0)):
    return np.asarray(centre, np.float64) + rng.uniform(-1, 1, (n, 3)) * np.asarray(half, np.float64)


def _shell(rng, n, lo, hi):
    """Uniform in [-hi, hi]^3 outside [-lo, lo]^3."""
    out = []
    while len(out) < n:
        p = rng.uniform(-hi, hi, 3)
        if np.max(np.abs(p)) >= lo:
            out.append(p)
    return np.array(out)


def _rot(q, v):
    """q * v (rows of v), double."""
    q = np.asarray(q, np.float64)
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


# ------------------------------------------------------------------------------------------ a. axes
def axes(axis: int, sign: int) -> Case:
    """One direction: the sensor runs to the last cube before a shift, then crosses 1, 2 and 3 cubes
    in one frame each, then 1 more together with 1 cube of another axis the other way.  The clouds
    reach +-300 m around the sensor, past the array edge, which is then 175 m away at the most."""
    rng = np.random.default_rng(100 + 2 * axis + (sign > 0))
    first = (340.0, 340.0, 90.0)[axis]
    other = (axis + 1) % 3
    frames, shifts = [], []
    for k, along in enumerate((0.0, first, first + 50, first + 150, first + 300, first + 350)):
        t = np.zeros(3)
        t[axis] = sign * along
        sh = [0, 0, 0]
        sh[axis] = -sign * (0, 0, 1, 2, 3, 1)[k]
        if k == 5:
            t[other] = -sign * (390.0, 390.0, 140.0)[other]
            sh[other] = sign
        frames.append((_xyzi(rng, _shell(rng, 40, 170.0, 300.0)), _xyzi(rng, _box(rng, 300, 300.0)), _odom(t)))
        shifts.append(tuple(sh))
    return Case(f"axes{'+' if sign > 0 else '-'}{'xyz'[axis]}", frames, ["none"] * 6, expect=dict(shifts=shifts))


# -------------------------------------------------------------------------------------- b. far_jump
def far_jump() -> Case:
    rng = np.random.default_rng(200)
    far = (3000.0, -3000.0, 900.0)
    frames = [(_xyzi(rng, _box(rng, 8, 100.0)), _xyzi(rng, _box(rng, 200, 100.0)), _odom(t))
              for t in ((0, 0, 0), far, far, (0, 0, 0))]
    return Case("far_jump", frames, ["none"] * 4)


# ----------------------------------------------------------------------------------------- c. merge
MERGE_SITES = ((25.0, 0.0, 0.0), (24.9, -25.0, 1.0), (0.0, 0.0, 25.0), (-25.0, -25.0, -25.0), (75.0, 75.0, 25.0),
               (10.0, 7.0, -3.0))
MERGE_Q = tuple(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]))


def merge(rotated: bool, rich: int) -> Case:
    """Clusters 1 m wide on cube faces, an edge and a corner, seen again from four poses less than a
    metre apart.  `rich` is the cloud (0 corner, 1 surf) that sees every cluster with 60 points; the
    other sees a few points of one cluster, which keeps the optimization off."""
    rng = np.random.default_rng(300 + 2 * rotated + rich)
    q = MERGE_Q if rotated else ID
    qc = (-q[0], -q[1], -q[2], q[3])
    frames = []
    for k in range(4):
        t = k * np.array([0.31, -0.23, 0.17])
        clouds = [None, None]
        clouds[rich] = np.concatenate([_box(rng, 60, 0.5, s) for s in MERGE_SITES])
        clouds[1 - rich] = _box(rng, 2 if rich else 10, 0.5, MERGE_SITES[3])
        frames.append(tuple(_xyzi(rng, _rot(qc, w - t)) for w in clouds) + (_odom(t, q),))
    return Case(f"merge_{'rot' if rotated else 'id'}_{'surf' if rich else 'corner'}", frames, ["none"] * 4,
                expect=dict(rich=rich))


# -------------------------------------------------------------------------------------- d. boundary
def _ulps(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def _boundary_points(t, axes_, shift=0.0):
    """Sensor-frame points (identity rotation, translation t) whose world coordinate on one axis is a
    cube boundary or one float ulp beside it, where float32 can express that; the other two
    coordinates lie near the origin, every point in a voxel of its own.  Returns the points and
    the (axis, world value) pairs."""
    pts, hits = [], []
    for a in axes_:
        for bi, b in enumerate(BOUNDS):
            for k in (-1, 0, 1):
                target = _ulps(b, k)
                p = np.float32(np.float64(target) - t[a])
                if np.float32(np.float64(p) + t[a]) != target:
                    continue
                w = np.zeros(3)  # world, near the origin
                w[(a + 1) % 3] = 2.0 + 3.0 * bi + k + shift
                w[(a + 2) % 3] = -7.0 - 3.0 * a + shift
                s = (w - t).astype(np.float32)
                s[a] = p
                pts.append(s)
                hits.append((a, float(target)))
    return np.array(pts, np.float32).reshape(-1, 3), hits


def boundary() -> Case:
    rng = np.random.default_rng(400)
    frames, hits = [], []
    poses = ((0.0, 0.0, 0.0), (390.0, -390.0, 140.0), (0.0, 0.0, 0.0), (-75.0, -25.0, -75.0), (-25.0, -75.0, -25.0))
    for k, t in enumerate(poses):
        t = np.array(t)
        if k == 1:  # the shift: cen becomes (9, 11, 4)
            frames.append((_xyzi(rng, _box(rng, 3, 5.0)), _xyzi(rng, _box(rng, 3, 5.0)), _odom(t)))
            hits.append(([], []))
            continue
        c, hc = _boundary_points(t, (0, 1, 2), 0.25 * k)
        s, hs = _boundary_points(t, (2,), 0.25 * k)
        frames.append((_xyzi(rng, c), _xyzi(rng, s), _odom(t)))
        hits.append((hc, hs))
    return Case("boundary", frames, ["none"] * 5, expect=dict(hits=hits, cen_after_shift=(9, 11, 4)))


# -------------------------------------------------------------------------------------- e. nonvalid
def nonvalid() -> Case:
    """The same cloud three times from the origin: points 3..8 cubes away on x / y or 2..4 on z, some
    of them pairs within one voxel, and a few points around the sensor."""
    rng = np.random.default_rng(500)

    def far(n):
        out = []
        while len(out) < n:
            o = np.array([rng.integers(-8, 9), rng.integers(-8, 9), rng.integers(-4, 5)])
            if abs(o[0]) >= 3 or abs(o[1]) >= 3 or abs(o[2]) >= 2:
                out.append(50.0 * o + rng.uniform(-24.0, 24.0, 3))
        out = np.array(out)
        return np.concatenate([out, out[:10] + 0.01])  # pairs 1 cm apart

    corner = _xyzi(rng, np.concatenate([far(60), _box(rng, 8, (20.0, 20.0, 20.0))]))
    surf = _xyzi(rng, np.concatenate([far(60), _box(rng, 40, (60.0, 60.0, 20.0))]))
    return Case("nonvalid", [(corner, surf, _odom((0, 0, 0)))] * 3, ["none"] * 3)


# --------------------------------------------------------------------------------------- f. empties
def empties() -> Case:
    rng = np.random.default_rng(600)
    c = lambda: _xyzi(rng, _box(rng, 100, 60.0))  # noqa: E731
    s = lambda: _xyzi(rng, _box(rng, 15, 60.0))  # noqa: E731
    beyond = lambda n: _xyzi(rng, _box(rng, n, (50.0, 100.0, 100.0), (650.0, 0.0, 0.0)))  # noqa: E731
    o = _odom((0, 0, 0))
    frames = [(EMPTY, EMPTY, o), (EMPTY, s(), o), (c(), EMPTY, o), (c(), s(), o), (EMPTY, EMPTY, o),
              (beyond(30), beyond(30), o), (c(), s(), _odom((1.0, -1.0, 0.5)))]
    return Case("empties", frames, ["none"] * 7, expect=dict(all_dropped=5, empty_after_points=4))


# ------------------------------------------------------------------------------------------ g. gate
def gate(nc: int, ns: int) -> Case:
    """Lattices 5 m apart, every point a voxel of its own and no five points within a metre: one frame
    builds the map, the second meets local maps of exactly nc corner and ns surf points."""
    rng = np.random.default_rng(700)
    g = np.array([(5.0 * i - 17.5, 5.0 * j - 15.0, 0.0) for j in range(7) for i in range(8)])
    corner = _xyzi(rng, g[:nc] + (2.5, 2.5, 3.0))
    surf = _xyzi(rng, g[:ns])
    both = nc > 10 and ns > 50
    return Case(f"gate_{nc}_{ns}", [(corner, surf, _odom((0, 0, 0)))] * 2, ["none", "zero" if both else "none"],
                expect=dict(local=(nc, ns)))


# -------------------------------------------------------------------------------- h. there_and_back
PLAN = ((0, 0), (1, 0), (2, 1), (3, 1), (1, 0), (2, 0), (3, 2), (0, 0))
LEG = np.array([-340.0, 380.0, 130.0])


def there_and_back(oracle, synth) -> Case:
    """The only case that optimizes: four synthetic 32 x 512 scans (the oracle's features and
    odometry) visited in PLAN order, frame (f, k) displaced by k legs.  The out-bound frames meet an
    empty local map; the frames that come back optimize against cubes that were translated."""
    scans = synth.make_sequence(4, 32, 512, start=3)
    feats = [oracle.scan_registration(s) for s in scans]
    _, pose, _ = oracle.odometry_chain(feats)
    frames = []
    for f, k in PLAN:
        od = pose[f].copy()
        od[4:] += k * LEG
        frames.append((feats[f].less_sharp, feats[f].less_flat, od))
    return Case("there_and_back", frames, ["none", "some", "none", "some", "some", "some", "none", "some"],
                expect=dict(returns=(4, 5, 7), outbound=(2, 6)))


# ------------------------------------------------------------------------------------- i. tiny_leaf
def tiny_leaf() -> Case:
    """line_res 0.01: the corner points of the centre cube span 48 m (4800^3 voxels, past 2^31: the
    cube's VoxelGrid returns its input), those of its +x neighbour 4 m (400^3).  The same cloud three
    times."""
    rng = np.random.default_rng(900)
    wide = _box(rng, 100, 24.0)
    near = _box(rng, 90, 2.0, (50.0, 0.0, 0.0))
    near = np.concatenate([near, near[:10] + 0.001])  # ten pairs within one 1 cm voxel
    corner = _xyzi(rng, np.concatenate([wide, near]))
    surf = _xyzi(rng, _box(rng, 10, 20.0))
    return Case("tiny_leaf", [(corner, surf, _odom((0, 0, 0)))] * 3, ["none"] * 3, line_res=0.01,
                expect=dict(wide_cube=(10, 10, 5), near_cube=(11, 10, 5), n_wide=100))


def bookkeeping_cases():
    out = [axes(a, s) for a in range(3) for s in (1, -1)]
    out.append(far_jump())
    out += [merge(r, w) for r in (False, True) for w in (0, 1)]
    out += [boundary(), nonvalid(), empties()]
    out += [gate(nc, ns) for nc in (10, 11) for ns in (50, 51)]
    out.append(tiny_leaf())
    return out


BOOKKEEPING = {c.name: c for c in bookkeeping_cases()}
