"""Independent Python transcription of the bookkeeping of laserMapping's 21 x 21 x 11 cube map
(laserMapping.cpp:319-1002): re-centring shifts (pointer rotation, wrapped cubes cleared), the
valid-cube loop order of the local map, insertion at the optimized pose (Eigen q * v + t in double,
stored as float) and the per-cube VoxelGrid of the valid cubes.  The VoxelGrid itself is the
oracle's (oracle.voxel_grid); the optimization is not restated (the caller passes the pose).
Checker only, no GPU.

tests/test_oracle_cubemap.py still carries the class this one grew from (fixed leaves, a _shift that
cannot take a map of empty cubes) for its two ordinary sequences; it is to import this one."""
import numpy as np

W, H, D = 21, 21, 11
DIMS = (W, H, D)


def _qrot(q, v):
    u = np.array([q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]])
    u = u + u
    c = np.array([q[1] * u[2] - q[2] * u[1], q[2] * u[0] - q[0] * u[2], q[0] * u[1] - q[1] * u[0]])
    return (v + q[3] * u) + c


def _cube(v, cen):
    c = int((v + 25.0) / 50.0) + cen
    return c - 1 if v + 25.0 < 0 else c


def _empty():
    return np.zeros((0, 4), np.float32)


def _voxel_keys(pts, leaf):
    """pcl::VoxelGrid's voxel index of every point of one cloud, or None where the index space
    exceeds 32 bits (the filter then returns its input).  Used for the merge and overflow facts only:
    the points come from oracle.voxel_grid, and the two are never compared point for point, so a
    drift between them would show as a fact assertion failing, not as a point mismatch."""
    inv = np.float32(1.0) / np.float32(leaf)
    xyz = pts[:, :3].astype(np.float32)
    mn, mx = xyz.min(0), xyz.max(0)
    d = [int(np.float32(np.float32(mx[k] - mn[k]) * inv)) + 1 for k in range(3)]
    if d[0] * d[1] * d[2] > 2**31 - 1:
        return None
    min_b = np.floor(mn * inv).astype(np.int64)
    div_b = np.floor(mx * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(xyz * inv) - min_b.astype(np.float32)).astype(np.int64)
    return ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]


class PyCubeMap:
    def __init__(self, oracle, line_res=0.4, plane_res=0.8):
        self.O = oracle
        self.res = (line_res, plane_res)
        self.cen = [10, 10, 5]
        self.arr = [[_empty() for _ in range(W * H * D)] for _ in range(2)]
        self._facts = None

    def at(self, i, j, k):
        return i + W * j + W * H * k

    def frame(self, stacks, x, t_curr):
        """stacks: voxelized corner / surf (sensor frame); x: the optimized pose; t_curr: the
        pose's translation before the optimization (decides the centre cube)."""
        cc = [_cube(t_curr[a], self.cen[a]) for a in range(3)]
        shift = [0, 0, 0]
        for a in range(3):
            while cc[a] < 3:
                cc[a] += 1
                shift[a] += 1
            while cc[a] >= DIMS[a] - 3:
                cc[a] -= 1
                shift[a] -= 1
        before = [sum(c.shape[0] for c in self.arr[w]) for w in (0, 1)]
        for a in range(3):
            if shift[a]:
                self._shift(a, shift[a])
                self.cen[a] += shift[a]
        kept = [sum(c.shape[0] for c in self.arr[w]) for w in (0, 1)]
        valid = [self.at(i, j, k) for i in range(cc[0] - 2, cc[0] + 3) for j in range(cc[1] - 2, cc[1] + 3)
                 for k in range(cc[2] - 1, cc[2] + 2) if 0 <= i < W and 0 <= j < H and 0 <= k < D]
        vset = set(valid)
        local = [np.concatenate([self.arr[w][v] for v in valid]) if valid else _empty() for w in (0, 1)]
        facts = dict(shift=tuple(shift), centre=tuple(cc), pool_before=before, kept=kept, local=[a.shape[0] for a in local],
                     stack=[len(s) for s in stacks], dropped=[0, 0], nonvalid=[0, 0], old_new=[0, 0], new_new=[0, 0],
                     overflow=[0, 0], touched=[set(), set()])
        n_old = [{v: self.arr[w][v].shape[0] for v in valid} for w in (0, 1)]
        for w in (0, 1):
            for p in stacks[w]:
                pw = (_qrot(x[:4], p[:3].astype(np.float64)) + x[4:]).astype(np.float32)
                ci = [_cube(float(pw[a]), self.cen[a]) for a in range(3)]
                if all(0 <= ci[a] < DIMS[a] for a in range(3)):
                    c = self.at(*ci)
                    self.arr[w][c] = np.concatenate([self.arr[w][c], np.array([[pw[0], pw[1], pw[2], p[3]]], np.float32)])
                    facts["touched"][w].add(c)
                    if c not in vset:
                        facts["nonvalid"][w] += 1
                else:
                    facts["dropped"][w] += 1
        for v in valid:
            for w in (0, 1):
                self._merges(facts, w, self.arr[w][v], n_old[w][v])
                self.arr[w][v] = self.O.voxel_grid(self.arr[w][v], self.res[w])
        self._facts = facts
        return local

    def facts(self):
        """Of the last frame, per cloud (corner, surf) where a pair: `dropped` new points outside the
        array, `nonvalid` new points into cubes outside the valid block, `shift` per axis, `kept` pool
        points after the shift (`pool_before` before it), `old_new` / `new_new` voxels of the valid cubes
        whose centroid averages old and new points / new points only, `overflow` valid cubes whose
        points span more than 2^31 voxels, `touched` the cubes that received points, `local` / `stack`
        sizes, `centre` the centre cube."""
        return self._facts

    def _merges(self, facts, w, pts, n_old):
        if pts.shape[0] == 0:
            return
        keys = _voxel_keys(pts, self.res[w])
        if keys is None:
            facts["overflow"][w] += 1
            return
        is_old = np.arange(pts.shape[0]) < n_old
        for k in np.unique(keys):
            m = keys == k
            if m.sum() < 2:
                continue
            no = int(is_old[m].sum())
            if no and no < m.sum():
                facts["old_new"][w] += 1
            elif no == 0:
                facts["new_new"][w] += 1

    def _shift(self, a, s):
        """Cube index along axis a grows by s (s < 0: shrinks); what leaves the array is dropped."""
        for w in (0, 1):
            if abs(s) >= DIMS[a]:
                self.arr[w] = [_empty() for _ in range(W * H * D)]
                continue
            g = np.empty(W * H * D, dtype=object)
            for i, c in enumerate(self.arr[w]):
                g[i] = c
            g = g.reshape(D, H, W)  # [k][j][i]
            ax = 2 - a
            g = np.roll(g, s, axis=ax)
            idx = [slice(None)] * 3
            idx[ax] = slice(0, s) if s > 0 else slice(s, None)  # the wrapped-around slabs are cleared
            cleared = g[tuple(idx)]
            for e in np.ndindex(cleared.shape):
                cleared[e] = _empty()
            self.arr[w] = list(g.reshape(-1))
