"""The keyframe selector restated literally: feature_tracker::getKeyframe
(src/intensity_feature_tracker.cpp:741-815, called at :721 on good frames only, :693) behind
tfBroadcast's T_s2m_ = T_s2m_ * T_s2s_ (:819), with p2p_calculateRandT's tail (:916-925) turning the
(q, t) row into the 4x4 matrix.

Plain Python floats and explicit sums in the order written here, so that no BLAS and no FMA enters:
every operation is one IEEE double operation, and lislam_keysel.hip performs the same ones in the same
order.  The first branch of getKeyframe (cloudKeyPoses3D_->points.empty(), :749, a container another
thread fills at :536) is taken exactly once: by the first good frame of the selector's life."""
import math

import numpy as np

NODE = 26  # time, id, cur_position_[3], prev_position_[3], cur_rotation_[9], prev_rotation_[9] (keyframe.h:115-121)


def rotation(x, y, z, w):
    """Eigen's QuaternionBase::toRotationMatrix, the quaternion as it is (not normalised)."""
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def matrix(row):
    """[R(q) t; 0 0 0 1] of a row q x,y,z,w, t (:916-925)."""
    x, y, z, w, t0, t1, t2 = (float(v) for v in row)
    R = rotation(x, y, z, w)
    return [R[0] + [t0], R[1] + [t1], R[2] + [t2], [0.0, 0.0, 0.0, 1.0]]


def product(A, B):
    """C(i,j) = ((A(i,0) B(0,j) + A(i,1) B(1,j)) + A(i,2) B(2,j)) + A(i,3) B(3,j), all 16 entries."""
    return [[((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j] for j in range(4)]
            for i in range(4)]


class Selector:
    """State as the constructor leaves it (:31-37).  ``gaps`` records, for every good frame after the first
    keyframe, (time - last_time, |p - prev_p|): what the two gates compared, for the tests' margin checks."""

    def __init__(self, time_interval=0.3, distance_interval=0.3):
        self.time_interval, self.distance_interval = float(time_interval), float(distance_interval)
        self.T = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
        self.prev_p = [0.0, 0.0, 0.0]
        self.prev_R = [[0.0] * 3 for _ in range(3)]
        self.next_id = 0
        self.have = False
        self.last_time = None
        self.gaps = []

    def step(self, T_s2s, good, times):
        """-> (keyframe_id (n,) int32, T_s2m (n, 4, 4), nodes (n_selected, 26))."""
        T_s2s = np.asarray(T_s2s, np.float64).reshape(-1, 7)
        ids, Ts, nodes = [], [], []
        for k in range(T_s2s.shape[0]):
            self.T = product(self.T, matrix(T_s2s[k]))  # :819, every frame
            Ts.append([list(r) for r in self.T])
            if int(good[k]) != 1:  # getKeyframe is called on good frames only
                ids.append(-1)
                continue
            t = float(times[k])
            p = [self.T[0][3], self.T[1][3], self.T[2][3]]           # :743
            R = [[self.T[i][j] for j in range(3)] for i in range(3)]  # :744
            if not self.have:  # :749
                select = True
            else:
                dx, dy, dz = p[0] - self.prev_p[0], p[1] - self.prev_p[1], p[2] - self.prev_p[2]
                distance = math.sqrt((dx * dx + dy * dy) + dz * dz)
                self.gaps.append((t - self.last_time, distance))
                select = t - self.last_time > self.time_interval and distance > self.distance_interval  # :774-777
            if not select:
                ids.append(-1)
                continue
            nodes.append([t, float(self.next_id)] + p + list(self.prev_p) + [v for r in R for v in r] +
                         [v for r in self.prev_R for v in r])
            ids.append(self.next_id)
            self.last_time, self.prev_p, self.prev_R = t, p, R
            self.next_id += 1
            self.have = True
        return (np.array(ids, np.int32).reshape(-1), np.array(Ts, np.float64).reshape(-1, 4, 4),
                np.array(nodes, np.float64).reshape(-1, NODE))

    def margins(self):
        """The smallest |time gap - time_interval| and |distance - distance_interval| met so far (inf: none)."""
        mt = min((abs(g[0] - self.time_interval) for g in self.gaps), default=math.inf)
        md = min((abs(g[1] - self.distance_interval) for g in self.gaps), default=math.inf)
        return mt, md
