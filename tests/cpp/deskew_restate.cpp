// TEST INFRASTRUCTURE ONLY.  CPU restatement of the scan-to-scan odometry with the reference's
// DISTORTION switch (src/laserOdometry.cpp:82), built on the oracle's headers (cost functors with s,
// Jet autodiff, the Ceres 1.14 LM restatement) without touching oracle/:
//   mode 0  DISTORTION 0: s = 1 everywhere (what oracle_odom.cpp restates)
//   mode 1  DISTORTION 1 as the file compiles: s = (intensity - int(intensity)) / SCAN_PERIOD per
//           query point in TransformToStart (:147-172) and in each LidarEdgeFactor / LidarPlaneFactor
//           (:548-556, :671-679)
//   mode 2  mode 1 with the block :762-790 enabled: TransformToEnd (:176-194) over the less-sharp,
//           less-flat and full-resolution clouds after every frame, so the next pair's targets (and
//           /velodyne_cloud_3, /laser_cloud_corner_last, /laser_cloud_surf_last) are de-skewed
// The association is :446-689 with a brute-force 1-NN returning the lexicographically smallest
// (float squared distance, index) — the oracle's kd-tree tie rule — followed by the scan-line walks.
#include <cfloat>
#include <cstring>
#include <vector>

#include "oracle_common.hpp"
#include "oracle_jet.hpp"
#include "oracle_solver.hpp"

namespace {

using namespace oracle;

constexpr double SCAN_PERIOD = 0.1, DIST_SQ = 25.0, NEARBY = 2.5;

// :153 — float subtraction of int(intensity), then a double division.  relTime may be negative
// (scanRegistration), then int() truncates towards the line below and s is near 10, or slightly
// negative on line 0: reference behaviour, kept.
inline double rel_s(int mode, const P4& p) { return mode == 0 ? 1.0 : (double)(p.i - (float)int(p.i)) / SCAN_PERIOD; }

// TransformToStart (:147-172): double math, stored as float.
P4 to_start(int mode, const P4& pi, const double* para) {
  const double s = rel_s(mode, pi);
  const Q4<double> q0{para[0], para[1], para[2], para[3]};
  const Q4<double> qq = mode == 0 ? slerp_identity_s1(q0) : slerp_identity(s, q0);
  const V3<double> p{(double)pi.x, (double)pi.y, (double)pi.z};
  const V3<double> u = rotate(qq, p) + V3<double>{s * para[4], s * para[5], s * para[6]};
  return P4{(float)u.x, (float)u.y, (float)u.z, pi.i};
}

// TransformToEnd (:176-194): q.inverse() is Eigen's conjugate / squaredNorm (the 4-vector reduction
// in Packet2d order: (x^2 + z^2) + (y^2 + w^2)).
P4 to_end(int mode, const P4& pi, const double* para) {
  const P4 us = to_start(mode, pi, para);
  const double n2 = (para[0] * para[0] + para[2] * para[2]) + (para[1] * para[1] + para[3] * para[3]);
  const Q4<double> qi{-para[0] / n2, -para[1] / n2, -para[2] / n2, para[3] / n2};
  const V3<double> d{(double)us.x - para[4], (double)us.y - para[5], (double)us.z - para[6]};
  const V3<double> e = rotate(qi, d);
  return P4{(float)e.x, (float)e.y, (float)e.z, (float)int(pi.i)};
}

inline float d2f(const P4& a, const P4& b) {  // FLANN L2_Simple in float
  const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return dx * dx + dy * dy + dz * dz;
}
inline double sqd_float(const P4& a, const P4& b) {  // :478-483, evaluated in float
  return (double)((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z));
}
int nearest(const P4* pts, int n, const P4& q, float* dist) {
  float best = FLT_MAX;
  int bi = -1;
  for (int j = 0; j < n; j++) {
    const float d = d2f(q, pts[j]);
    if (d < best) { best = d; bi = j; }  // ascending j: ties keep the smaller index
  }
  *dist = best;
  return bi;
}

struct Cloud {
  const P4* p;
  int n;
};

void associate_and_solve(int mode, Cloud sharp, Cloud flat, Cloud cornerLast, Cloud surfLast, double* para, int* st) {
  for (int opti = 0; opti < 2; opti++) {
    Problem prob;
    int nc = 0, np = 0;
    for (int i = 0; i < sharp.n; i++) {
      const P4 sel = to_start(mode, sharp.p[i], para);
      float d;
      const int ci = nearest(cornerLast.p, cornerLast.n, sel, &d);
      int closest = -1, min2 = -1;
      if (ci >= 0 && (double)d < DIST_SQ) {
        closest = ci;
        const int cid = int(cornerLast.p[closest].i);
        double best2 = DIST_SQ;
        for (int j = closest + 1; j < cornerLast.n; ++j) {
          if (int(cornerLast.p[j].i) <= cid) continue;
          if ((double)int(cornerLast.p[j].i) > cid + NEARBY) break;
          const double dd = sqd_float(cornerLast.p[j], sel);
          if (dd < best2) { best2 = dd; min2 = j; }
        }
        for (int j = closest - 1; j >= 0; --j) {
          if (int(cornerLast.p[j].i) >= cid) continue;
          if ((double)int(cornerLast.p[j].i) < cid - NEARBY) break;
          const double dd = sqd_float(cornerLast.p[j], sel);
          if (dd < best2) { best2 = dd; min2 = j; }
        }
      }
      if (min2 >= 0) {
        Block b;
        b.kind = 0;
        const P4& c = sharp.p[i];
        const P4& a = cornerLast.p[closest];
        const P4& bb = cornerLast.p[min2];
        b.e = EdgeFactor{{c.x, c.y, c.z}, {a.x, a.y, a.z}, {bb.x, bb.y, bb.z}, rel_s(mode, c)};
        prob.blocks.push_back(b);
        nc++;
      }
    }
    for (int i = 0; i < flat.n; i++) {
      const P4 sel = to_start(mode, flat.p[i], para);
      float d;
      const int ci = nearest(surfLast.p, surfLast.n, sel, &d);
      if (!(ci >= 0 && (double)d < DIST_SQ)) continue;
      const int closest = ci;
      int min2 = -1, min3 = -1;
      const int cid = int(surfLast.p[closest].i);
      double best2 = DIST_SQ, best3 = DIST_SQ;
      for (int j = closest + 1; j < surfLast.n; ++j) {
        if ((double)int(surfLast.p[j].i) > cid + NEARBY) break;
        const double dd = sqd_float(surfLast.p[j], sel);
        if (int(surfLast.p[j].i) <= cid && dd < best2) { best2 = dd; min2 = j; }
        else if (int(surfLast.p[j].i) > cid && dd < best3) { best3 = dd; min3 = j; }
      }
      for (int j = closest - 1; j >= 0; --j) {
        if ((double)int(surfLast.p[j].i) < cid - NEARBY) break;
        const double dd = sqd_float(surfLast.p[j], sel);
        if (int(surfLast.p[j].i) >= cid && dd < best2) { best2 = dd; min2 = j; }
        else if (int(surfLast.p[j].i) < cid && dd < best3) { best3 = dd; min3 = j; }
      }
      if (min2 >= 0 && min3 >= 0) {
        const P4& c = flat.p[i];
        const P4& a = surfLast.p[closest];
        const P4& b2 = surfLast.p[min2];
        const P4& b3 = surfLast.p[min3];
        const double cc[3] = {c.x, c.y, c.z}, aa[3] = {a.x, a.y, a.z};
        const double bb[3] = {b2.x, b2.y, b2.z}, dd[3] = {b3.x, b3.y, b3.z};
        Block b;
        b.kind = 1;
        b.p = PlaneFactor(cc, aa, bb, dd, rel_s(mode, c));
        prob.blocks.push_back(b);
        np++;
      }
    }
    st[2 * opti + 0] = nc;
    st[2 * opti + 1] = np;
    const SolveSummary s = ceres_solve(prob, para, 4);
    st[4 + opti] = s.iterations;
  }
}

}  // namespace

extern "C" {

// A fresh laserOdometry node over n frames, shaped like oracle_odometry_chain_gated (clouds
// concatenated, n + 1 offsets in points, use_aloam nullable) plus the mode, the full-resolution
// clouds (nullable) and, for mode 2, the three clouds as the block :762-790 leaves them
// (out_corner_last / out_surf_last / out_full_end: the inputs' sizes and offsets; nullable).
// out_stats[6n] = corner / plane counts of the two passes, LM iterations of the two passes.
int deskew_odometry_chain(int mode, int n, const float* sharp, const int* sharp_off, const float* less_sharp,
                          const int* less_sharp_off, const float* flat, const int* flat_off, const float* less_flat,
                          const int* less_flat_off, const float* full, const int* full_off, const int* use_aloam,
                          double* out_pose, double* out_rel, int* out_stats, float* out_corner_last,
                          float* out_surf_last, float* out_full_end) {
  if (mode < 0 || mode > 2) return -1;
  double para[7] = {0, 0, 0, 1, 0, 0, 0};
  Q4<double> qw{0, 0, 0, 1};
  double tw[3] = {0, 0, 0};
  const P4* S = reinterpret_cast<const P4*>(sharp);
  const P4* LS = reinterpret_cast<const P4*>(less_sharp);
  const P4* F = reinterpret_cast<const P4*>(flat);
  const P4* LF = reinterpret_cast<const P4*>(less_flat);
  const P4* FU = reinterpret_cast<const P4*>(full);
  std::vector<P4> cornerLast, surfLast, cornerCur, surfCur;
  for (int f = 0; f < n; f++) {
    const Cloud sh{S + sharp_off[f], sharp_off[f + 1] - sharp_off[f]};
    const Cloud fl{F + flat_off[f], flat_off[f + 1] - flat_off[f]};
    cornerCur.assign(LS + less_sharp_off[f], LS + less_sharp_off[f + 1]);
    surfCur.assign(LF + less_flat_off[f], LF + less_flat_off[f + 1]);
    int st[6] = {0, 0, 0, 0, 0, 0};
    if (f > 0) {  // systemInited
      if (!use_aloam || use_aloam[f])
        associate_and_solve(mode, sh, fl, Cloud{cornerLast.data(), (int)cornerLast.size()},
                            Cloud{surfLast.data(), (int)surfLast.size()}, para, st);
      // :716-717
      const V3<double> tr = rotate(qw, V3<double>{para[4], para[5], para[6]});
      tw[0] = tw[0] + tr.x; tw[1] = tw[1] + tr.y; tw[2] = tw[2] + tr.z;
      qw = qmul(qw, Q4<double>{para[0], para[1], para[2], para[3]});
    }
    if (out_pose) {
      double* o = out_pose + 7 * f;
      o[0] = qw.x; o[1] = qw.y; o[2] = qw.z; o[3] = qw.w; o[4] = tw[0]; o[5] = tw[1]; o[6] = tw[2];
    }
    if (out_rel) std::memcpy(out_rel + 7 * f, para, sizeof(para));
    if (out_stats) std::memcpy(out_stats + 6 * f, st, sizeof(st));
    if (mode == 2) {  // :762-790, after the systemInited if / else: the first frame and gated-off frames too
      for (P4& p : cornerCur) p = to_end(mode, p, para);
      for (P4& p : surfCur) p = to_end(mode, p, para);
      if (out_corner_last && !cornerCur.empty())
        std::memcpy(out_corner_last + 4 * (size_t)less_sharp_off[f], cornerCur.data(), sizeof(P4) * cornerCur.size());
      if (out_surf_last && !surfCur.empty())
        std::memcpy(out_surf_last + 4 * (size_t)less_flat_off[f], surfCur.data(), sizeof(P4) * surfCur.size());
      if (FU && full_off && out_full_end)
        for (int i = full_off[f]; i < full_off[f + 1]; i++)
          reinterpret_cast<P4*>(out_full_end)[i] = to_end(mode, FU[i], para);
    }
    cornerLast.swap(cornerCur);  // :793-808
    surfLast.swap(surfCur);
  }
  return 0;
}

}  // extern "C"
