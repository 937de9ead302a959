// TEST INFRASTRUCTURE ONLY.  The arithmetic of the CPU restatement of mapOptimization's sliding-
// window step (tests/restate_mapwin.py) over the oracle's headers, without touching oracle/:
//   mapwin_solve      ceres::Solve(DENSE_QR, max_iterations) under HuberLoss(0.1) over a mixed record
//                     list: kind 2 LidarPlaneNormFactor(curr, n, d) (mapOptimization.cpp:424) and
//                     kind 3 FeatureMatchingResidual(src, dst) (:350), -1 skipped; blocks in list order
//   mapwin_compose    transformAssociateToMap (:730-736)
//   mapwin_update     transformUpdate (:740-746)
//   mapwin_to_world   pcl::transformPointCloud by (q, t): double transform, stored as float
//   mapwin_point_world  q * Vector3d(p) + t (:339-340), Eigen's _transformVector
// Same expressions, in the same order, as oracle_map.cpp's mapopt step, so that with an empty window
// the restated step is that step bit for bit.
#include <vector>

#include "oracle_common.hpp"
#include "oracle_jet.hpp"
#include "oracle_solver.hpp"

namespace {

using namespace oracle;

void qrot(const double* q, const double* v, double* o) {
  const double u[3] = {2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])};
  const double c[3] = {q[1] * u[2] - q[2] * u[1], q[2] * u[0] - q[0] * u[2], q[0] * u[1] - q[1] * u[0]};
  for (int k = 0; k < 3; k++) o[k] = (v[k] + q[3] * u[k]) + c[k];
}

}  // namespace

extern "C" {

void mapwin_solve(const double* rec, const int* kind, int n, double* x, int max_iterations, int* summary) {
  Problem P;
  P.huber_a = 0.1;
  for (int i = 0; i < n; i++) {
    const double* r = rec + (size_t)i * 9;
    if (kind[i] < 0) continue;
    Block b{};
    if (kind[i] == 3) {
      b.kind = 3;
      for (int k = 0; k < 3; k++) { b.pp.src[k] = r[k]; b.pp.dst[k] = r[3 + k]; }
    } else {
      b.kind = 2;
      for (int k = 0; k < 3; k++) { b.pn.cp[k] = r[k]; b.pn.n[k] = r[3 + k]; }
      b.pn.d = r[6];
    }
    P.blocks.push_back(b);
  }
  const SolveSummary s = ceres_solve(P, x, max_iterations);
  summary[0] = s.iterations;
  summary[1] = s.termination;
}

// x = (q_wmap_wodom * q_wodom_curr, q_wmap_wodom * t_wodom_curr + t_wmap_wodom)
void mapwin_compose(const double* state, const double* odom, double* x) {
  const Q4<double> qw = qmul(Q4<double>{state[0], state[1], state[2], state[3]}, Q4<double>{odom[0], odom[1], odom[2], odom[3]});
  x[0] = qw.x; x[1] = qw.y; x[2] = qw.z; x[3] = qw.w;
  double tr[3];
  qrot(state, odom + 4, tr);
  for (int k = 0; k < 3; k++) x[4 + k] = tr[k] + state[4 + k];
}

// q_wmap_wodom = q_w_curr q_wodom_curr^-1; t_wmap_wodom = t_w_curr - q_wmap_wodom t_wodom_curr
void mapwin_update(const double* x, const double* odom, double* state) {
  const Q4<double> nq = qmul(Q4<double>{x[0], x[1], x[2], x[3]}, Q4<double>{-odom[0], -odom[1], -odom[2], odom[3]});
  state[0] = nq.x; state[1] = nq.y; state[2] = nq.z; state[3] = nq.w;
  double r[3];
  qrot(state, odom + 4, r);
  for (int k = 0; k < 3; k++) state[4 + k] = x[4 + k] - r[k];
}

void mapwin_to_world(const double* x, const float* p, int n, float* w) {
  for (int i = 0; i < n; i++) {
    const double v[3] = {p[(size_t)i * 4], p[(size_t)i * 4 + 1], p[(size_t)i * 4 + 2]};
    double o[3];
    qrot(x, v, o);
    for (int k = 0; k < 3; k++) w[(size_t)i * 4 + k] = (float)(o[k] + x[4 + k]);
    w[(size_t)i * 4 + 3] = 0.f;
  }
}

void mapwin_point_world(const double* x, const float* p, double* w) {
  const double v[3] = {p[0], p[1], p[2]};
  double o[3];
  qrot(x, v, o);
  for (int k = 0; k < 3; k++) w[k] = o[k] + x[4 + k];
}

}  // extern "C"
