// Pose-graph optimization (lislam_pgo_*): the factor graph of feature_tracker::mapOdomHandle and
// loopClosureThread (src/intensity_feature_tracker.cpp:395-583, :314-381) -- a prior on the first
// keyframe, a BetweenFactor<Pose3> per consecutive pair, one per accepted ICP loop -- as a
// device-resident least-squares problem, solved in batch by Levenberg-Marquardt.  It replaces
// iSAM2's incremental update with the batch optimum of the same factors.
//
//   k_pgo_linearize  one thread per factor: residual, both 6x6 Jacobians (in registers), the IRLS
//                    weight and cost term; writes either the cost term alone, the factor's blocks of
//                    the normal equations (w Jf'Jf, w Jt'Jt, w Jf'Jt, w Jf'e, w Jt'e), or the raw
//                    residual / Jacobians (lislam_pgo_linearize)
//   k_pgo_assemble   per node: its diagonal block, its block to node + 1 and its gradient, summed over
//                    the node's incident factors in factor-id order through the adjacency index
//                    (no atomics: the same graph gives the same bytes every run)
//   k_pgo_sum        the cost: a fixed-order sum of the factors' terms
//   k_pgo_factor     block LDL' of the block-tridiagonal part of H + lambda diag(H), one wave, 36 lanes
//                    = the 36 elements of a block (block Thomas; cyclic reduction is not built)
//   k_pgo_cg         the whole preconditioned CG solve in one workgroup: matrix-vector products and
//                    dot products by 256 threads, the two Thomas sweeps of each preconditioner
//                    application by wave 0; its scalars never leave the device
//   k_pgo_retract    T <- T Exp(delta) into the trial poses
//   k_pgo_add_batch  nodes and odometry edges from the LISLAM_OUT_POSE rows of a batch
//   k_pgo_pose6d     PointTypePose (x, y, z, roll, pitch, yaw) of the nodes
//
// All arithmetic is double, no FMA contraction (-ffp-contract=off).  tests/restate_pgo.py is the same
// problem in numpy.  Tangent vectors are [omega, v]; ad(xi) = [[W, 0], [V, W]] has the minimal
// polynomial x (x^2 + th^2)^2, so D = Jr^-1(xi) = I + ad / 2 + a2 ad^2 + a4 ad^4 exactly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lislam_batch.hpp"
#include "lislam_ctx.hpp"
#include "lislam_device.hpp"
#include "lislam_host.hpp"

namespace lislam {
namespace pgo {

constexpr int kThreads = 256;
// Below kSmall the coefficient functions use their series (truncation below 1e-16 relative there; the
// closed forms cancel to about 60 eps / angle^2 = 1e-10 at worst); below kTiny = |vec q| the quaternion
// logarithm's atan2(n, w) / n is replaced by its limit.  An exact-chain graph (residuals of 1e-16) takes both.
constexpr double kSmall = 1e-2, kTiny = 1e-8;
constexpr double kLambdaMin = 1e-12, kLambdaMax = 1e10, kDiagMin = 1e-6, kDiagMax = 1e32;

struct Pose {
  double q[4];  // x y z w
  double t[3];
};

__device__ __forceinline__ Pose load_pose(const double* __restrict__ p) {
  Pose o;
  const double x = p[0], y = p[1], z = p[2], w = p[3];
  const double n = sqrt(x * x + y * y + z * z + w * w);
  o.q[0] = x / n; o.q[1] = y / n; o.q[2] = z / n; o.q[3] = w / n;
  o.t[0] = p[4]; o.t[1] = p[5]; o.t[2] = p[6];
  return o;
}

__device__ __forceinline__ void q_mul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

__device__ __forceinline__ void q_rot(const double* q, double* R /*row-major 3x3*/) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// a^-1 b
__device__ __forceinline__ Pose between(const Pose& a, const Pose& b) {
  Pose o;
  const double qi[4] = {-a.q[0], -a.q[1], -a.q[2], a.q[3]};
  q_mul(qi, b.q, o.q);
  double R[9];
  q_rot(qi, R);
  const double d[3] = {b.t[0] - a.t[0], b.t[1] - a.t[1], b.t[2] - a.t[2]};
#pragma unroll
  for (int r = 0; r < 3; r++) o.t[r] = R[r * 3] * d[0] + R[r * 3 + 1] * d[1] + R[r * 3 + 2] * d[2];
  return o;
}

__device__ __forceinline__ void cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void skew(const double* w, double* S) {
  S[0] = 0; S[1] = -w[2]; S[2] = w[1];
  S[3] = w[2]; S[4] = 0; S[5] = -w[0];
  S[6] = -w[1]; S[7] = w[0]; S[8] = 0;
}

__device__ __forceinline__ void mul3(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}

// xi = Log(p): the rotation vector of the unit quaternion (angle below pi), v = V^-1 t with
// V^-1 = I - W / 2 + c W^2, c = (1 - (th / 2) cot(th / 2)) / th^2.
__device__ __forceinline__ void se3_log(const Pose& p, double* xi) {
  double v[3] = {p.q[0], p.q[1], p.q[2]}, w = p.q[3];
  if (w < 0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; w = -w; }
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double k = n < kTiny ? 2.0 / w * (1.0 - n * n / (3.0 * w * w)) : 2.0 * atan2(n, w) / n;
  xi[0] = k * v[0]; xi[1] = k * v[1]; xi[2] = k * v[2];
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  double c;
  if (th < kSmall) {
    const double t2 = th * th;
    c = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
  } else {
    const double g = 0.5 * th * cos(0.5 * th) / sin(0.5 * th);
    c = (1.0 - g) / (th * th);
  }
  double wt[3], wwt[3];
  cross(xi, p.t, wt);
  cross(xi, wt, wwt);
#pragma unroll
  for (int r = 0; r < 3; r++) xi[3 + r] = p.t[r] - 0.5 * wt[r] + c * wwt[r];
}

// Exp(xi): q = (sin(th / 2) / th w, cos(th / 2)), t = (I + b W + c W^2) v
__device__ __forceinline__ Pose se3_exp(const double* xi) {
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), t2 = th * th;
  double a, b, c;
  if (th < kSmall) {
    a = 0.5 - t2 / 48.0 + t2 * t2 / 3840.0;
    b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
    c = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
  } else {
    a = sin(0.5 * th) / th;
    b = (1.0 - cos(th)) / t2;
    c = (th - sin(th)) / (t2 * th);
  }
  Pose o;
  o.q[0] = a * xi[0]; o.q[1] = a * xi[1]; o.q[2] = a * xi[2]; o.q[3] = cos(0.5 * th);
  double wv[3], wwv[3];
  cross(xi, xi + 3, wv);
  cross(xi, wv, wwv);
#pragma unroll
  for (int r = 0; r < 3; r++) o.t[r] = xi[3 + r] + b * wv[r] + c * wwv[r];
  return o;
}

// D = Jr^-1(xi) = [[Dr, 0], [Dq, Dr]]: Dr = I + W/2 + a2 W^2 + a4 W^4,
// Dq = V/2 + a2 B + a4 (B W^2 + W^2 B), B = V W + W V.
__device__ __forceinline__ void dlog_blocks(const double* xi, double* Dr, double* Dq) {
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), t2 = th * th;
  double a2, a4;
  if (th < kSmall) {
    a2 = 1.0 / 12.0 - t2 * t2 / 30240.0;
    a4 = -1.0 / 720.0 - t2 / 15120.0;
  } else {
    const double s = sin(0.5 * th), c = cos(0.5 * th);
    const double g = 0.5 * th * c / s;
    const double dg = 0.5 * c / s - 0.25 * th / (s * s);
    a2 = (2.0 * (1.0 - g) + 0.5 * th * dg) / t2;
    a4 = (1.0 - g + 0.5 * th * dg) / (t2 * t2);
  }
  double W[9], V[9], W2[9], W4[9], VW[9], WV[9], B[9], BW2[9], W2B[9];
  skew(xi, W);
  skew(xi + 3, V);
  mul3(W, W, W2);
  mul3(W2, W2, W4);
  mul3(V, W, VW);
  mul3(W, V, WV);
#pragma unroll
  for (int k = 0; k < 9; k++) B[k] = VW[k] + WV[k];
  mul3(B, W2, BW2);
  mul3(W2, B, W2B);
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double id = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    Dr[k] = id + 0.5 * W[k] + a2 * W2[k] + a4 * W4[k];
    Dq[k] = 0.5 * V[k] + a2 * B[k] + a4 * (BW2[k] + W2B[k]);
  }
}

struct Graph {
  const int* from;       // [E]
  const int* to;         // [E]
  const double* meas;    // [E][7]
  const double* sigma;   // [E][6] sqrt(variances)
  const int* robust;     // [E]
  const double* prior;   // [7] pose, [6] sigma
  int prior_node;
  int E;
};

struct Blocks {
  double* Af;    // [E][36]    w Jf'Jf      (raw mode: J_from)
  double* At;    // [E+1][36]  w Jt'Jt      (raw mode: J_to)
  double* W;     // [E][36]    w Jf'Jt
  double* bf;    // [E][6]     w Jf'e
  double* bt;    // [E+1][6]   w Jt'e       (raw mode: the residual)
  double* wt;    // [E+1]      IRLS weight
  double* term;  // [E+1]      cost term
};

enum { kCost = 0, kNormal = 1, kRaw = 2 };

// C = w A' B of two 6x6 row-major blocks
__device__ __forceinline__ void atb(const double* A, const double* B, double w, double* __restrict__ out) {
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += A[k * 6 + r] * B[k * 6 + c];
      out[r * 6 + c] = w * s;
    }
}

template <int kMode>
__global__ __launch_bounds__(64) void k_pgo_linearize(Graph G, const double* __restrict__ x, Blocks o) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f > G.E) return;
  const bool edge = f < G.E;
  const Pose Tj = load_pose(x + (size_t)(edge ? G.to[f] : G.prior_node) * 7);
  Pose h = Tj;
  if (edge) h = between(load_pose(x + (size_t)G.from[f] * 7), Tj);
  const Pose Z = load_pose(edge ? G.meas + (size_t)f * 7 : G.prior);
  const double* sg = edge ? G.sigma + (size_t)f * 6 : G.prior + 7;
  double sig[6], xi[6], e[6];
#pragma unroll
  for (int k = 0; k < 6; k++) sig[k] = sg[k];
  se3_log(between(Z, h), xi);
  double s = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    e[k] = xi[k] / sig[k];
    s += e[k] * e[k];
  }
  const bool robust = edge && G.robust[f] != 0;
  const double w = robust ? 1.0 / (1.0 + s) : 1.0;
  o.term[f] = robust ? 0.5 * log1p(s) : 0.5 * s;
  if (kMode == kCost) return;

  double Dr[9], Dq[9];
  dlog_blocks(xi, Dr, Dq);
  double Jt[36], Jf[36];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      Jt[r * 6 + c] = Dr[r * 3 + c] / sig[r];
      Jt[r * 6 + 3 + c] = 0.0;
      Jt[(3 + r) * 6 + c] = Dq[r * 3 + c] / sig[3 + r];
      Jt[(3 + r) * 6 + 3 + c] = Dr[r * 3 + c] / sig[3 + r];
    }
  if (edge) {
    // Ad(h^-1) = [[R', 0], [skew(-R't) R', R']]
    double R[9], Rt[9], tp[3], S[9], SRt[9], M0[9], M1[9], M2[9];
    q_rot(h.q, R);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Rt[r * 3 + c] = R[c * 3 + r];
#pragma unroll
    for (int r = 0; r < 3; r++) tp[r] = -(Rt[r * 3] * h.t[0] + Rt[r * 3 + 1] * h.t[1] + Rt[r * 3 + 2] * h.t[2]);
    skew(tp, S);
    mul3(S, Rt, SRt);
    mul3(Dr, Rt, M0);   // Dr R'
    mul3(Dq, Rt, M1);   // Dq R'
    mul3(Dr, SRt, M2);  // Dr skew(t') R'
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        Jf[r * 6 + c] = -M0[r * 3 + c] / sig[r];
        Jf[r * 6 + 3 + c] = 0.0;
        Jf[(3 + r) * 6 + c] = -(M1[r * 3 + c] + M2[r * 3 + c]) / sig[3 + r];
        Jf[(3 + r) * 6 + 3 + c] = -M0[r * 3 + c] / sig[3 + r];
      }
  }
  o.wt[f] = w;
  if (kMode == kRaw) {
#pragma unroll
    for (int k = 0; k < 6; k++) o.bt[(size_t)f * 6 + k] = e[k];
#pragma unroll
    for (int k = 0; k < 36; k++) o.At[(size_t)f * 36 + k] = Jt[k];
    if (edge) {
#pragma unroll
      for (int k = 0; k < 36; k++) o.Af[(size_t)f * 36 + k] = Jf[k];
    }
    return;
  }
  atb(Jt, Jt, w, o.At + (size_t)f * 36);
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double s1 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) s1 += Jt[k * 6 + c] * e[k];
    o.bt[(size_t)f * 6 + c] = w * s1;
  }
  if (edge) {
    atb(Jf, Jf, w, o.Af + (size_t)f * 36);
    atb(Jf, Jt, w, o.W + (size_t)f * 36);
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s1 = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) s1 += Jf[k * 6 + c] * e[k];
      o.bf[(size_t)f * 6 + c] = w * s1;
    }
  }
}

// Adjacency: node n's incident factors are adj[adj_off[n] .. adj_off[n + 1]), ascending factor id,
// each coded 2 * factor + side (0: n is the factor's `from`, 1: its `to`; the prior is factor E, side 1).
struct Adj {
  const int* off;
  const int* inc;
};

// 48 threads per node: 36 elements of the diagonal block and of the block to node + 1, 6 of the gradient.
__global__ __launch_bounds__(kThreads) void k_pgo_assemble(int N, Graph G, Adj A, Blocks b, double* __restrict__ Hd,
                                                           double* __restrict__ U, double* __restrict__ g) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int n = idx / 48, t = idx % 48;
  if (n >= N || t >= 42) return;
  const int lo = A.off[n], hi = A.off[n + 1];
  if (t < 36) {
    const int tt = (t % 6) * 6 + t / 6;  // the transposed element
    double d = 0, u = 0;
    for (int k = lo; k < hi; k++) {
      const int f = A.inc[k] >> 1, side = A.inc[k] & 1;
      d += side ? b.At[(size_t)f * 36 + t] : b.Af[(size_t)f * 36 + t];
      if (f < G.E) {
        const int other = side ? G.from[f] : G.to[f];
        if (other == n + 1) u += side ? b.W[(size_t)f * 36 + tt] : b.W[(size_t)f * 36 + t];
      }
    }
    Hd[(size_t)n * 36 + t] = d;
    U[(size_t)n * 36 + t] = u;
  } else {
    const int c = t - 36;
    double s = 0;
    for (int k = lo; k < hi; k++) {
      const int f = A.inc[k] >> 1, side = A.inc[k] & 1;
      s += side ? b.bt[(size_t)f * 6 + c] : b.bf[(size_t)f * 6 + c];
    }
    g[(size_t)n * 6 + c] = s;
  }
}

// Sum of v over the workgroup, the same on every thread, in a fixed order.
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// What one LM iteration hands back to the host (one copy, one synchronisation).
struct Result {
  double cost_cur, cost_try, cg_relres;
  int cg_iterations, pad;
};

__global__ __launch_bounds__(kThreads) void k_pgo_sum(int n, const double* __restrict__ term, double* __restrict__ out) {
  __shared__ double red[kThreads];
  double s = 0;
  for (int k = threadIdx.x; k < n; k += kThreads) s += term[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = s;
}

__device__ __forceinline__ double damped(double d) { return fmin(fmax(d, kDiagMin), kDiagMax); }

// Block LDL' of the block-tridiagonal M (diagonal A_n = Hd_n + lambda clamp(diag Hd_n), M(n, n+1) = U_n):
// S_0 = A_0, L_n = U_{n-1}' S_{n-1}^-1, S_n = A_n - L_n U_{n-1}.  Stores S_n^-1 and L_n.  One wave;
// lane 6 r + c owns element (r, c); the blocks go round through LDS.  M is positive definite (the chain's
// Hessian plus a positive semi-definite block diagonal per loop edge plus the damping), so the
// Gauss-Jordan inverse needs no pivoting.
__global__ __launch_bounds__(64) void k_pgo_factor(int N, double lambda, const double* __restrict__ Hd,
                                                   const double* __restrict__ U, double* __restrict__ Sinv,
                                                   double* __restrict__ L) {
  __shared__ double s[36], v[36], l[36];
  const int t = threadIdx.x < 36 ? threadIdx.x : 35, r = t / 6, c = t % 6;
  const bool on = threadIdx.x < 36;
  // the next step's blocks are loaded a step ahead: they do not depend on the recurrence
  double a_next = Hd[t], Ucp[6] = {0, 0, 0, 0, 0, 0};
  for (int n = 0; n < N; n++) {
    double a = a_next, Uc[6], Ur[6];  // U_n as (k, c) for S_{n+1} and as (k, r) for L_{n+1}
    if (n + 1 < N) {
      a_next = Hd[(size_t)(n + 1) * 36 + t];
      const double* Un = U + (size_t)n * 36;
#pragma unroll
      for (int k = 0; k < 6; k++) { Uc[k] = Un[k * 6 + c]; Ur[k] = Un[k * 6 + r]; }
    } else {
#pragma unroll
      for (int k = 0; k < 6; k++) Uc[k] = Ur[k] = 0.0;
    }
    if (r == c) a = a + lambda * damped(a);
    if (n > 0) {
#pragma unroll
      for (int k = 0; k < 6; k++) a -= l[r * 6 + k] * Ucp[k];
    }
    double inv = r == c ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      wave_lds_sync();
      if (on) { s[t] = a; v[t] = inv; }
      wave_lds_sync();
      const double p = s[k * 6 + k], sk = s[k * 6 + c] / p, vk = v[k * 6 + c] / p, fk = s[r * 6 + k];
      if (r == k) { a = sk; inv = vk; }
      else { a -= fk * sk; inv -= fk * vk; }
    }
    if (on) Sinv[(size_t)n * 36 + t] = inv;
    if (n + 1 < N) {
      wave_lds_sync();
      if (on) v[t] = inv;
      wave_lds_sync();
      double ln = 0;
#pragma unroll
      for (int k = 0; k < 6; k++) ln += Ur[k] * v[k * 6 + c];
      if (on) { l[t] = ln; L[(size_t)(n + 1) * 36 + t] = ln; }
      wave_lds_sync();
    }
#pragma unroll
    for (int k = 0; k < 6; k++) Ucp[k] = Uc[k];
  }
}

// lane `src`'s value on every lane (src is a compile-time constant after unrolling)
__device__ __forceinline__ double lane_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

struct Cg {
  int N, E, max_iterations;
  double lambda, rel_tol;
  const double* Hd;    // [N][36]
  const double* W;     // [E][36]
  const double* g;     // [N][6]
  const double* Sinv;  // [N][36]
  const double* L;     // [N][36]
  double* x;           // [N][6] the step
  double* r;
  double* z;
  double* p;
  double* Ap;
  double* y;
};

// z = M^-1 r through the factorization: forward y_n = r_n - L_n y_{n-1} (wave 0, lane = row, the
// previous y broadcast from its lanes), z_n = S_n^-1 y_n (every thread), backward
// z_n -= L_{n+1}' z_{n+1} (wave 0).  Every wave of the workgroup calls it.  A sweep loads kChunk
// steps' blocks at once (they do not depend on the recurrence) and then runs those steps from
// registers, so a step waits on no memory.
constexpr int kChunk = 16;
__device__ void precondition(const Cg& a) {
  const int N = a.N, wave = threadIdx.x / 64, r = lane_id() % 6;
  const bool store = lane_id() < 6;
  __syncthreads();
  if (wave == 0) {
    double yv = a.r[r];
    if (store) a.y[r] = yv;
    for (int n0 = 1; n0 < N; n0 += kChunk) {
      double Lr[kChunk][6], rv[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; j++) {
        const int n = min(n0 + j, N - 1);  // past the end: an in-bounds load that is not used
        rv[j] = a.r[(size_t)n * 6 + r];
#pragma unroll
        for (int c = 0; c < 6; c++) Lr[j][c] = a.L[(size_t)n * 36 + r * 6 + c];
      }
#pragma unroll
      for (int j = 0; j < kChunk; j++) {
        if (n0 + j < N) {
          double acc = rv[j];
#pragma unroll
          for (int c = 0; c < 6; c++) acc -= Lr[j][c] * lane_bcast(yv, c);
          yv = acc;
          if (store) a.y[(size_t)(n0 + j) * 6 + r] = yv;
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N * 6; i += kThreads) {
    const int n = i / 6, rr = i % 6;
    const double* Sn = a.Sinv + (size_t)n * 36 + rr * 6;
    const double* yn = a.y + (size_t)n * 6;
    double s = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) s += Sn[c] * yn[c];
    a.z[i] = s;
  }
  __syncthreads();
  if (wave == 0) {
    double xv = a.z[(size_t)(N - 1) * 6 + r];
    for (int n0 = N - 2; n0 >= 0; n0 -= kChunk) {
      double Lc[kChunk][6], zv[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; j++) {
        const int n = max(n0 - j, 0);
        zv[j] = a.z[(size_t)n * 6 + r];
#pragma unroll
        for (int c = 0; c < 6; c++) Lc[j][c] = a.L[(size_t)(n + 1) * 36 + c * 6 + r];
      }
#pragma unroll
      for (int j = 0; j < kChunk; j++) {
        if (n0 - j >= 0) {
          double acc = zv[j];
#pragma unroll
          for (int c = 0; c < 6; c++) acc -= Lc[j][c] * lane_bcast(xv, c);
          xv = acc;
          if (store) a.z[(size_t)(n0 - j) * 6 + r] = xv;
        }
      }
    }
  }
  __syncthreads();
}

// Preconditioned CG on (H + lambda D) x = -g in one workgroup.  H's off-diagonal blocks are the
// factors' W through the adjacency index.
__global__ __launch_bounds__(kThreads) void k_pgo_cg(Cg a, Graph G, Adj A, Result* __restrict__ res) {
  __shared__ double red[kThreads];
  const int N = a.N, n6 = N * 6;
  double part = 0;
  for (int i = threadIdx.x; i < n6; i += kThreads) {
    const double v = -a.g[i];
    a.r[i] = v;
    a.x[i] = 0.0;
    part += v * v;
  }
  const double rr0 = block_sum(part, red);
  int iterations = 0;
  double rr = rr0;
  if (rr0 > 0.0) {
    precondition(a);
    part = 0;
    for (int i = threadIdx.x; i < n6; i += kThreads) {
      a.p[i] = a.z[i];
      part += a.r[i] * a.z[i];
    }
    double rz = block_sum(part, red);
    const double stop = a.rel_tol * a.rel_tol * rr0;
    for (int it = 1; it <= a.max_iterations; it++) {
      // Ap = (H + lambda D) p and p'Ap; p was written by other threads
      __syncthreads();
      part = 0;
      for (int n = threadIdx.x; n < N; n += kThreads) {
        const double* Hn = a.Hd + (size_t)n * 36;
        double pn[6], y[6];
#pragma unroll
        for (int c = 0; c < 6; c++) pn[c] = a.p[(size_t)n * 6 + c];
#pragma unroll
        for (int r = 0; r < 6; r++) {
          double s = a.lambda * damped(Hn[r * 6 + r]) * pn[r];
#pragma unroll
          for (int c = 0; c < 6; c++) s += Hn[r * 6 + c] * pn[c];
          y[r] = s;
        }
        for (int k = A.off[n]; k < A.off[n + 1]; k++) {
          const int f = A.inc[k] >> 1, side = A.inc[k] & 1;
          if (f >= G.E) continue;  // the prior has no off-diagonal block
          const double* Wf = a.W + (size_t)f * 36;
          const double* po = a.p + (size_t)(side ? G.from[f] : G.to[f]) * 6;
          double q[6];
#pragma unroll
          for (int c = 0; c < 6; c++) q[c] = po[c];
#pragma unroll
          for (int r = 0; r < 6; r++) {
            double s = 0;
#pragma unroll
            for (int c = 0; c < 6; c++) s += (side ? Wf[c * 6 + r] : Wf[r * 6 + c]) * q[c];
            y[r] += s;
          }
        }
#pragma unroll
        for (int r = 0; r < 6; r++) {
          a.Ap[(size_t)n * 6 + r] = y[r];
          part += pn[r] * y[r];
        }
      }
      const double pAp = block_sum(part, red);
      if (!(pAp > 0.0)) break;
      const double alpha = rz / pAp;
      part = 0;
      for (int i = threadIdx.x; i < n6; i += kThreads) {
        a.x[i] = a.x[i] + alpha * a.p[i];
        const double v = a.r[i] - alpha * a.Ap[i];
        a.r[i] = v;
        part += v * v;
      }
      rr = block_sum(part, red);
      iterations = it;
      if (rr <= stop) break;
      precondition(a);
      part = 0;
      for (int i = threadIdx.x; i < n6; i += kThreads) part += a.r[i] * a.z[i];
      const double rz_new = block_sum(part, red);
      const double beta = rz_new / rz;
      rz = rz_new;
      for (int i = threadIdx.x; i < n6; i += kThreads) a.p[i] = a.z[i] + beta * a.p[i];
    }
  }
  if (threadIdx.x == 0) {
    res->cg_iterations = iterations;
    res->cg_relres = rr0 > 0.0 ? sqrt(rr / rr0) : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void k_pgo_retract(int N, const double* __restrict__ x, const double* __restrict__ dx,
                                                          double* __restrict__ out) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const Pose T = load_pose(x + (size_t)n * 7);
  double d[6];
#pragma unroll
  for (int k = 0; k < 6; k++) d[k] = dx[(size_t)n * 6 + k];
  const Pose X = se3_exp(d);
  double q[4], R[9];
  q_mul(T.q, X.q, q);
  q_rot(T.q, R);
  const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double* o = out + (size_t)n * 7;
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = q[k] / nn;
#pragma unroll
  for (int r = 0; r < 3; r++) o[4 + r] = T.t[r] + (R[r * 3] * X.t[0] + R[r * 3 + 1] * X.t[1] + R[r * 3 + 2] * X.t[2]);
}

// Scan first + k of a batch becomes node base + k (its LISLAM_OUT_POSE row, byte for byte); edge
// ebase + k - k0 ties it to the scan before: pose[k-1]^-1 pose[k] (k0 = 1 when scan `first` has none).
__global__ __launch_bounds__(kThreads) void k_pgo_add_batch(int n, int k0, const double* __restrict__ pose /*at scan first*/,
                                                            int base, int ebase, double* __restrict__ x, int* __restrict__ from,
                                                            int* __restrict__ to, double* __restrict__ meas,
                                                            double* __restrict__ sigma, int* __restrict__ robust,
                                                            const double* __restrict__ sig6) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
#pragma unroll
  for (int e = 0; e < 7; e++) x[(size_t)(base + k) * 7 + e] = pose[(ptrdiff_t)k * 7 + e];
  if (k < k0) return;
  const int id = ebase + k - k0;
  const Pose z = between(load_pose(pose + (ptrdiff_t)(k - 1) * 7), load_pose(pose + (ptrdiff_t)k * 7));
  from[id] = base + k - 1;
  to[id] = base + k;
  robust[id] = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) meas[(size_t)id * 7 + e] = z.q[e];
#pragma unroll
  for (int e = 0; e < 3; e++) meas[(size_t)id * 7 + 4 + e] = z.t[e];
#pragma unroll
  for (int e = 0; e < 6; e++) sigma[(size_t)id * 6 + e] = sig6[e];
}

// lislam_pgo_add_keyframes: keyframe k = pose[index[k]] becomes node base + k (the row, byte for byte);
// edge ebase + k - k0 measures prev^-1 pose[index[k]], prev = pose[index[k-1]], for k = 0 the pose the
// graph's last node was added with (k0 = 1 when the graph was empty).  The last keyframe's row is
// left in added_out for the next call (another buffer than added_in: thread 0 reads that one).
__global__ __launch_bounds__(kThreads) void k_pgo_add_keyframes(int n, int k0, const double* __restrict__ pose,
                                                                const int* __restrict__ index,
                                                                const double* __restrict__ added_in,
                                                                double* __restrict__ added_out, int base, int ebase,
                                                                double* __restrict__ x, int* __restrict__ from,
                                                                int* __restrict__ to, double* __restrict__ meas,
                                                                double* __restrict__ sigma, int* __restrict__ robust,
                                                                const double* __restrict__ sig6) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const double* cur = pose + (size_t)index[k] * 7;
#pragma unroll
  for (int e = 0; e < 7; e++) x[(size_t)(base + k) * 7 + e] = cur[e];
  if (k == n - 1) {
#pragma unroll
    for (int e = 0; e < 7; e++) added_out[e] = cur[e];
  }
  if (k < k0) return;
  const int id = ebase + k - k0;
  const double* prev = k > 0 ? pose + (size_t)index[k - 1] * 7 : added_in;
  const Pose z = between(load_pose(prev), load_pose(cur));
  from[id] = base + k - 1;
  to[id] = base + k;
  robust[id] = 0;
#pragma unroll
  for (int e = 0; e < 4; e++) meas[(size_t)id * 7 + e] = z.q[e];
#pragma unroll
  for (int e = 0; e < 3; e++) meas[(size_t)id * 7 + 4 + e] = z.t[e];
#pragma unroll
  for (int e = 0; e < 6; e++) sigma[(size_t)id * 6 + e] = sig6[e];
}

// PointTypePose of each node as getTransformMatrix (:152-165) reads it back: R = Rz(roll) Ry(pitch) Rx(yaw).
__global__ __launch_bounds__(kThreads) void k_pgo_pose6d(int n, const double* __restrict__ x, float* __restrict__ out) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const Pose T = load_pose(x + (size_t)k * 7);
  double R[9];
  q_rot(T.q, R);
  float* o = out + (size_t)k * 6;
  o[0] = (float)T.t[0]; o[1] = (float)T.t[1]; o[2] = (float)T.t[2];
  o[3] = (float)atan2(R[3], R[0]);
  o[4] = (float)asin(fmin(1.0, fmax(-1.0, -R[6])));
  o[5] = (float)atan2(R[7], R[8]);
}

}  // namespace pgo
}  // namespace lislam

using namespace lislam::pgo;
using namespace lislam;

struct lislam_pgo {
  lislam_ctx* ctx = nullptr;
  lislam_pgo_config cfg{};
  int ncap = 0, ecap = 0, n = 0, e = 0;
  int prior_node = -1;
  bool adj_dirty = true;
  std::vector<int> h_from, h_to;  // host copy of the edge list (the adjacency index is built from it)
  std::vector<void*> allocs;
  double* x[2] = {nullptr, nullptr};  // current / trial poses
  int cur = 0;
  int *from = nullptr, *to = nullptr, *robust = nullptr;
  double *meas = nullptr, *sigma = nullptr, *prior = nullptr, *odom_sigma = nullptr;
  // the pose the last node was added with (graph_prev_rotation_ / graph_prev_translation_, :513-514):
  // added[added_cur]; lislam_pgo_add_keyframes reads it and writes the other one
  double* added[2] = {nullptr, nullptr};
  int added_cur = 0;
  // grow-only staging of lislam_pgo_add_keyframes: [pose7 n_poses x 7][index n]
  DBuf kstage;
  int *adj_off = nullptr, *adj = nullptr;
  Blocks b{};
  double *Hd = nullptr, *U = nullptr, *g = nullptr, *Sinv = nullptr, *L = nullptr;
  double* vec[6] = {};  // dx, r, z, p, Ap, y
  float* p6 = nullptr;
  Result* d_res = nullptr;
  Result* h_res = nullptr;  // pinned
  Graph graph() const { return Graph{from, to, meas, sigma, robust, prior, prior_node, e}; }
  Adj adjacency() const { return Adj{adj_off, adj}; }
};

namespace {

const double kOdometryVariances[6] = {1e-6, 1e-6, 1e-6, 1e-8, 1e-8, 1e-6};  // odometryNoise_ (:41-44)

template <typename T>
bool dalloc(lislam_pgo* p, T** out, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return false;
  p->allocs.push_back(q);
  *out = static_cast<T*>(q);
  return true;
}

void free_pgo(lislam_pgo* p) {
  for (void* q : p->allocs) (void)hipFree(q);
  if (p->h_res) (void)hipHostFree(p->h_res);
  delete p;
}

bool positive(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!(v[k] > 0) || !std::isfinite(v[k])) return false;
  return true;
}

bool finite_pose(const double* p) {
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(p[k])) return false;
  return p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3] > 0;
}

// The adjacency index of the current edge list and prior, uploaded when it changed.
int sync_adjacency(lislam_pgo* p) {
  if (!p->adj_dirty) return LISLAM_OK;
  lislam_ctx* c = p->ctx;
  std::vector<int> off(p->n + 1, 0), inc((size_t)2 * p->e + 1);
  for (int k = 0; k < p->e; k++) { off[p->h_from[k] + 1]++; off[p->h_to[k] + 1]++; }
  if (p->prior_node >= 0) off[p->prior_node + 1]++;
  for (int k = 0; k < p->n; k++) off[k + 1] += off[k];
  std::vector<int> fill(off.begin(), off.end() - 1);
  for (int k = 0; k < p->e; k++) {  // ascending factor id per node
    inc[fill[p->h_from[k]]++] = 2 * k;
    inc[fill[p->h_to[k]]++] = 2 * k + 1;
  }
  if (p->prior_node >= 0) inc[fill[p->prior_node]++] = 2 * p->e + 1;
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->adj_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->adj, inc.data(), inc.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));  // the vectors leave scope
  p->adj_dirty = false;
  return LISLAM_OK;
}

template <int kMode>
void launch_linearize(lislam_pgo* p, const double* x) {
  hipLaunchKernelGGL(k_pgo_linearize<kMode>, dim3((p->e + 1 + 63) / 64), dim3(64), 0, p->ctx->stream, p->graph(), x, p->b);
}

int ready(lislam_pgo* p, const char* who) {
  if (p->n > 0 && p->prior_node < 0) return fail(p->ctx, LISLAM_ERR_STATE, "%s: set a prior first (lislam_pgo_set_prior)", who);
  return LISLAM_OK;
}

}  // namespace

extern "C" {

int lislam_pgo_create(lislam_ctx* c, const lislam_pgo_config* cfg, int32_t node_capacity, int32_t edge_capacity, lislam_pgo** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  lislam_pgo_config d = {50, 0, 1e-4, 1e-10, 1e-12};
  if (cfg) d = *cfg;
  if (node_capacity < 1 || edge_capacity < 0 || node_capacity > (1 << 24) || edge_capacity > (1 << 24))
    return fail(c, LISLAM_ERR_ARG, "lislam_pgo_create: node_capacity 1..2^24, edge_capacity 0..2^24");
  if (d.max_iterations < 0 || d.cg_max_iterations < 0 || !(d.lambda_init > 0) || !std::isfinite(d.lambda_init) ||
      !(d.rel_cost_tol >= 0) || !(d.cg_rel_tol >= 0))
    return fail(c, LISLAM_ERR_ARG, "lislam_pgo_create: invalid configuration");
  hipSetDevice(c->device);
  lislam_pgo* p = new lislam_pgo();
  p->ctx = c;
  p->cfg = d;
  p->ncap = node_capacity;
  p->ecap = edge_capacity;
  const size_t N = (size_t)node_capacity, E = (size_t)edge_capacity;
  bool ok = dalloc(p, &p->x[0], N * 7) && dalloc(p, &p->x[1], N * 7) && dalloc(p, &p->from, E) && dalloc(p, &p->to, E) &&
            dalloc(p, &p->robust, E) && dalloc(p, &p->meas, E * 7) && dalloc(p, &p->sigma, E * 6) && dalloc(p, &p->prior, 13) &&
            dalloc(p, &p->odom_sigma, 6) && dalloc(p, &p->added[0], 7) && dalloc(p, &p->added[1], 7) && dalloc(p, &p->adj_off, N + 1) && dalloc(p, &p->adj, 2 * E + 1) &&
            dalloc(p, &p->b.Af, E * 36) && dalloc(p, &p->b.At, (E + 1) * 36) && dalloc(p, &p->b.W, E * 36) &&
            dalloc(p, &p->b.bf, E * 6) && dalloc(p, &p->b.bt, (E + 1) * 6) && dalloc(p, &p->b.wt, E + 1) &&
            dalloc(p, &p->b.term, E + 1) && dalloc(p, &p->Hd, N * 36) && dalloc(p, &p->U, N * 36) && dalloc(p, &p->g, N * 6) &&
            dalloc(p, &p->Sinv, N * 36) && dalloc(p, &p->L, N * 36) && dalloc(p, &p->p6, N * 6) && dalloc(p, &p->d_res, 1);
  for (int k = 0; ok && k < 6; k++) ok = dalloc(p, &p->vec[k], N * 6);
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&p->h_res), sizeof(Result)) == hipSuccess;
  ok = ok && hipMemsetAsync(p->d_res, 0, sizeof(Result), c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    free_pgo(p);
    return fail(c, LISLAM_ERR_DEVICE, "lislam_pgo_create: device allocation failed");
  }
  p->h_from.reserve(E);
  p->h_to.reserve(E);
  *out = p;
  return LISLAM_OK;
}

int lislam_pgo_destroy(lislam_pgo* p) {
  if (!p) return LISLAM_ERR_ARG;
  hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  free_pgo(p);
  return LISLAM_OK;
}

int lislam_pgo_size(lislam_pgo* p, int32_t* nodes, int32_t* edges) {
  if (!p) return LISLAM_ERR_ARG;
  if (nodes) *nodes = p->n;
  if (edges) *edges = p->e;
  return LISLAM_OK;
}

int lislam_pgo_add_nodes(lislam_pgo* p, const double* pose7, int32_t n) {
  if (!p || n < 0 || (n > 0 && !pose7)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n == 0) return LISLAM_OK;
  if ((int64_t)p->n + n > p->ncap)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_pgo_add_nodes: %d + %d nodes exceed the capacity %d", p->n, n, p->ncap);
  for (int k = 0; k < n; k++)
    if (!finite_pose(pose7 + (size_t)k * 7)) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_nodes: pose %d is not finite", k);
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->x[p->cur] + (size_t)p->n * 7, pose7, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->added[p->added_cur], pose7 + (size_t)(n - 1) * 7, 7 * sizeof(double), hipMemcpyHostToDevice,
                                  c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  p->n += n;
  p->adj_dirty = true;
  return LISLAM_OK;
}

int lislam_pgo_set_prior(lislam_pgo* p, int32_t node, const double* pose7, const double* var6) {
  if (!p || !pose7 || !var6) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (node < 0 || node >= p->n) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_set_prior: node %d out of range (size %d)", node, p->n);
  if (!positive(var6, 6) || !finite_pose(pose7)) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_set_prior: variances must be positive, the pose finite");
  double h[13];
  for (int k = 0; k < 7; k++) h[k] = pose7[k];
  for (int k = 0; k < 6; k++) h[7 + k] = std::sqrt(var6[k]);
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->prior, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  p->prior_node = node;
  p->adj_dirty = true;
  return LISLAM_OK;
}

int lislam_pgo_add_edges(lislam_pgo* p, const int32_t* from, const int32_t* to, const double* meas7, const double* var6,
                         const int32_t* robust, int32_t n) {
  if (!p || n < 0 || (n > 0 && (!from || !to || !meas7 || !var6))) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n == 0) return LISLAM_OK;
  for (int k = 0; k < n; k++) {
    if (from[k] < 0 || from[k] >= p->n || to[k] < 0 || to[k] >= p->n || from[k] == to[k])
      return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_edges: edge %d = (%d, %d) invalid (size %d)", k, from[k], to[k], p->n);
    if (!positive(var6 + (size_t)k * 6, 6) || !finite_pose(meas7 + (size_t)k * 7))
      return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_edges: edge %d: variances must be positive, the measurement finite", k);
  }
  if ((int64_t)p->e + n > p->ecap)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_pgo_add_edges: %d + %d edges exceed the capacity %d", p->e, n, p->ecap);
  std::vector<double> sg((size_t)n * 6);
  std::vector<int> rb(n, 0);
  for (size_t k = 0; k < sg.size(); k++) sg[k] = std::sqrt(var6[k]);
  if (robust)
    for (int k = 0; k < n; k++) rb[k] = robust[k] != 0;
  hipSetDevice(c->device);
  const size_t at = (size_t)p->e;
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->from + at, from, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->to + at, to, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->robust + at, rb.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->meas + at * 7, meas7, (size_t)n * 7 * 8, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->sigma + at * 6, sg.data(), (size_t)n * 6 * 8, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  p->h_from.insert(p->h_from.end(), from, from + n);
  p->h_to.insert(p->h_to.end(), to, to + n);
  p->e += n;
  p->adj_dirty = true;
  return LISLAM_OK;
}

int lislam_pgo_add_batch(lislam_pgo* p, lislam_batch* b, int32_t first_scan, int32_t n_scans, const double* var6) {
  if (!p || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  LISLAM_RC(check_same_context(c, "lislam_pgo_add_batch", b));
  LISLAM_RC(check_scan_range(c, "lislam_pgo_add_batch", b, first_scan, n_scans));
  if (var6 && !positive(var6, 6)) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_batch: variances must be positive");
  if (first_scan + n_scans > b->extracted)
    return fail(c, LISLAM_ERR_STATE, "lislam_pgo_add_batch: extract and run the odometry of %d scans first", first_scan + n_scans);
  if (n_scans == 0) return LISLAM_OK;
  // the scan before `first_scan` anchors the first new node when the graph already holds its node
  const int k0 = (p->n > 0 && first_scan > 0) ? 0 : 1;
  const int n_edges = n_scans - k0;
  if ((int64_t)p->n + n_scans > p->ncap || (int64_t)p->e + n_edges > p->ecap)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_pgo_add_batch: %d + %d nodes / %d + %d edges exceed the capacity %d / %d", p->n,
                n_scans, p->e, n_edges, p->ncap, p->ecap);
  int rc = lislam_batch_settle(b);
  if (rc != LISLAM_OK) return rc;
  hipSetDevice(c->device);
  double sg[6];
  for (int k = 0; k < 6; k++) sg[k] = std::sqrt(var6 ? var6[k] : kOdometryVariances[k]);
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->odom_sigma, sg, sizeof(sg), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  hipLaunchKernelGGL(k_pgo_add_batch, dim3((n_scans + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, n_scans, k0,
                     b->oa.pose + (size_t)first_scan * 7, p->n, p->e, p->x[p->cur], p->from, p->to, p->meas, p->sigma, p->robust,
                     p->odom_sigma);
  LISLAM_HIPCHK(c, hipGetLastError());
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->added[p->added_cur], b->oa.pose + (size_t)(first_scan + n_scans - 1) * 7, 7 * sizeof(double),
                                  hipMemcpyDeviceToDevice, c->stream));
  for (int k = k0; k < n_scans; k++) {
    p->h_from.push_back(p->n + k - 1);
    p->h_to.push_back(p->n + k);
  }
  p->n += n_scans;
  p->e += n_edges;
  p->adj_dirty = true;
  return LISLAM_OK;
}

namespace {

// The body of lislam_pgo_add_keyframes / lislam_pgo_add_batch_scans once the arguments are checked:
// d_pose = the trajectory on the device (null: stage pose7 first), index = the host list.
int add_keyframes(lislam_pgo* p, const char* who, const double* d_pose, const double* pose7, int n_poses, const int32_t* index,
                  int n, const double* var6) {
  lislam_ctx* c = p->ctx;
  const int k0 = p->n > 0 ? 0 : 1;
  const int n_edges = n - k0;
  if ((int64_t)p->n + n > p->ncap || (int64_t)p->e + n_edges > p->ecap)
    return fail(c, LISLAM_ERR_CAPACITY, "%s: %d + %d nodes / %d + %d edges exceed the capacity %d / %d", who, p->n, n, p->e,
                n_edges, p->ncap, p->ecap);
  hipSetDevice(c->device);
  const size_t staged = d_pose ? 0 : (size_t)n_poses * 7 * sizeof(double);
  const size_t want = staged + (size_t)n * sizeof(int);
  LISLAM_HIPCHK(c, p->kstage.reserve(want, c->stream));
  int* d_index = reinterpret_cast<int*>(p->kstage.as<char>() + staged);
  double sg[6];
  for (int k = 0; k < 6; k++) sg[k] = std::sqrt(var6 ? var6[k] : kOdometryVariances[k]);
  if (!d_pose) {
    LISLAM_HIPCHK(c, hipMemcpyAsync(p->kstage.p, pose7, staged, hipMemcpyDefault, c->stream));
    d_pose = p->kstage.as<const double>();
  }
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_index, index, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->odom_sigma, sg, sizeof(sg), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));  // sg leaves scope
  hipLaunchKernelGGL(k_pgo_add_keyframes, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, n, k0, d_pose,
                     d_index, p->added[p->added_cur], p->added[p->added_cur ^ 1], p->n, p->e, p->x[p->cur], p->from, p->to,
                     p->meas, p->sigma, p->robust, p->odom_sigma);
  LISLAM_HIPCHK(c, hipGetLastError());
  p->added_cur ^= 1;
  for (int k = k0; k < n; k++) {
    p->h_from.push_back(p->n + k - 1);
    p->h_to.push_back(p->n + k);
  }
  p->n += n;
  p->e += n_edges;
  p->adj_dirty = true;
  return LISLAM_OK;
}

}  // namespace

int lislam_pgo_add_keyframes(lislam_pgo* p, const double* pose7, int32_t n_poses, const int32_t* index, int32_t n,
                             const double* var6) {
  if (!p || n < 0 || n_poses < 0 || (n > 0 && (!pose7 || !index))) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (var6 && !positive(var6, 6)) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_keyframes: variances must be positive");
  LISLAM_RC(check_index(c, "lislam_pgo_add_keyframes", "index", index, n, n_poses, true));
  if (n == 0) return LISLAM_OK;
  return add_keyframes(p, "lislam_pgo_add_keyframes", nullptr, pose7, n_poses, index, n, var6);
}

int lislam_pgo_add_batch_scans(lislam_pgo* p, lislam_batch* b, const int32_t* scans, int32_t n, const double* var6) {
  if (!p || !b || n < 0 || (n > 0 && !scans)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  LISLAM_RC(check_same_context(c, "lislam_pgo_add_batch_scans", b));
  if (var6 && !positive(var6, 6)) return fail(c, LISLAM_ERR_ARG, "lislam_pgo_add_batch_scans: variances must be positive");
  if (n > 0 && b->extracted < 1)
    return fail(c, LISLAM_ERR_STATE, "lislam_pgo_add_batch_scans: extract the batch and run its odometry first");
  LISLAM_RC(check_index(c, "lislam_pgo_add_batch_scans", "scans", scans, n, b->extracted, true));
  if (n == 0) return LISLAM_OK;
  LISLAM_RC(lislam_batch_settle(b));
  return add_keyframes(p, "lislam_pgo_add_batch_scans", b->oa.pose, nullptr, b->extracted, scans, n, var6);
}

int lislam_pgo_linearize(lislam_pgo* p, double* residual, double* J_from, double* J_to, double* weight, double* cost) {
  if (!p) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  int rc;
  if (p->n == 0) return fail(c, LISLAM_ERR_STATE, "lislam_pgo_linearize: the graph is empty");
  if ((rc = ready(p, "lislam_pgo_linearize"))) return rc;
  hipSetDevice(c->device);
  const size_t E = (size_t)p->e;
  launch_linearize<kRaw>(p, p->x[p->cur]);
  hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(kThreads), 0, c->stream, p->e + 1, p->b.term, &p->d_res->cost_cur);
  LISLAM_HIPCHK(c, hipGetLastError());
  if (residual) LISLAM_HIPCHK(c, hipMemcpyAsync(residual, p->b.bt, (E + 1) * 6 * 8, hipMemcpyDeviceToHost, c->stream));
  if (J_from && E) LISLAM_HIPCHK(c, hipMemcpyAsync(J_from, p->b.Af, E * 36 * 8, hipMemcpyDeviceToHost, c->stream));
  if (J_to) LISLAM_HIPCHK(c, hipMemcpyAsync(J_to, p->b.At, (E + 1) * 36 * 8, hipMemcpyDeviceToHost, c->stream));
  if (weight) LISLAM_HIPCHK(c, hipMemcpyAsync(weight, p->b.wt, (E + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (cost) LISLAM_HIPCHK(c, hipMemcpyAsync(cost, &p->d_res->cost_cur, 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_pgo_optimize(lislam_pgo* p, int32_t* info, double* stats) {
  if (!p) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  int rc;
  if ((rc = ready(p, "lislam_pgo_optimize"))) return rc;
  int status = LISLAM_PGO_MAX_ITERATIONS, iterations = 0, accepted = 0, cg_total = 0, cg_most = 0;
  double cost0 = 0, cost = 0, lambda = p->cfg.lambda_init, relres = 0;
  if (p->n > 0) {
    hipSetDevice(c->device);
    if ((rc = sync_adjacency(p))) return rc;
    const int N = p->n, E = p->e;
    int loops = 0;  // edges off the tridiagonal: the rank of what the preconditioner leaves out is 6 per edge
    for (int k = 0; k < E; k++) loops += std::abs(p->h_from[k] - p->h_to[k]) != 1;
    const int cg_max = p->cfg.cg_max_iterations > 0 ? p->cfg.cg_max_iterations : 6 * loops + 8;
    bool relinearize = true;
    if (p->cfg.max_iterations == 0) {
      launch_linearize<kCost>(p, p->x[p->cur]);
      hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(kThreads), 0, c->stream, E + 1, p->b.term, &p->d_res->cost_cur);
      LISLAM_HIPCHK(c, hipMemcpyAsync(p->h_res, p->d_res, sizeof(Result), hipMemcpyDeviceToHost, c->stream));
      LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
      cost0 = cost = p->h_res->cost_cur;
    }
    while (iterations < p->cfg.max_iterations) {
      double* xc = p->x[p->cur];
      double* xt = p->x[p->cur ^ 1];
      if (relinearize) {
        launch_linearize<kNormal>(p, xc);
        hipLaunchKernelGGL(k_pgo_assemble, dim3((N * 48 + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, N, p->graph(),
                           p->adjacency(), p->b, p->Hd, p->U, p->g);
        hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(kThreads), 0, c->stream, E + 1, p->b.term, &p->d_res->cost_cur);
        relinearize = false;
      }
      hipLaunchKernelGGL(k_pgo_factor, dim3(1), dim3(64), 0, c->stream, N, lambda, p->Hd, p->U, p->Sinv, p->L);
      const Cg a{N, E, cg_max, lambda, p->cfg.cg_rel_tol, p->Hd, p->b.W, p->g, p->Sinv, p->L,
                 p->vec[0], p->vec[1], p->vec[2], p->vec[3], p->vec[4], p->vec[5]};
      hipLaunchKernelGGL(k_pgo_cg, dim3(1), dim3(kThreads), 0, c->stream, a, p->graph(), p->adjacency(), p->d_res);
      hipLaunchKernelGGL(k_pgo_retract, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, N, xc, p->vec[0], xt);
      launch_linearize<kCost>(p, xt);
      hipLaunchKernelGGL(k_pgo_sum, dim3(1), dim3(kThreads), 0, c->stream, E + 1, p->b.term, &p->d_res->cost_try);
      LISLAM_HIPCHK(c, hipGetLastError());
      // the iteration's one synchronisation: both costs and the CG summary
      LISLAM_HIPCHK(c, hipMemcpyAsync(p->h_res, p->d_res, sizeof(Result), hipMemcpyDeviceToHost, c->stream));
      LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
      const Result r = *p->h_res;
      if (iterations == 0) cost0 = cost = r.cost_cur;
      iterations++;
      cg_total += r.cg_iterations;
      cg_most = std::max(cg_most, r.cg_iterations);
      relres = r.cg_relres;
      if (r.cost_try < cost) {
        const double rel = (cost - r.cost_try) / cost;
        cost = r.cost_try;
        p->cur ^= 1;
        accepted++;
        lambda = std::max(lambda / 10.0, kLambdaMin);
        relinearize = true;
        if (rel < p->cfg.rel_cost_tol) { status = LISLAM_PGO_CONVERGED; break; }
      } else {
        lambda *= 10.0;
        if (lambda > kLambdaMax) { status = LISLAM_PGO_LAMBDA_LIMIT; break; }
      }
    }
  } else {
    status = LISLAM_PGO_CONVERGED;
  }
  if (info) {
    const int32_t v[8] = {status, iterations, accepted, cg_total, cg_most, p->n, p->e, 0};
    memcpy(info, v, sizeof(v));
  }
  if (stats) {
    stats[0] = cost0; stats[1] = cost; stats[2] = lambda; stats[3] = relres;
  }
  return LISLAM_OK;
}

int lislam_pgo_poses(lislam_pgo* p, int32_t first, int32_t n, double* pose7, float* pose6d) {
  if (!p || n < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (first < 0 || (int64_t)first + n > p->n)
    return fail(c, LISLAM_ERR_ARG, "lislam_pgo_poses: nodes [%d, %d + %d) out of range (size %d)", first, first, n, p->n);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const double* src = p->x[p->cur] + (size_t)first * 7;
  if (pose7) LISLAM_HIPCHK(c, hipMemcpyAsync(pose7, src, (size_t)n * 7 * 8, hipMemcpyDeviceToHost, c->stream));
  if (pose6d) {
    hipLaunchKernelGGL(k_pgo_pose6d, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, n, src, p->p6);
    LISLAM_HIPCHK(c, hipGetLastError());
    LISLAM_HIPCHK(c, hipMemcpyAsync(pose6d, p->p6, (size_t)n * 6 * 4, hipMemcpyDeviceToHost, c->stream));
  }
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

// Device-side edges of the test surface: from, to, meas (7), variances (6), robust of edges [first, first + n).
int lislam_pgo_edges(lislam_pgo* p, int32_t first, int32_t n, int32_t* from, int32_t* to, double* meas7, double* var6,
                     int32_t* robust) {
  if (!p || n < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (first < 0 || (int64_t)first + n > p->e)
    return fail(c, LISLAM_ERR_ARG, "lislam_pgo_edges: edges [%d, %d + %d) out of range (size %d)", first, first, n, p->e);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t at = (size_t)first, N = (size_t)n;
  if (from) LISLAM_HIPCHK(c, hipMemcpyAsync(from, p->from + at, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (to) LISLAM_HIPCHK(c, hipMemcpyAsync(to, p->to + at, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (robust) LISLAM_HIPCHK(c, hipMemcpyAsync(robust, p->robust + at, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (meas7) LISLAM_HIPCHK(c, hipMemcpyAsync(meas7, p->meas + at * 7, N * 7 * 8, hipMemcpyDeviceToHost, c->stream));
  if (var6) LISLAM_HIPCHK(c, hipMemcpyAsync(var6, p->sigma + at * 6, N * 6 * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  if (var6)
    for (size_t k = 0; k < N * 6; k++) var6[k] = var6[k] * var6[k];
  return LISLAM_OK;
}

}  // extern "C"
