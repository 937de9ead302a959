// Keyframe selection (lislam_keysel_*): feature_tracker::getKeyframe
// (src/intensity_feature_tracker.cpp:741-815, called at :721) behind tfBroadcast's accumulation
// T_s2m = T_s2m * T_s2s (:819), for a run of frames in one launch, the state device resident.
//
//   k_keysel   one workgroup of one wave.  Per chunk of 64 frames: the lanes turn the (q, t) rows
//              into 4x4 matrices (p2p_calculateRandT's tail, :916-925) and stage the stamps and good
//              flags, lane 0 runs the products and
//              the decisions in stream order, the lanes write the rows out.
//
// Semantics pinned here (tests/restate_keysel.py is the same text in plain Python floats):
//  * R(q) is Eigen's toRotationMatrix formula, q not normalized.
//  * The product is the literal 4x4 one, C(i,j) = ((A(i,0) B(0,j) + A(i,1) B(1,j)) + A(i,2) B(2,j)) +
//    A(i,3) B(3,j), plain double, no FMA (-ffp-contract=off), bottom rows included, every frame (the
//    identity of a skipped frame too).  Eigen's own order may differ in the last ulp.  The chain is
//    one serial dependency and stays one: a parallel scan would round differently.
//  * getKeyframe runs on good frames only (:693, :721).  Its first branch tests
//    cloudKeyPoses3D_->points.empty(), a container another thread fills (:536), so how many frames
//    take it depends on scheduling in the reference; here exactly the first good frame of the
//    selector's life takes it.
//  * Both gates are strict: time - last_time > time_interval and |p - prev_p| > distance_interval,
//    the norm as sqrt((dx dx + dy dy) + dz dz).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "lislam_batch.hpp"
#include "lislam_ctx.hpp"
#include "lislam_device.hpp"
#include "lislam_host.hpp"

namespace lislam {
namespace keysel {

constexpr int kChunk = 64;  // frames staged in LDS per pass: one per lane
constexpr int kNode = 26;   // FactorGraphNode (keyframe.h:115-121): time, id, p, prev_p, R, prev_R

struct State {
  double T[16];      // T_s2m_, row-major
  double prev_p[3];  // prev_position_
  double prev_R[9];  // prev_rotation_
  double last_time;  // last_skip_time (NaN until the first keyframe)
  int next_id;       // keyframeId_
  int have;          // the first branch has been taken
};

struct Args {
  const double* T_s2s;  // [n][7] q x,y,z,w, t
  const int* good;      // frame k is good iff good[k * good_stride] == 1
  int good_stride;
  const double* time;  // [n]
  int n;
  double time_interval, distance_interval;
  State* st;
  int* keyframe_id;  // [n]
  int* n_selected;   // [1]
  double* T_s2m;     // [n][16]
  double* node;      // [n][26], the first *n_selected rows written
};

__global__ __launch_bounds__(kChunk) void k_keysel(Args a) {
  __shared__ double Ts[kChunk][16];    // T_s2s of the chunk's frames
  __shared__ double Tm[kChunk][16];    // T_s2m after each frame
  __shared__ double prev[kChunk][12];  // prev_p, prev_R as a selected frame found them
  __shared__ double tm[kChunk];  // the chunk's stamps and good flags
  __shared__ int gd[kChunk];
  __shared__ int id[kChunk];
  __shared__ int sel[kChunk];  // the chunk's r-th selected frame
  __shared__ int n_sel;
  const int lane = threadIdx.x;
  // lane 0 carries the state in registers; the other lanes' copies are never read
  double T[16], pp[3], pR[9], last_time = 0;
  int next_id = 0, have = 0;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < 16; e++) T[e] = a.st->T[e];
#pragma unroll
    for (int e = 0; e < 3; e++) pp[e] = a.st->prev_p[e];
#pragma unroll
    for (int e = 0; e < 9; e++) pR[e] = a.st->prev_R[e];
    last_time = a.st->last_time;
    next_id = a.st->next_id;
    have = a.st->have;
  }
  int rows = 0;  // node rows written so far (uniform)
  for (int base = 0; base < a.n; base += kChunk) {
    const int m = min(kChunk, a.n - base);
    if (lane < m) {
      const double* r = a.T_s2s + (size_t)(base + lane) * 7;
      const double x = r[0], y = r[1], z = r[2], w = r[3];
      const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
      const double twx = tx * w, twy = ty * w, twz = tz * w;
      const double txx = tx * x, txy = ty * x, txz = tz * x;
      const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
      double* o = Ts[lane];
      o[0] = 1.0 - (tyy + tzz); o[1] = txy - twz;          o[2] = txz + twy;          o[3] = r[4];
      o[4] = txy + twz;          o[5] = 1.0 - (txx + tzz); o[6] = tyz - twx;          o[7] = r[5];
      o[8] = txz - twy;          o[9] = tyz + twx;          o[10] = 1.0 - (txx + tyy); o[11] = r[6];
      o[12] = 0.0;               o[13] = 0.0;               o[14] = 0.0;               o[15] = 1.0;
      tm[lane] = a.time[base + lane];
      gd[lane] = a.good[(size_t)(base + lane) * a.good_stride];
    }
    wave_lds_sync();
    if (lane == 0) {
      int cnt = 0;
      for (int f = 0; f < m; f++) {
        const double* B = Ts[f];
        double C[16];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++)
            C[i * 4 + j] = ((T[i * 4] * B[j] + T[i * 4 + 1] * B[4 + j]) + T[i * 4 + 2] * B[8 + j]) + T[i * 4 + 3] * B[12 + j];
#pragma unroll
        for (int e = 0; e < 16; e++) {
          T[e] = C[e];
          Tm[f][e] = C[e];
        }
        int out = -1;
        if (gd[f] == 1) {
          const double t = tm[f];
          bool take = !have;
          if (!take && t - last_time > a.time_interval) {
            const double dx = T[3] - pp[0], dy = T[7] - pp[1], dz = T[11] - pp[2];
            take = sqrt((dx * dx + dy * dy) + dz * dz) > a.distance_interval;
          }
          if (take) {
#pragma unroll
            for (int e = 0; e < 3; e++) prev[f][e] = pp[e];
#pragma unroll
            for (int e = 0; e < 9; e++) prev[f][3 + e] = pR[e];
#pragma unroll
            for (int e = 0; e < 3; e++) pp[e] = T[e * 4 + 3];
#pragma unroll
            for (int e = 0; e < 9; e++) pR[e] = T[(e / 3) * 4 + e % 3];
            out = next_id;
            sel[cnt] = f;
            cnt = cnt + 1;
            next_id = next_id + 1;
            last_time = t;
            have = 1;
          }
        }
        id[f] = out;
      }
      n_sel = cnt;
    }
    wave_lds_sync();
    if (lane < m) a.keyframe_id[base + lane] = id[lane];
    if (a.T_s2m) {
      const double* src = &Tm[0][0];
      double* dst = a.T_s2m + (size_t)base * 16;
      for (int i = lane; i < m * 16; i += kChunk) dst[i] = src[i];
    }
    const int cnt = n_sel;
    if (a.node) {
      double* dst = a.node + (size_t)rows * kNode;
      for (int i = lane; i < cnt * kNode; i += kChunk) {
        const int r = i / kNode, e = i - r * kNode, f = sel[r];
        double v;
        if (e == 0) v = tm[f];
        else if (e == 1) v = (double)id[f];
        else if (e < 5) v = Tm[f][(e - 2) * 4 + 3];
        else if (e < 8) v = prev[f][e - 5];
        else if (e < 17) v = Tm[f][((e - 8) / 3) * 4 + (e - 8) % 3];
        else v = prev[f][3 + (e - 17)];
        dst[i] = v;
      }
    }
    rows += cnt;
    wave_lds_sync();  // the next chunk overwrites the staging
  }
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < 16; e++) a.st->T[e] = T[e];
#pragma unroll
    for (int e = 0; e < 3; e++) a.st->prev_p[e] = pp[e];
#pragma unroll
    for (int e = 0; e < 9; e++) a.st->prev_R[e] = pR[e];
    a.st->last_time = last_time;
    a.st->next_id = next_id;
    a.st->have = have;
    *a.n_selected = rows;
  }
}

}  // namespace keysel
}  // namespace lislam

using namespace lislam::keysel;
using lislam::DBuf;
using lislam::fail;

struct lislam_keysel {
  lislam_ctx* ctx = nullptr;
  lislam_keysel_config cfg{};
  State* st = nullptr;
  // grow-only staging: [T_s2s n x 7][time n][good n] in, [T_s2m n x 16][node n x 26][id n][n_selected] out
  DBuf in, out;
};

namespace {

void free_keysel(lislam_keysel* s) {
  if (s->st) (void)hipFree(s->st);
  delete s;
}

// The launch over n > 0 frames whose T_s2s / good lie on the device, and the copies back.
int run(lislam_keysel* s, const double* d_T, const int* d_good, int good_stride, const double* d_time, int n,
        int32_t* keyframe_id, int32_t* n_selected, double* T_s2m, double* node) {
  lislam_ctx* c = s->ctx;
  const size_t N = (size_t)n;
  LISLAM_HIPCHK(c, s->out.reserve(N * (16 + kNode) * 8 + (N + 1) * 4, c->stream));
  double* d_Tm = s->out.as<double>();
  double* d_node = d_Tm + N * 16;
  int* d_id = reinterpret_cast<int*>(d_node + N * kNode);
  int* d_nsel = d_id + N;
  const Args a{d_T, d_good, good_stride, d_time, n, s->cfg.time_interval, s->cfg.distance_interval, s->st, d_id, d_nsel,
               T_s2m ? d_Tm : nullptr, node ? d_node : nullptr};
  hipLaunchKernelGGL(k_keysel, dim3(1), dim3(kChunk), 0, c->stream, a);
  LISLAM_HIPCHK(c, hipGetLastError());
  int nsel = 0;
  if (keyframe_id) LISLAM_HIPCHK(c, hipMemcpyAsync(keyframe_id, d_id, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (T_s2m) LISLAM_HIPCHK(c, hipMemcpyAsync(T_s2m, d_Tm, N * 16 * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(&nsel, d_nsel, 4, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_selected) *n_selected = nsel;
  if (node && nsel > 0) {
    LISLAM_HIPCHK(c, hipMemcpyAsync(node, d_node, (size_t)nsel * kNode * 8, hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return LISLAM_OK;
}

}  // namespace

extern "C" {

int lislam_keysel_create(lislam_ctx* c, const lislam_keysel_config* cfg, lislam_keysel** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  lislam_keysel_config d = {0.3, 0.3};  // config/spot.yaml:35-36
  if (cfg) d = *cfg;
  if (std::isnan(d.time_interval) || std::isnan(d.distance_interval))
    return fail(c, LISLAM_ERR_ARG, "lislam_keysel_create: the intervals must be numbers");
  hipSetDevice(c->device);
  lislam_keysel* s = new lislam_keysel();
  s->ctx = c;
  s->cfg = d;
  State h{};  // ctor :31-37: prev_p = 0, prev_R = 0, keyframeId_ = 0
  h.T[0] = h.T[5] = h.T[10] = h.T[15] = 1.0;
  h.last_time = std::numeric_limits<double>::quiet_NaN();
  if (hipMalloc(reinterpret_cast<void**>(&s->st), sizeof(State)) != hipSuccess ||
      hipMemcpyAsync(s->st, &h, sizeof(State), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {  // h leaves scope
    (void)hipGetLastError();
    free_keysel(s);
    return fail(c, LISLAM_ERR_DEVICE, "lislam_keysel_create: device allocation failed");
  }
  *out = s;
  return LISLAM_OK;
}

int lislam_keysel_destroy(lislam_keysel* s) {
  if (!s) return LISLAM_ERR_ARG;
  hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  free_keysel(s);
  return LISLAM_OK;
}

int lislam_keysel_step(lislam_keysel* s, const double* T_s2s, const int32_t* good, const double* time, int32_t n,
                       int32_t* keyframe_id, int32_t* n_selected, double* T_s2m, double* node) {
  if (!s || n < 0 || (n > 0 && (!T_s2s || !good || !time))) return LISLAM_ERR_ARG;
  lislam_ctx* c = s->ctx;
  if (n == 0) {
    if (n_selected) *n_selected = 0;
    return LISLAM_OK;
  }
  hipSetDevice(c->device);
  const size_t N = (size_t)n;
  LISLAM_HIPCHK(c, s->in.reserve(N * 8 * 8 + N * 4, c->stream));
  double* d_T = s->in.as<double>();
  double* d_time = d_T + N * 7;
  int* d_good = reinterpret_cast<int*>(d_time + N);
  // pageable sources: these copies have read them when they return
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_T, T_s2s, N * 7 * 8, hipMemcpyDefault, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_good, good, N * 4, hipMemcpyDefault, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_time, time, N * 8, hipMemcpyHostToDevice, c->stream));
  return run(s, d_T, d_good, 1, d_time, n, keyframe_id, n_selected, T_s2m, node);
}

int lislam_keysel_step_batch(lislam_keysel* s, lislam_batch* b, int32_t first_scan, int32_t n_scans, const double* time,
                             int32_t* keyframe_id, int32_t* n_selected, double* T_s2m, double* node) {
  if (!s || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = s->ctx;
  const char* who = "lislam_keysel_step_batch";
  LISLAM_RC(lislam::check_same_context(c, who, b));
  LISLAM_RC(lislam::check_scan_range(c, who, b, first_scan, n_scans));
  if (n_scans > 0 && !time) return fail(c, LISLAM_ERR_ARG, "lislam_keysel_step_batch: null time");
  lislam::OrbDescriptors o;  // not read: the call settles a device-decided cascade, whose verdict is final after it
  LISLAM_RC(lislam::orb_descriptors(c, who, b, first_scan + n_scans, &o));
  if (n_scans == 0) {
    if (n_selected) *n_selected = 0;
    return LISLAM_OK;
  }
  const void *src_T = nullptr, *src_S = nullptr;
  int cnt = 0;
  size_t esz = 0;
  LISLAM_RC(lislam_orb_batch_output(b, LISLAM_OUT_ORB_T, first_scan, &src_T, &cnt, &esz));
  LISLAM_RC(lislam_orb_batch_output(b, LISLAM_OUT_ORB_STATS, first_scan, &src_S, &cnt, &esz));
  hipSetDevice(c->device);
  const size_t N = (size_t)n_scans;
  LISLAM_HIPCHK(c, s->in.reserve(N * 8 * 8 + N * 4, c->stream));
  double* d_time = s->in.as<double>() + N * 7;
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_time, time, N * 8, hipMemcpyHostToDevice, c->stream));
  return run(s, static_cast<const double*>(src_T), static_cast<const int*>(src_S), 8, d_time, n_scans, keyframe_id, n_selected,
             T_s2m, node);
}

int lislam_keysel_state(lislam_keysel* s, int32_t* n_keyframes, double* T_s2m16, double* last_time) {
  if (!s) return LISLAM_ERR_ARG;
  lislam_ctx* c = s->ctx;
  hipSetDevice(c->device);
  State h;
  LISLAM_HIPCHK(c, hipMemcpyAsync(&h, s->st, sizeof(State), hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_keyframes) *n_keyframes = h.next_id;
  if (T_s2m16) std::copy(h.T, h.T + 16, T_s2m16);
  if (last_time) *last_time = h.last_time;
  return LISLAM_OK;
}

}  // extern "C"
