// mapOptimization's ORB keyframe sliding window on the GPU (keyframe_sliding_window_,
// src/mapOptimization.cpp:155-169, :295-361, :481-493).
//
// The window is a ring of window_size + 1 keyframe slots in HBM (descriptors, sensor-frame points,
// pose): the current keyframe is staged into the free slot, matched from there against every live
// slot, and a push only stores its pose and advances the ring.
//
// Kernels, one launch each for the whole window:
//   k_mw_match   per (window keyframe, 64 queries, 256 trains): cv::BFMatcher(NORM_L2) — the exact
//                integer sum of squared byte differences of every (query, train) pair, the best
//                per query kept with a 64-bit atomicMin of (sum << 12 | train index), so equal sums
//                resolve to the lowest train index whatever order the train tiles finish in
//   k_mw_select  per window keyframe: the M > 100 test, std::sort of the matches as a bitonic
//                sort of the unique keys (sum << 12 | query index) in LDS, G in double, the :327
//                conditions
//   k_mw_gate    one workgroup: the fp64 map-frame transforms, the 0.3 m gate and the order-
//                preserving compaction into kind-3 records, window keyframes newest to oldest
//   k_mw_append  the ground-plane records behind the feature records (one problem, :354 / :424)
//
// L2 on the vector ALU, not the int8 matrix cores: with unsigned bytes
// sum (a - b)^2 = sum a^2 + sum b^2 - 2 a.b and a.b is 8 v_dot4_u32_u8 per pair, exact in 32
// bits (<= 32 * 255^2 = 2,080,800).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "lislam_device.hpp"
#include "lislam_host.hpp"
#include "lislam_mapwin.hpp"

namespace lislam {
namespace mapwin {

constexpr int kQTile = 64;   // queries per workgroup: one per lane
constexpr int kTTile = 256;  // trains per workgroup: 64 per wave
constexpr int kSelThreads = 1024;
constexpr int kGateThreads = 1024;  // >= kMaxKeep: one match per thread
constexpr unsigned long long kNoMatch = ~0ull;

struct View {
  const uint8_t* desc;  // [slots][cap][32]
  const float4* p3d;    // [slots][cap]
  const double* pose;   // [slots][8]
  int cap, nw, qslot, nq;
  int slot[kMaxWindow], nt[kMaxWindow];  // newest first
};

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {
#if __has_builtin(__builtin_amdgcn_udot4)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else  // the host pass of this file, which has no such builtin
  for (int k = 0; k < 4; k++) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
  return c;
#endif
}
__device__ __forceinline__ uint32_t dot32(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  uint32_t d = dot4(a0.x, b0.x, 0u);
  d = dot4(a0.y, b0.y, d); d = dot4(a0.z, b0.z, d); d = dot4(a0.w, b0.w, d);
  d = dot4(a1.x, b1.x, d); d = dot4(a1.y, b1.y, d); d = dot4(a1.z, b1.z, d); d = dot4(a1.w, b1.w, d);
  return d;
}

// best[w][q] = min over trains j of (sum_i (a_i - b_i)^2 << 12 | j); best is kNoMatch beforehand.
// Every lane of a wave reads the same train row from LDS (a broadcast), its own query from registers.
__global__ __launch_bounds__(kTTile) void k_mw_match(View v, unsigned long long* best) {
  __shared__ uint4 tr[kTTile][2];
  __shared__ uint32_t tn[kTTile];
  const int w = blockIdx.z, nt = v.nt[w], t0 = blockIdx.y * kTTile;
  if (t0 >= nt) return;
  {
    const uint4* T = reinterpret_cast<const uint4*>(v.desc + (size_t)v.slot[w] * v.cap * 32);
    const int j = t0 + threadIdx.x;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (j < nt) { a = T[2 * (size_t)j]; b = T[2 * (size_t)j + 1]; }
    tr[threadIdx.x][0] = a;
    tr[threadIdx.x][1] = b;
    tn[threadIdx.x] = dot32(a, b, a, b);
  }
  __syncthreads();
  const int q = blockIdx.x * kQTile + (threadIdx.x & 63), sub = threadIdx.x >> 6;
  if (q >= v.nq) return;
  const uint4* Q = reinterpret_cast<const uint4*>(v.desc + (size_t)v.qslot * v.cap * 32);
  const uint4 a0 = Q[2 * (size_t)q], a1 = Q[2 * (size_t)q + 1];
  const uint32_t qn = dot32(a0, a1, a0, a1);
  const int jend = min(sub * 64 + 64, nt - t0);
  unsigned long long key = kNoMatch;
  for (int jj = sub * 64; jj < jend; jj++) {
    const uint32_t sum = qn + tn[jj] - 2u * dot32(a0, a1, tr[jj][0], tr[jj][1]);
    const unsigned long long k = (unsigned long long)sum << 12 | (unsigned)(t0 + jj);
    key = k < key ? k : key;
  }
  if (key != kNoMatch) atomicMin(best + (size_t)w * v.cap + q, key);
}

// matches[w][q] = train, sum (or -1, -1) for lislam_mapwin_match
__global__ void k_mw_export(View v, const unsigned long long* best, int* matches) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
  if (q >= v.nq) return;
  const unsigned long long k = best[(size_t)w * v.cap + q];
  int* o = matches + ((size_t)w * v.nq + q) * 2;
  o[0] = k == kNoMatch ? -1 : (int)(k & 4095u);
  o[1] = k == kNoMatch ? -1 : (int)(k >> 12);
}

// :309-327 per window keyframe.  The DMatch distance is sqrtf((float)sum): the conversion and sqrtf
// are monotone and injective on these integers (< 2^24), so sorting the integer sums is std::sort's
// order; operator< compares distances only and the keys carry the query index below the sum, which
// is the stable order (k_orb_match's convention for equal distances) — the keys are unique, so any
// sorting network gives it.  sel[w][i] = (query, train) of the i-th match, i < G.
__global__ __launch_bounds__(kSelThreads) void k_mw_select(View v, const unsigned long long* best, int2* sel, int* info) {
  __shared__ unsigned long long keys[kMaxFeatures];
  const int w = blockIdx.x, nt = v.nt[w], nq = v.nq;
  const int M = (nt > 0 && nq > 0) ? nq : 0;
  // for (size_t i = 0; i < matches.size() * 0.2; ++i): the number of integers i >= 0 below the double
  const double lim = (double)M * 0.2;
  int G = (int)lim;
  if ((double)G < lim) G++;
  const bool used = M > 100 && G > 50 && G != M && nt != nq;
  if (threadIdx.x == 0) {
    int* o = info + w * 6;
    o[0] = nt; o[1] = M; o[2] = G; o[3] = used; o[4] = 0; o[5] = 0;
  }
  if (!used) return;
  int n2 = 128;
  while (n2 < nq) n2 <<= 1;
  const unsigned long long* b = best + (size_t)w * v.cap;
  for (int i = threadIdx.x; i < n2; i += kSelThreads) keys[i] = i < nq ? ((b[i] >> 12) << 12 | (unsigned)i) : kNoMatch;
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < n2; i += kSelThreads) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long x = keys[i], y = keys[p];
          if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[p] = x; }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G; i += kSelThreads) {
    const int q = (int)(keys[i] & 4095u);
    sel[w * kMaxKeep + i] = make_int2(q, (int)(b[q] & 4095u));
  }
}

// :333-356 in the fixed block order: window keyframes newest to oldest, matches in sorted order.
// info[w][4..5] = blocks kept, offset; info[nw * 6] = the record count, [nw * 6 + 1] = keyframes used.
__global__ __launch_bounds__(kGateThreads) void k_mw_gate(View v, const int2* sel, const double* xcur, int* info, double* rec,
                                                         int* kind, int* pairs) {
  __shared__ int wcnt[kGateThreads / 64];
  const DQ qc{xcur[0], xcur[1], xcur[2], xcur[3]};
  const D3 tc{xcur[4], xcur[5], xcur[6]};
  const float4* pc = v.p3d + (size_t)v.qslot * v.cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int off = 0, nused = 0;
  for (int w = 0; w < v.nw; w++) {
    const int n = info[w * 6 + 3] ? info[w * 6 + 2] : 0;
    nused += n > 0;
    bool keep = false;
    int2 m = make_int2(0, 0);
    D3 src{0, 0, 0}, dst{0, 0, 0};
    if ((int)threadIdx.x < n) {
      m = sel[w * kMaxKeep + threadIdx.x];
      const double* xp = v.pose + (size_t)v.slot[w] * 8;
      const float4 a = v.p3d[(size_t)v.slot[w] * v.cap + m.y], c = pc[m.x];
      src = D3{(double)c.x, (double)c.y, (double)c.z};
      dst = qrot(DQ{xp[0], xp[1], xp[2], xp[3]}, D3{(double)a.x, (double)a.y, (double)a.z}) + D3{xp[4], xp[5], xp[6]};
      const D3 d = dst - (qrot(qc, src) + tc);
      keep = !(sqrt(d.x * d.x + d.y * d.y + d.z * d.z) > 0.3);
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, tot = 0;
    for (int k = 0; k < kGateThreads / 64; k++) {
      const int c = wcnt[k];
      before += k < wave ? c : 0;
      tot += c;
    }
    if (keep) {
      const int i = off + before + __popcll(bal & ((1ull << lane) - 1ull));
      double* r = rec + (size_t)i * 9;
      r[0] = src.x; r[1] = src.y; r[2] = src.z; r[3] = dst.x; r[4] = dst.y; r[5] = dst.z; r[6] = 0; r[7] = 0; r[8] = 0;
      kind[i] = 3;
      pairs[i * 3 + 0] = w; pairs[i * 3 + 1] = m.x; pairs[i * 3 + 2] = m.y;
    }
    if (threadIdx.x == 0) { info[w * 6 + 4] = tot; info[w * 6 + 5] = off; }
    off += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) { info[v.nw * 6] = off; info[v.nw * 6 + 1] = nused; }
}

// rec[nfeat + i] = plane record i (i < *ncount <= n); *total = nfeat + *ncount
__global__ void k_mw_append(const double* prec, const int* pkind, const int* ncount, int n, const int* nfeat, double* rec,
                            int* kind, int* total) {
  const int nn = ncount ? min(*ncount, n) : n, f = *nfeat;
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = f + nn;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nn * 9; e += gridDim.x * blockDim.x) {
    rec[(size_t)f * 9 + e] = prec[e];
    if (e < nn) kind[f + e] = pkind[e];
  }
}

}  // namespace mapwin
}  // namespace lislam

// ================================================================== host side
using namespace lislam::mapwin;
using namespace lislam;

struct lislam_mapwin {
  lislam_ctx* ctx = nullptr;
  int W = 0, cap = 0, slots = 1;
  int head = 0, count = 0;  // oldest live slot, live slots
  int nslot[kMaxWindow + 1] = {};
  int staged = 0;           // features in the free slot
  uint8_t* desc = nullptr;
  float4* p3d = nullptr;
  double* pose = nullptr;
  unsigned long long* best = nullptr;
  int2* sel = nullptr;
  int *info = nullptr, *pairs = nullptr, *total = nullptr;
  DBuf rec, kind;  // records of 9 doubles, their kinds
  // rows both buffers hold: read from the buffers, so a failed reallocation leaves 0
  int rec_rows() const { return (int)std::min<size_t>(std::min(rec.bytes / 72, kind.bytes / 4), INT_MAX); }
  int free_slot() const { return (head + count) % slots; }
  int frec() const { return std::max(W, 1) * kMaxKeep; }
  View view() const {
    View v{};
    v.desc = desc; v.p3d = p3d; v.pose = pose; v.cap = cap; v.nw = count; v.qslot = free_slot(); v.nq = staged;
    for (int i = 0; i < count; i++) {
      v.slot[i] = (head + count - 1 - i) % slots;
      v.nt[i] = nslot[v.slot[i]];
    }
    return v;
  }
};

namespace {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

int reserve_records(lislam_mapwin* w, int rows) {
  lislam_ctx* c = w->ctx;
  LISLAM_HIPCHK(c, w->rec.reserve((size_t)rows * 72, c->stream));
  LISLAM_HIPCHK(c, w->kind.reserve((size_t)rows * 4, c->stream));
  return LISLAM_OK;
}

// the staged keyframe against every live slot: best[w][q]
int match_device(lislam_mapwin* w) {
  lislam_ctx* c = w->ctx;
  const View v = w->view();
  if (v.nw == 0 || v.nq == 0) return LISLAM_OK;
  LISLAM_HIPCHK(c, hipMemsetAsync(w->best, 0xff, (size_t)v.nw * w->cap * 8, c->stream));
  int mt = 0;
  for (int i = 0; i < v.nw; i++) mt = std::max(mt, v.nt[i]);
  if (mt > 0) {
    TimedScope ts(c, kT_mw_match);
    hipLaunchKernelGGL(k_mw_match, dim3(cdiv(v.nq, kQTile), cdiv(mt, kTTile), v.nw), dim3(kTTile), 0, c->stream, v, w->best);
  }
  LISLAM_HIPCHK(c, hipGetLastError());
  return LISLAM_OK;
}

}  // namespace

namespace lislam {
namespace mapwin {

lislam_ctx* context(lislam_mapwin* w) { return w->ctx; }
int window_size(lislam_mapwin* w) { return w->W; }
int feature_capacity(lislam_mapwin* w) { return w->cap; }
double* rec(lislam_mapwin* w) { return w->rec.as<double>(); }
int* kind(lislam_mapwin* w) { return w->kind.as<int>(); }
int* total(lislam_mapwin* w) { return w->total; }
int* info(lislam_mapwin* w) { return w->info; }
int* pairs(lislam_mapwin* w) { return w->pairs; }
int capacity_records(lislam_mapwin* w) { return w->frec(); }

int stage(lislam_mapwin* w, const uint8_t* desc, const float* p3d, int n) {
  lislam_ctx* c = w->ctx;
  if (n < 0 || (n > 0 && (!desc || !p3d))) return LISLAM_ERR_ARG;
  if (n > w->cap) return fail(c, LISLAM_ERR_CAPACITY, "lislam_mapwin: %d features > feature_capacity %d", n, w->cap);
  if (n > 0 && desc != stage_desc(w))
    LISLAM_HIPCHK(c, hipMemcpyAsync(stage_desc(w), desc, (size_t)n * 32, hipMemcpyDefault, c->stream));
  if (n > 0 && p3d != stage_p3d(w))
    LISLAM_HIPCHK(c, hipMemcpyAsync(stage_p3d(w), p3d, (size_t)n * 16, hipMemcpyDefault, c->stream));
  w->staged = n;
  return LISLAM_OK;
}

uint8_t* stage_desc(lislam_mapwin* w) { return w->desc + (size_t)w->free_slot() * w->cap * 32; }
float* stage_p3d(lislam_mapwin* w) { return reinterpret_cast<float*>(w->p3d + (size_t)w->free_slot() * w->cap); }

int records(lislam_mapwin* w, const double* pose, int plane_cap) {
  lislam_ctx* c = w->ctx;
  hipStream_t st = c->stream;
  LISLAM_RC(reserve_records(w, w->frec() + std::max(plane_cap, 0)));
  const View v = w->view();
  LISLAM_HIPCHK(c, hipMemsetAsync(w->info, 0, (size_t)(kMaxWindow * 6 + 2) * 4, st));
  if (v.nw == 0) return LISLAM_OK;
  LISLAM_RC(match_device(w));
  {
    TimedScope ts(c, kT_mw_select);
    hipLaunchKernelGGL(k_mw_select, dim3(v.nw), dim3(kSelThreads), 0, st, v, w->best, w->sel, w->info);
  }
  {
    TimedScope ts(c, kT_mw_gate);
    hipLaunchKernelGGL(k_mw_gate, dim3(1), dim3(kGateThreads), 0, st, v, w->sel, pose, w->info, w->rec.as<double>(), w->kind.as<int>(),
                       w->pairs);
  }
  LISLAM_HIPCHK(c, hipGetLastError());
  return LISLAM_OK;
}

int append(lislam_mapwin* w, const double* prec, const int* pkind, const int* ncount, int n) {
  lislam_ctx* c = w->ctx;
  if (w->frec() + n > w->rec_rows()) return fail(c, LISLAM_ERR_STATE, "lislam_mapwin: plane records beyond the reserved rows");
  hipLaunchKernelGGL(k_mw_append, dim3(std::max(1, std::min(cdiv(n * 9, 256), 1024))), dim3(256), 0, c->stream, prec, pkind,
                     ncount, n, w->info + w->count * 6, w->rec.as<double>(), w->kind.as<int>(), w->total);
  LISLAM_HIPCHK(c, hipGetLastError());
  return LISLAM_OK;
}

int push_staged(lislam_mapwin* w, const double* pose) {
  lislam_ctx* c = w->ctx;
  const int s = w->free_slot();
  LISLAM_HIPCHK(c, hipMemcpyAsync(w->pose + (size_t)s * 8, pose, 56, hipMemcpyDefault, c->stream));
  w->nslot[s] = w->staged;
  w->staged = 0;
  w->count++;
  if (w->count > w->W) {  // pop_front
    w->head = (w->head + 1) % w->slots;
    w->count--;
  }
  return LISLAM_OK;
}

}  // namespace mapwin
}  // namespace lislam

extern "C" {

int lislam_mapwin_create(lislam_ctx* c, int32_t window_size, int32_t feature_capacity, lislam_mapwin** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  if (window_size < 0 || window_size > kMaxWindow || feature_capacity < 1 || feature_capacity > kMaxFeatures)
    return fail(c, LISLAM_ERR_ARG, "lislam_mapwin_create: window_size 0..%d, feature_capacity 1..%d", kMaxWindow, kMaxFeatures);
  hipSetDevice(c->device);
  lislam_mapwin* w = new lislam_mapwin();
  w->ctx = c;
  w->W = window_size;
  w->cap = feature_capacity;
  w->slots = window_size + 1;
  const int nw = std::max(window_size, 1);
  hipError_t e = hipMalloc(&w->desc, (size_t)w->slots * w->cap * 32);
  if (e == hipSuccess) e = hipMalloc(&w->p3d, (size_t)w->slots * w->cap * 16);
  if (e == hipSuccess) e = hipMalloc(&w->pose, (size_t)(w->slots + 1) * 64)  /* + a row for lislam_mapwin_records' pose */;
  if (e == hipSuccess) e = hipMalloc(&w->best, (size_t)nw * w->cap * 8);
  if (e == hipSuccess) e = hipMalloc(&w->sel, (size_t)nw * kMaxKeep * 8);
  if (e == hipSuccess) e = hipMalloc(&w->info, (size_t)(kMaxWindow * 6 + 2) * 4);
  if (e == hipSuccess) e = hipMalloc(&w->pairs, (size_t)nw * kMaxKeep * 12);
  if (e == hipSuccess) e = hipMalloc(&w->total, 4);
  if (e == hipSuccess) e = hipMemsetAsync(w->info, 0, (size_t)(kMaxWindow * 6 + 2) * 4, c->stream);
  if (e != hipSuccess) {
    lislam_mapwin_destroy(w);
    return fail(c, LISLAM_ERR_DEVICE, "lislam_mapwin_create: %s", hipGetErrorString(e));
  }
  *out = w;
  return LISLAM_OK;
}

int lislam_mapwin_destroy(lislam_mapwin* w) {
  if (!w) return LISLAM_OK;
  hipSetDevice(w->ctx->device);
  (void)hipStreamSynchronize(w->ctx->stream);
  for (void* p : {(void*)w->desc, (void*)w->p3d, (void*)w->pose, (void*)w->best, (void*)w->sel, (void*)w->info,
                  (void*)w->pairs, (void*)w->total})
    if (p) (void)hipFree(p);
  delete w;
  return LISLAM_OK;
}

int lislam_mapwin_size(lislam_mapwin* w, int32_t* n) {
  if (!w || !n) return LISLAM_ERR_ARG;
  *n = w->count;
  return LISLAM_OK;
}

int lislam_mapwin_push(lislam_mapwin* w, const uint8_t* desc, const float* p3d, int32_t n, const double* pose) {
  if (!w || !pose) return LISLAM_ERR_ARG;
  hipSetDevice(w->ctx->device);
  LISLAM_RC(stage(w, desc, p3d, n));
  LISLAM_RC(push_staged(w, pose));
  LISLAM_HIPCHK(w->ctx, hipStreamSynchronize(w->ctx->stream));
  return LISLAM_OK;
}

int lislam_mapwin_keyframe(lislam_mapwin* w, int32_t index, uint8_t* desc, float* p3d, int32_t cap, int32_t* n,
                           double* pose) {
  if (!w || !n || index < 0 || index >= w->count || cap < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = w->ctx;
  hipSetDevice(c->device);
  const int s = (w->head + index) % w->slots, cnt = w->nslot[s];
  *n = cnt;
  if ((desc || p3d) && cnt > cap) return fail(c, LISLAM_ERR_CAPACITY, "lislam_mapwin_keyframe: %d features > cap %d", cnt, cap);
  if (desc && cnt) LISLAM_HIPCHK(c, hipMemcpyAsync(desc, w->desc + (size_t)s * w->cap * 32, (size_t)cnt * 32, hipMemcpyDefault, c->stream));
  if (p3d && cnt) LISLAM_HIPCHK(c, hipMemcpyAsync(p3d, w->p3d + (size_t)s * w->cap, (size_t)cnt * 16, hipMemcpyDefault, c->stream));
  if (pose) LISLAM_HIPCHK(c, hipMemcpyAsync(pose, w->pose + (size_t)s * 8, 56, hipMemcpyDefault, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_mapwin_match(lislam_mapwin* w, const uint8_t* desc, int32_t n, int32_t* matches) {
  if (!w || n < 0 || (n > 0 && !desc) || (n > 0 && w->count > 0 && !matches)) return LISLAM_ERR_ARG;
  lislam_ctx* c = w->ctx;
  hipSetDevice(c->device);
  if (n > w->cap) return fail(c, LISLAM_ERR_CAPACITY, "lislam_mapwin_match: %d features > feature_capacity %d", n, w->cap);
  if (n == 0 || w->count == 0) return LISLAM_OK;
  hipStream_t st = c->stream;
  LISLAM_HIPCHK(c, hipMemcpyAsync(w->desc + (size_t)w->free_slot() * w->cap * 32, desc, (size_t)n * 32, hipMemcpyDefault, st));
  w->staged = n;
  LISLAM_RC(match_device(w));
  int* dm = nullptr;
  LISLAM_HIPCHK(c, hipMalloc(&dm, (size_t)w->count * n * 8));
  const View v = w->view();
  hipLaunchKernelGGL(k_mw_export, dim3(cdiv(n, 256), v.nw), dim3(256), 0, st, v, w->best, dm);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(matches, dm, (size_t)w->count * n * 8, hipMemcpyDefault, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(dm);
  w->staged = 0;
  LISLAM_HIPCHK(c, e);
  return LISLAM_OK;
}

int lislam_mapwin_records(lislam_mapwin* w, const uint8_t* desc, const float* p3d, int32_t n, const double* pose,
                          double* rec, int32_t cap, int32_t* n_rec, int32_t* info, int32_t* pairs) {
  if (!w || !pose || !n_rec || cap < 0 || (cap > 0 && !rec)) return LISLAM_ERR_ARG;
  lislam_ctx* c = w->ctx;
  hipSetDevice(c->device);
  hipStream_t st = c->stream;
  LISLAM_RC(stage(w, desc, p3d, n));
  double* dpose = w->pose + (size_t)w->slots * 8;
  int hi[kMaxWindow * 6 + 2];
  hipError_t e = hipMemcpyAsync(dpose, pose, 56, hipMemcpyDefault, st);
  int rc = e == hipSuccess ? records(w, dpose, 0) : LISLAM_OK;
  if (e == hipSuccess && rc == LISLAM_OK) e = hipMemcpyAsync(hi, w->info, sizeof(hi), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  w->staged = 0;
  LISLAM_HIPCHK(c, e);
  LISLAM_RC(rc);
  const int nr = hi[w->count * 6];
  *n_rec = nr;
  if (info)
    for (int i = 0; i < w->W * 6; i++) info[i] = i < w->count * 6 ? hi[i] : 0;
  if (nr > cap) return fail(c, LISLAM_ERR_CAPACITY, "lislam_mapwin_records: %d records > cap %d", nr, cap);
  if (nr) {
    LISLAM_HIPCHK(c, hipMemcpyAsync(rec, w->rec.p, (size_t)nr * 72, hipMemcpyDefault, st));
    if (pairs) LISLAM_HIPCHK(c, hipMemcpyAsync(pairs, w->pairs, (size_t)nr * 12, hipMemcpyDefault, st));
    LISLAM_HIPCHK(c, hipStreamSynchronize(st));
  }
  return LISLAM_OK;
}

}  // extern "C"
