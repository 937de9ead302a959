// Scan Context place recognition (lislam_place_*): the reference's SCManager
// (include/Scancontext.h, src/Scancontext.cpp) as a device-resident database.
//
//   k_sc_describe   makeScancontext (:160-204): scatter-max of the points of many clouds into
//                   their ring x sector grids
//   k_sc_finish     the NO_POINT -> 0 rule, makeRingkeyFromScancontext (:206-219),
//                   makeSectorkeyFromScancontext (:222-235) and the column norms distDirectSC uses
//   k_sc_detect     detectLoopClosureID (:253-344) of many queries, each against the prefix of ring
//                   keys its tree held when that keyframe was the newest
//   k_sc_distance   distanceBtnScanContext (:126-157) of arbitrary pairs (the routine k_sc_detect uses)
//
// Semantics pinned here (tests/restate_sc.py is the same text in numpy):
//  * Dropout points.  cloud_track holds (0, 0, 0, .) for every dropped return.  xy2theta gives
//    0 / 0 = NaN there and int(ceil(NaN)) is INT_MIN on the reference's x86-64 build, so the sector
//    index clamps to 1; the range is 0, so the ring index is 1: every cloud with a dropout has
//    desc(0, 0) >= lidar_height.  Kept.
//  * NaN coordinates.  A point whose x or y is NaN takes none of xy2theta's four branches; the
//    reference falls off the function's end (undefined).  Such a point is skipped: the one deviation.
//  * NaN height.  `desc < pt.z` is false for a NaN pt.z, so it never wins; it is dropped before the
//    integer-keyed maximum (whose order would put it above every number).
//  * The maximum is taken over order-preserving integer keys of the float height, so it does not
//    depend on the order the points arrive in.  A zero height is stored as +0.0 (the reference keeps
//    whichever sign came first; no later expression tells them apart).
//  * Dot products, norms and the sums over columns run in one fixed order (sequential in the ring
//    index inside a column, sequential in the sector index across columns), plain double, no FMA
//    (-ffp-contract=off).  Eigen's vectorized order in the reference may differ in the last ulp.
//  * The candidates are the exact num_candidates nearest ring keys in nanoflann's float metric
//    (L2_Adaptor::evalMetric, nanoflann.hpp:383-408), equal distances by lower index; nanoflann's
//    order among equals is its tree's traversal order.
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
namespace place {

constexpr int kMaxRing = 40, kMaxSector = 120, kMaxCand = 32;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPointsPerBlock = 8192;  // 32 points per thread between the LDS grid's fill and flush
constexpr float kNoPoint = -1000.0f;   // NO_POINT (:167)
constexpr double kFar = 10000000.0;    // the initial minimum of every search (:107, :144, :284)

struct Params {
  double lidar_height, max_radius, search_ratio, dist_thres;
  int R, S, E, K, P;
};

// Order-preserving key of a float (not NaN): a < b  <=>  key(a) < key(b).
__host__ __device__ inline uint32_t height_key(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_height(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// max(min(n, int(ceil(v))), 1) with the x86-64 conversion of a NaN (INT_MIN, so 1).  v is at most n
// for every point that passed the range test, so no other value leaves the int range.
__device__ __forceinline__ int bin_index(double v, int n) {
  const double c = ceil(v);
  if (!(c >= 1.0)) return 1;  // NaN included
  return c >= (double)n ? n : (int)c;
}

// xy2theta (:25-42): the branches in the source's order (-0.0 counts as >= 0), the quotient in
// float, atan and the scaling by 180 / M_PI in double, the result narrowed to float on return.
// false: x or y is NaN (no branch taken).
__device__ __forceinline__ bool xy2theta(float x, float y, float* out) {
  const double k = 180 / kPi;
  double a;
  if ((x >= 0) & (y >= 0)) a = k * atan((double)(y / x));
  else if ((x < 0) & (y >= 0)) a = 180 - (k * atan((double)(y / (-x))));
  else if ((x < 0) & (y < 0)) a = 180 + (k * atan((double)(y / x)));
  else if ((x >= 0) & (y < 0)) a = 360 - (k * atan((double)((-y) / x)));
  else return false;
  *out = (float)a;
  return true;
}

// Clouds of one launch: cloud c holds cnt points from pts + off, with (off, cnt) = (offsets[c],
// counts[c]) for a packed array or (c * stride, stride) for the scans of a batch.
struct Clouds {
  const float4* pts;
  const long long* offsets;  // null: uniform
  const int* counts;
  int stride;
  int blocks_per_cloud;
};

__global__ __launch_bounds__(kThreads) void k_sc_describe(Clouds cl, Params P, uint32_t* __restrict__ keys /*[n][R*S]*/) {
  __shared__ uint32_t grid[kMaxRing * kMaxSector];
  const int c = blockIdx.x / cl.blocks_per_cloud, part = blockIdx.x % cl.blocks_per_cloud;
  const int n = cl.offsets ? cl.counts[c] : cl.stride;
  const long long off = cl.offsets ? cl.offsets[c] : (long long)c * cl.stride;
  if (part * kThreads >= n) return;  // nothing for this part (uniform over the workgroup)
  const int bins = P.R * P.S;
  const uint32_t empty = height_key(kNoPoint);
  for (int b = threadIdx.x; b < bins; b += kThreads) grid[b] = empty;
  __syncthreads();
  const float4* pts = cl.pts + off;
  // the parts of a cloud interleave by workgroup-sized runs, so every wave reads 1 KB at a time
  for (int i = part * kThreads + threadIdx.x; i < n; i += cl.blocks_per_cloud * kThreads) {
    const float4 p = ldg(pts + i);
    float pz = (float)((double)p.z + P.lidar_height);
    const float range = sqrtf(p.x * p.x + p.y * p.y);
    float angle;
    if (!xy2theta(p.x, p.y, &angle)) continue;  // NaN x or y
    if ((double)range > P.max_radius) continue;
    if (pz != pz) continue;  // a NaN height never wins
    if (pz == 0.0f) pz = 0.0f;  // -0.0 -> +0.0
    const int ring = bin_index((double)range / P.max_radius * P.R, P.R);
    const int sector = bin_index((double)angle / 360.0 * P.S, P.S);
    const int b = (ring - 1) * P.S + (sector - 1);
    const uint32_t k = height_key(pz);
    if (k > grid[b]) atomicMax(&grid[b], k);  // the plain read only spares atomics: a maximum only grows
  }
  __syncthreads();
  uint32_t* out = keys + (size_t)c * bins;
  for (int b = threadIdx.x; b < bins; b += kThreads)
    if (grid[b] != empty) atomicMax(out + b, grid[b]);
}

__global__ __launch_bounds__(kThreads) void k_sc_finish(Params P, int first, const uint32_t* __restrict__ keys,
                                                        double* __restrict__ desc, float* __restrict__ rkey,
                                                        double* __restrict__ skey, double* __restrict__ cnorm) {
  __shared__ double d[kMaxRing * kMaxSector];
  const int e = first + blockIdx.x, bins = P.R * P.S;
  const uint32_t* k = keys + (size_t)e * bins;
  double* out = desc + (size_t)e * bins;
  for (int b = threadIdx.x; b < bins; b += kThreads) {
    const float h = key_height(k[b]);
    const double v = (h == kNoPoint) ? 0.0 : (double)h;
    d[b] = v;
    out[b] = v;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < P.R + P.S; t += kThreads) {
    if (t < P.R) {  // curr_row.mean(), narrowed to float by eig2stdvec
      double s = 0;
      for (int j = 0; j < P.S; j++) s = s + d[t * P.S + j];
      rkey[(size_t)e * P.R + t] = (float)(s / (double)P.S);
    } else {  // curr_col.mean() and the column's norm
      const int j = t - P.R;
      double s = 0, q = 0;
      for (int r = 0; r < P.R; r++) {
        const double v = d[r * P.S + j];
        s = s + v;
        q = q + v * v;
      }
      skey[(size_t)e * P.S + j] = s / (double)P.R;
      cnorm[(size_t)e * P.S + j] = sqrt(q);
    }
  }
}

struct Db {
  const double* desc;   // [n][R*S]
  const float* rkey;    // [n][R]
  const double* skey;   // [n][S]
  const double* cnorm;  // [n][S]
};

// distanceBtnScanContext(desc[a], desc[b]) by one wave; every lane returns the same (dist, shift).
// tmp: S doubles of LDS owned by this wave.
__device__ void pair_distance(const Params& P, const Db& db, int a, int b, double* tmp, double* dist_out, int* shift_out) {
  const int lane = lane_id(), S = P.S, R = P.R;
  const double* v1 = db.skey + (size_t)a * S;
  const double* v2 = db.skey + (size_t)b * S;
  // fastAlignUsingVkey: the norm of vkey1 - circshift(vkey2, s) for every s, then a strict < scan
  for (int s = lane; s < S; s += 64) {
    double q = 0;
    for (int j = 0; j < S; j++) {
      int src = j - s;
      if (src < 0) src += S;
      const double df = v1[j] - v2[src];
      q = q + df * df;
    }
    tmp[s] = sqrt(q);
  }
  wave_lds_sync();
  int argmin = 0;
  double best = kFar;
  for (int s = 0; s < S; s++) {
    const double v = tmp[s];
    if (v < best) { best = v; argmin = s; }
  }
  wave_lds_sync();
  const int radius = (int)round(0.5 * P.search_ratio * S);
  const double* d1 = db.desc + (size_t)a * R * S;
  const double* d2 = db.desc + (size_t)b * R * S;
  const double* n1 = db.cnorm + (size_t)a * S;
  const double* n2 = db.cnorm + (size_t)b * S;
  // the sorted shift set {argmin, argmin +- 1 .. radius} mod S, ascending; its duplicates change nothing
  int arg = 0;
  double mind = kFar;
  for (int s = 0; s < S; s++) {
    int dd = s - argmin;
    if (dd < 0) dd += S;
    if (!(dd <= radius || S - dd <= radius)) continue;
    // distDirectSC against circshift(sc2, s): column j of sc2_shifted is column j - s of sc2
    uint64_t counted[2] = {0, 0};  // columns where neither norm is 0 (S <= 128)
    for (int t = 0; t < 2; t++) {
      const int j = lane + 64 * t;
      bool use = false;
      if (j < S) {
        int src = j - s;
        if (src < 0) src += S;
        const double na = n1[j], nb = n2[src];
        use = !(na == 0 || nb == 0);
        if (use) {
          double dot = 0;
          for (int r = 0; r < R; r++) dot = dot + d1[r * S + j] * d2[r * S + src];
          tmp[j] = dot / (na * nb);
        }
      }
      counted[t] = __ballot(use);
    }
    wave_lds_sync();
    double sum = 0;
    int cols = 0;
    for (int j = 0; j < S; j++) {
      if (!((counted[j >> 6] >> (j & 63)) & 1)) continue;
      sum = sum + tmp[j];
      cols = cols + 1;
    }
    wave_lds_sync();
    const double cur = 1.0 - sum / (double)cols;  // no column: 0 / 0 = NaN, never the minimum
    if (cur < mind) { mind = cur; arg = s; }
  }
  *dist_out = mind;
  *shift_out = arg;
}

__global__ __launch_bounds__(64) void k_sc_distance(Params P, Db db, const int* __restrict__ a, const int* __restrict__ b,
                                                    double* __restrict__ dist, int* __restrict__ shift) {
  __shared__ double tmp[kMaxSector];
  double d;
  int s;
  pair_distance(P, db, a[blockIdx.x], b[blockIdx.x], tmp, &d, &s);
  if (threadIdx.x == 0) {
    dist[blockIdx.x] = d;
    shift[blockIdx.x] = s;
  }
}

// nanoflann L2_Adaptor::evalMetric in float: four terms at a time, left to right, then the tail.
__device__ __forceinline__ float key_distance(const float* q, const float* __restrict__ k, int R) {
  float result = 0;
  int d = 0;
  for (; d + 3 < R; d += 4) {
    const float d0 = q[d] - k[d], d1 = q[d + 1] - k[d + 1], d2 = q[d + 2] - k[d + 2], d3 = q[d + 3] - k[d + 3];
    result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  for (; d < R; d++) {
    const float d0 = q[d] - k[d];
    result += d0 * d0;
  }
  return result;
}

struct DetectOut {
  int* loop_id;
  float* yaw;
  double* min_dist;
  int* nn_idx;
  int* nn_align;
};

// One workgroup per query keyframe i = first + blockIdx.x.
__global__ __launch_bounds__(kThreads) void k_sc_detect(Params P, Db db, int first, DetectOut o) {
  __shared__ float q[kMaxRing];
  __shared__ uint64_t wave_min[kWaves];
  __shared__ int cand[kMaxCand];
  __shared__ double cand_dist[kMaxCand];
  __shared__ int cand_shift[kMaxCand];
  __shared__ double tmp[kWaves][kMaxSector];
  const int i = first + blockIdx.x, out = blockIdx.x;
  if (i < P.E) {  // polarcontext_invkeys_mat_.size() < NUM_EXCLUDE_RECENT + 1
    if (threadIdx.x == 0) {
      o.loop_id[out] = -1; o.yaw[out] = 0.0f; o.min_dist[out] = kFar; o.nn_idx[out] = 0; o.nn_align[out] = 0;
    }
    return;
  }
  // the tree in use was built at the last eligible call whose counter was a multiple of P, over
  // every key but the newest E of that time
  const int prefix = 1 + P.P * ((i - P.E) / P.P);
  const int found = min(P.K, prefix);
  const int lane = lane_id(), wave = threadIdx.x / 64;
  if (threadIdx.x < P.R) q[threadIdx.x] = db.rkey[(size_t)i * P.R + threadIdx.x];
  __syncthreads();
  // exact k nearest in (distance, index) order: round k takes the smallest key above round k-1's.
  // A distance is a non-negative float (or NaN, above every number), so its bits order as it does.
  uint64_t last = 0;
  for (int k = 0; k < found; k++) {
    uint64_t best = ~0ull;
    for (int j = threadIdx.x; j < prefix; j += kThreads) {
      const float d = key_distance(q, db.rkey + (size_t)j * P.R, P.R);
      const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)j;
      if ((k == 0 || key > last) && key < best) best = key;
    }
    best = wave_min_u64(best);
    if (lane == 0) wave_min[wave] = best;
    __syncthreads();
    best = wave_min[0];
    for (int w = 1; w < kWaves; w++) best = wave_min[w] < best ? wave_min[w] : best;
    if (threadIdx.x == 0) cand[k] = (int)(uint32_t)best;
    last = best;
    __syncthreads();
  }
  // one wave per candidate
  for (int k = wave; k < found; k += kWaves) {
    double d;
    int s;
    pair_distance(P, db, i, cand[k], tmp[wave], &d, &s);
    if (lane == 0) { cand_dist[k] = d; cand_shift[k] = s; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double min_dist = kFar;
    int nn_align = 0, nn_idx = 0;
    for (int k = 0; k < found; k++) {
      if (cand_dist[k] < min_dist) { min_dist = cand_dist[k]; nn_align = cand_shift[k]; nn_idx = cand[k]; }
    }
    o.loop_id[out] = min_dist < P.dist_thres ? nn_idx : -1;
    // deg2rad(float degrees): degrees * M_PI / 180.0 in double, returned as float
    const float deg = (float)((double)nn_align * (360.0 / (double)P.S));
    o.yaw[out] = (float)((double)deg * kPi / 180.0);
    o.min_dist[out] = min_dist;
    o.nn_idx[out] = nn_idx;
    o.nn_align[out] = nn_align;
  }
}

}  // namespace place
}  // namespace lislam

using namespace lislam::place;
using namespace lislam;

struct lislam_place {
  lislam_ctx* ctx = nullptr;
  Params P{};
  int capacity = 0, n = 0;
  uint32_t* keys = nullptr;
  double* desc = nullptr;
  float* rkey = nullptr;
  double* skey = nullptr;
  double* cnorm = nullptr;
  // grow-only staging: packed points and their per-cloud (offset, count); detect / distance results
  lislam::DBuf stage, meta, res;
  Db db() const { return Db{desc, rkey, skey, cnorm}; }
};

namespace {

void free_place(lislam_place* p) {
  for (void* q : {(void*)p->keys, (void*)p->desc, (void*)p->rkey, (void*)p->skey, (void*)p->cnorm})
    if (q) (void)hipFree(q);
  delete p;
}

// describe + finish of n_clouds clouds into entries [p->n, p->n + n_clouds)
int describe(lislam_place* p, const Clouds& cl, int n_clouds) {
  lislam_ctx* c = p->ctx;
  const int bins = p->P.R * p->P.S;
  hipLaunchKernelGGL(k_sc_describe, dim3((unsigned)n_clouds * cl.blocks_per_cloud), dim3(kThreads), 0, c->stream, cl, p->P,
                     p->keys + (size_t)p->n * bins);
  hipLaunchKernelGGL(k_sc_finish, dim3(n_clouds), dim3(kThreads), 0, c->stream, p->P, p->n, p->keys, p->desc, p->rkey, p->skey,
                     p->cnorm);
  LISLAM_HIPCHK(c, hipGetLastError());
  p->n += n_clouds;
  return LISLAM_OK;
}

int blocks_for(int max_count) { return std::max(1, std::min(64, (max_count + kPointsPerBlock - 1) / kPointsPerBlock)); }

}  // namespace

extern "C" {

int lislam_place_create(lislam_ctx* c, const lislam_place_config* cfg, int32_t capacity, lislam_place** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  lislam_place_config d = {2.0, 80.0, 0.1, 0.13, 20, 60, 50, 10, 50};  // Scancontext.h:77-96
  if (cfg) d = *cfg;
  if (d.num_ring < 1 || d.num_ring > kMaxRing || d.num_sector < 1 || d.num_sector > kMaxSector || d.num_candidates < 1 ||
      d.num_candidates > kMaxCand)
    return fail(c, LISLAM_ERR_ARG, "lislam_place_create: num_ring 1..%d, num_sector 1..%d, num_candidates 1..%d", kMaxRing,
                kMaxSector, kMaxCand);
  if (!(d.max_radius > 0) || !std::isfinite(d.max_radius) || !std::isfinite(d.lidar_height) || !(d.search_ratio >= 0) ||
      !(d.search_ratio <= 1e6) || d.num_exclude_recent < 0 || d.tree_making_period < 1 || capacity < 1)
    return fail(c, LISLAM_ERR_ARG, "lislam_place_create: invalid configuration or capacity");
  hipSetDevice(c->device);
  lislam_place* p = new lislam_place();
  p->ctx = c;
  p->P = Params{d.lidar_height, d.max_radius, d.search_ratio, d.dist_thres, d.num_ring, d.num_sector, d.num_exclude_recent,
                d.num_candidates, d.tree_making_period};
  p->capacity = capacity;
  const size_t cap = (size_t)capacity, bins = (size_t)d.num_ring * d.num_sector;
  const bool ok = hipMalloc(&p->keys, cap * bins * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc(&p->desc, cap * bins * sizeof(double)) == hipSuccess &&
                  hipMalloc(&p->rkey, cap * d.num_ring * sizeof(float)) == hipSuccess &&
                  hipMalloc(&p->skey, cap * d.num_sector * sizeof(double)) == hipSuccess &&
                  hipMalloc(&p->cnorm, cap * d.num_sector * sizeof(double)) == hipSuccess &&
                  // every entry is described once: all grids start at NO_POINT
                  hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->keys), (int)height_key(kNoPoint), cap * bins,
                                    c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    free_place(p);
    return fail(c, LISLAM_ERR_DEVICE, "lislam_place_create: device allocation failed");
  }
  *out = p;
  return LISLAM_OK;
}

int lislam_place_destroy(lislam_place* p) {
  if (!p) return LISLAM_ERR_ARG;
  hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  free_place(p);
  return LISLAM_OK;
}

int lislam_place_size(lislam_place* p, int32_t* n) {
  if (!p || !n) return LISLAM_ERR_ARG;
  *n = p->n;
  return LISLAM_OK;
}

int lislam_place_add_clouds(lislam_place* p, const void* points, const int32_t* counts, int32_t n_clouds) {
  if (!p || n_clouds < 0 || (n_clouds > 0 && !counts)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n_clouds == 0) return LISLAM_OK;
  int64_t total = 0;
  int max_count = 0;
  for (int k = 0; k < n_clouds; k++) {
    if (counts[k] < 0) return fail(c, LISLAM_ERR_ARG, "lislam_place_add_clouds: counts[%d] = %d", k, counts[k]);
    total += counts[k];
    max_count = std::max(max_count, counts[k]);
  }
  if (total > 0 && !points) return fail(c, LISLAM_ERR_ARG, "lislam_place_add_clouds: null points");
  if (total > 0x3fffffff) return fail(c, LISLAM_ERR_CAPACITY, "lislam_place_add_clouds: clouds too large");
  if ((int64_t)p->n + n_clouds > p->capacity)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_place_add_clouds: %d + %d entries exceed the capacity %d", p->n, n_clouds,
                p->capacity);
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, p->stage.reserve((size_t)std::max<int64_t>(total, 1) * 16, c->stream));
  LISLAM_HIPCHK(c, p->meta.reserve((size_t)n_clouds * (sizeof(long long) + sizeof(int)), c->stream));
  std::vector<long long> off(n_clouds);
  long long run = 0;
  for (int k = 0; k < n_clouds; k++) { off[k] = run; run += counts[k]; }
  long long* d_off = p->meta.as<long long>();
  int* d_cnt = reinterpret_cast<int*>(d_off + n_clouds);
  // pageable sources: these copies have read them when they return
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)n_clouds * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_cnt, counts, (size_t)n_clouds * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (total) LISLAM_HIPCHK(c, hipMemcpyAsync(p->stage.p, points, (size_t)total * 16, hipMemcpyDefault, c->stream));
  Clouds cl{p->stage.as<const float4>(), d_off, d_cnt, 0, blocks_for(max_count)};
  LISLAM_RC(describe(p, cl, n_clouds));
  // the host arrays above leave scope: the copies that read them must have run
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_place_add_batch(lislam_place* p, lislam_batch* b, int32_t first_scan, int32_t n_scans) {
  if (!p || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  const char* who = "lislam_place_add_batch";
  LISLAM_RC(check_same_context(c, who, b));
  LISLAM_RC(check_scan_range(c, who, b, first_scan, n_scans));
  LISLAM_RC(check_cloud_track(c, who, b));
  LISLAM_RC(check_extracted(c, who, b, first_scan, n_scans));
  LISLAM_RC(check_capacity(c, who, p->n, n_scans, "entries", p->capacity));
  if (n_scans == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  Clouds cl{reinterpret_cast<const float4*>(b->fa.track) + (size_t)first_scan * b->N, nullptr, nullptr, b->N, blocks_for(b->N)};
  return describe(p, cl, n_scans);
}

int lislam_place_add_batch_scans(lislam_place* p, lislam_batch* b, const int32_t* scans, int32_t n) {
  if (!p || !b || n < 0 || (n > 0 && !scans)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  const char* who = "lislam_place_add_batch_scans";
  LISLAM_RC(check_same_context(c, who, b));
  LISLAM_RC(check_cloud_track(c, who, b));
  LISLAM_RC(check_extracted_any(c, who, b, n));
  LISLAM_RC(check_index(c, who, "scans", scans, n, b->extracted, false));
  LISLAM_RC(check_capacity(c, who, p->n, n, "entries", p->capacity));
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, p->meta.reserve((size_t)n * (sizeof(long long) + sizeof(int)), c->stream));
  // cloud k = scan scans[k]: the packed form's (offset, count) pairs over the batch's cloud_track
  std::vector<long long> off(n);
  std::vector<int> cnt(n, b->N);
  for (int k = 0; k < n; k++) off[k] = (long long)scans[k] * b->N;
  long long* d_off = p->meta.as<long long>();
  int* d_cnt = reinterpret_cast<int*>(d_off + n);
  // pageable sources: these copies have read them when they return
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_cnt, cnt.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  Clouds cl{reinterpret_cast<const float4*>(b->fa.track), d_off, d_cnt, 0, blocks_for(b->N)};
  LISLAM_RC(describe(p, cl, n));
  // the host arrays above leave scope: the copies that read them must have run
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_place_detect(lislam_place* p, int32_t first, int32_t n, int32_t* loop_id, float* yaw, double* min_dist,
                        int32_t* nn_idx, int32_t* nn_align) {
  if (!p || n < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (first < 0 || (int64_t)first + n > p->n)
    return fail(c, LISLAM_ERR_ARG, "lislam_place_detect: keyframes [%d, %d + %d) out of range (size %d)", first, first, n, p->n);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n;
  LISLAM_HIPCHK(c, p->res.reserve(N * 24, c->stream));
  // [min_dist double][loop_id][yaw][nn_idx][nn_align]
  double* d_dist = p->res.as<double>();
  int* d_loop = reinterpret_cast<int*>(d_dist + N);
  float* d_yaw = reinterpret_cast<float*>(d_loop + N);
  int* d_idx = reinterpret_cast<int*>(d_yaw + N);
  int* d_align = d_idx + N;
  hipLaunchKernelGGL(k_sc_detect, dim3(n), dim3(kThreads), 0, c->stream, p->P, p->db(), first,
                     DetectOut{d_loop, d_yaw, d_dist, d_idx, d_align});
  LISLAM_HIPCHK(c, hipGetLastError());
  if (loop_id) LISLAM_HIPCHK(c, hipMemcpyAsync(loop_id, d_loop, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (yaw) LISLAM_HIPCHK(c, hipMemcpyAsync(yaw, d_yaw, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (min_dist) LISLAM_HIPCHK(c, hipMemcpyAsync(min_dist, d_dist, N * 8, hipMemcpyDeviceToHost, c->stream));
  if (nn_idx) LISLAM_HIPCHK(c, hipMemcpyAsync(nn_idx, d_idx, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (nn_align) LISLAM_HIPCHK(c, hipMemcpyAsync(nn_align, d_align, N * 4, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_place_distance(lislam_place* p, const int32_t* a, const int32_t* b, int32_t n_pairs, double* dist, int32_t* shift) {
  if (!p || n_pairs < 0 || (n_pairs > 0 && (!a || !b))) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  for (int k = 0; k < n_pairs; k++)
    if (a[k] < 0 || a[k] >= p->n || b[k] < 0 || b[k] >= p->n)
      return fail(c, LISLAM_ERR_ARG, "lislam_place_distance: pair %d = (%d, %d) out of range (size %d)", k, a[k], b[k], p->n);
  if (n_pairs == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n_pairs;
  LISLAM_HIPCHK(c, p->res.reserve(N * 24, c->stream));
  double* d_dist = p->res.as<double>();
  int* d_shift = reinterpret_cast<int*>(d_dist + N);
  int* d_a = d_shift + N;
  int* d_b = d_a + N;
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_a, a, N * 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_b, b, N * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_sc_distance, dim3(n_pairs), dim3(64), 0, c->stream, p->P, p->db(), d_a, d_b, d_dist, d_shift);
  LISLAM_HIPCHK(c, hipGetLastError());
  if (dist) LISLAM_HIPCHK(c, hipMemcpyAsync(dist, d_dist, N * 8, hipMemcpyDeviceToHost, c->stream));
  if (shift) LISLAM_HIPCHK(c, hipMemcpyAsync(shift, d_shift, N * 4, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_place_download(lislam_place* p, int32_t what, int32_t index, void* dst, int32_t cap, int32_t* n) {
  if (!p || !dst || cap < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (index < 0 || index >= p->n)
    return fail(c, LISLAM_ERR_ARG, "lislam_place_download: index %d out of range (size %d)", index, p->n);
  const void* src;
  int cnt;
  size_t esz;
  switch (what) {
    case LISLAM_PLACE_DESC: cnt = p->P.R * p->P.S; esz = 8; src = p->desc + (size_t)index * cnt; break;
    case LISLAM_PLACE_RING_KEY: cnt = p->P.R; esz = 4; src = p->rkey + (size_t)index * cnt; break;
    case LISLAM_PLACE_SECTOR_KEY: cnt = p->P.S; esz = 8; src = p->skey + (size_t)index * cnt; break;
    default: return fail(c, LISLAM_ERR_ARG, "lislam_place_download: unknown output %d", what);
  }
  if (n) *n = cnt;
  if (cap < cnt) return fail(c, LISLAM_ERR_CAPACITY, "lislam_place_download: %d elements, capacity %d", cnt, cap);
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)cnt * esz, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

}  // extern "C"
