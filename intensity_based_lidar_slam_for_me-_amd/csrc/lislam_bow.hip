// ORB bag-of-words loop detection (lislam_bow_*): the reference's live loop detector, the DBoW3
// query of loopClosureHandler::detectLoop (src/loop_closure_handler.cpp:127-188, called from
// keyframeProcessor :108-111), as a device-resident database.  DBoW3 itself is restated from the
// published library (rmsalinas/DBoW3: Vocabulary.cpp, Database.cpp, BowVector.cpp,
// ScoringObject.cpp, DescManip.cpp) for the one combination the reference runs: TF_IDF weights,
// L1_NORM scoring, no direct index.
//
//   k_bow_words    Vocabulary::transform(feature, id, weight): the descent of many descriptors
//   k_bow_vector   transform(features, v) + normalize(L1): one image's sorted (word, value) list
//   k_bow_query    Database::queryL1: the accumulated score of every (query, earlier entry) pair
//   k_bow_select   the max_results best of each query and detectLoop's decision
//   k_bow_score    L1Scoring::score of arbitrary pairs of entries
//   k_bow_gather   one entry's vector out of the interleaved store
//
// Semantics pinned here (tests/restate_bow.py is the same text in Python):
//  * Descent: among a node's children, in ascending node id, the first with the smallest Hamming
//    distance (strict <).  The minimum is taken over the key (distance << 8 | child slot), so the
//    first child wins a tie by the key's order.
//  * v[word] += w once per occurrence, in double: a word seen c times holds ((w + w) + w) ..., not
//    c * w.  Words of weight 0 never enter the vector.
//  * The L1 norm is one sequential sum in ascending word id; the values are divided by it.
//  * A query accumulates fabs(q - d) - fabs(q) - fabs(d) per entry in ascending query word id; an
//    entry sharing no word with the query is no result.  Results are ordered by (score, entry id):
//    DBoW3 leaves equal scores to std::sort, here the lower id comes first.
//  * max_id == -1 means "no limit" in Database::query, so the keyframe with i - gap == -1 is queried
//    against every earlier entry although detectLoop then returns -1.  Kept.
//  * All arithmetic is plain double without FMA (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lislam_batch.hpp"
#include "lislam_ctx.hpp"
#include "lislam_device.hpp"

namespace lislam {
namespace bow {

constexpr int kThreads = 256;
constexpr int kMaxFeat = 2048;     // max_features: one image's words are sorted in LDS (32 KB)
constexpr int kMaxChildren = 64;   // one wave per descriptor covers a node
constexpr int kMaxResults = 16;
constexpr int kQueryChunk = 512;   // queries per k_bow_query launch (bounds the score scratch)

struct Tree {
  const int2* node;      // [n_nodes] (first child, child count); a leaf: (word id, 0)
  const uint4* desc;     // [n_nodes][2] 256-bit descriptors, children of a node contiguous
  const double* weight;  // [n_words]
  int depth;             // the deepest leaf
};

// The descriptors of n_images images: image k holds min(counts[k], max_count) rows of 32 bytes from
// row (offsets ? offsets[k] : k * stride) of desc; its words go to words[k * per_image ..].
struct Source {
  const uint4* desc;
  const long long* offsets;  // null: uniform stride
  const int* counts;         // device
  long long stride;
  int n_images, per_image, max_count;
};

template <int kLanes>
__device__ __forceinline__ uint32_t group_umin(uint32_t v) {
  if constexpr (kLanes == 64) {
    return wave_umin(v);
  } else {  // one 16-lane DPP row: every lane of the row ends with the row's minimum
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true));  // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
  }
}

__device__ __forceinline__ int popc4(uint4 a, uint4 b) {
  return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

// kLanes lanes per descriptor (16: four descriptors per wave, every node has <= 16 children; 64:
// one wave per descriptor).  The descriptor stays in registers; every level is one 32-byte load
// per lane and one group minimum.  The level loop is uniform over the wave (the DPP reductions
// need every lane); a group that has reached its leaf idles.
template <int kLanes>
__global__ __launch_bounds__(kThreads) void k_bow_words(Tree T, Source s, int* __restrict__ words,
                                                        double* __restrict__ weights /* nullable */) {
  const int slot = (int)((blockIdx.x * (unsigned)kThreads + threadIdx.x) / kLanes);
  const int l = threadIdx.x % kLanes;
  const int img = slot / s.per_image, j = slot - img * s.per_image;
  bool live = false;
  if (img < s.n_images) live = j < min(s.counts[img], s.max_count);
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (live) {
    const long long row = (s.offsets ? s.offsets[img] : (long long)img * s.stride) + j;
    d0 = s.desc[row * 2];
    d1 = s.desc[row * 2 + 1];
  }
  int node = 0, word = -1;
  bool walking = live;
  for (int level = 0; level <= T.depth; level++) {
    int2 info = make_int2(0, 0);
    if (walking) info = T.node[node];
    if (walking && info.y == 0) {
      word = info.x;
      walking = false;
    }
    uint32_t key = 0xffffffffu;
    if (walking && l < info.y) {
      const uint4 c0 = T.desc[(size_t)(info.x + l) * 2], c1 = T.desc[(size_t)(info.x + l) * 2 + 1];
      key = ((uint32_t)(popc4(d0, c0) + popc4(d1, c1)) << 8) | (uint32_t)l;
    }
    key = group_umin<kLanes>(key);
    if (walking) node = info.x + (int)(key & 0xffu);
  }
  if (live && l == 0) {
    words[(size_t)img * s.per_image + j] = word;
    if (weights) weights[(size_t)img * s.per_image + j] = T.weight[word];
  }
}

// The interleaved store: word j of entry e at words[j * capacity + e] (the query walks many
// entries in step, one per lane).
struct Store {
  int* words;
  double* vals;
  int* len;
  int capacity;
};

// LDS of k_bow_vector / k_bow_query, sized by the database's max_features (a 1,000-feature database
// keeps eight waves per SIMD where the 4,096 limit would leave two).
__host__ __device__ inline int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
inline size_t vector_lds(int max_features) { return (size_t)pow2_at_least(max_features) * 16 + 16; }
inline size_t query_lds(int max_features) { return (size_t)max_features * 12; }

// One workgroup per image.  lds: [val double P2][key int P2][pos int P2 + 1], P2 = pow2_at_least(max_features).
__global__ __launch_bounds__(kThreads) void k_bow_vector(Tree T, Source s, const int* __restrict__ words, Store st, int first,
                                                         int P2) {
  extern __shared__ double bow_lds[];
  double* val = bow_lds;
  int* key = reinterpret_cast<int*>(val + P2);
  int* pos = key + P2;
  __shared__ int heads[kThreads], valid[kThreads];
  __shared__ double norm_s;
  const int img = blockIdx.x, e = first + img, tid = threadIdx.x;
  const int c = min(s.counts[img], s.max_count);
  const int P = pow2_at_least(c);
  const int* w = words + (size_t)img * s.per_image;
  for (int i = tid; i < P; i += kThreads) {
    int k = INT_MAX;
    if (i < c) {
      const int id = w[i];
      if (id >= 0 && T.weight[id] > 0) k = id;  // if (w > 0) v.addWeight(id, w)
    }
    key[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int i = tid; i < P; i += kThreads) {
        const int p = i ^ jj;
        if (p > i) {
          const int a = key[i], b = key[p];
          if ((a > b) == ((i & k) == 0)) { key[i] = b; key[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  // run heads of the sorted ids: thread t owns [t * C, t * C + C)
  const int C = (P + kThreads - 1) / kThreads;
  const int lo = min(tid * C, P), hi = min(lo + C, P);
  int nh = 0, nv = 0;
  for (int i = lo; i < hi; i++) {
    const int k = key[i];
    if (k == INT_MAX) continue;
    nv++;
    if (i == 0 || key[i - 1] != k) nh++;
  }
  heads[tid] = nh;
  valid[tid] = nv;
  __syncthreads();
  int base = 0, U = 0, V = 0;
  for (int t = 0; t < kThreads; t++) {
    if (t < tid) base += heads[t];
    U += heads[t];
    V += valid[t];
  }
  for (int i = lo; i < hi; i++) {
    const int k = key[i];
    if (k == INT_MAX) continue;
    if (i == 0 || key[i - 1] != k) pos[base++] = i;
  }
  if (tid == 0) pos[U] = V;
  __syncthreads();
  for (int u = tid; u < U; u += kThreads) {
    const int n = pos[u + 1] - pos[u];
    const double wt = T.weight[key[pos[u]]];
    double v = wt;
    for (int r = 1; r < n; r++) v = v + wt;
    val[u] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    for (int u = 0; u < U; u++) norm = norm + fabs(val[u]);
    norm_s = norm;
  }
  __syncthreads();
  const double norm = norm_s;
  for (int u = tid; u < U; u += kThreads) {
    double v = val[u];
    if (norm > 0.0) v = v / norm;
    st.words[(size_t)u * st.capacity + e] = key[pos[u]];
    st.vals[(size_t)u * st.capacity + e] = v;
  }
  if (tid == 0) st.len[e] = U;
}

struct Decide {
  double th, index_th;
  int gap, max_results, min_frame, index_bound;
};

// Entries a query of keyframe k sees: Database::query(.., max_id = k - gap) over the k entries
// added before it.
__device__ __forceinline__ int query_limit(int k, int gap) {
  const long long max_id = (long long)k - gap;
  if (max_id == -1) return k;
  return max_id < 0 ? 0 : (int)min((long long)k, max_id);
}

// grid (entry tiles, queries): lane = one entry, walking its words in step with its neighbours
// (coalesced across the interleaved store) against the query's list in LDS.
__global__ __launch_bounds__(kThreads) void k_bow_query(Store st, Decide D, int first, double* __restrict__ scores,
                                                        int stride, int F) {
  extern __shared__ double bow_lds[];  // [qv double F][qw int F]
  double* qv = bow_lds;
  int* qw = reinterpret_cast<int*>(qv + F);
  const int k = first + blockIdx.y;
  const int limit = query_limit(k, D.gap);
  if ((int)(blockIdx.x * kThreads) >= limit) return;
  const int Q = st.len[k];
  for (int j = threadIdx.x; j < Q; j += kThreads) {
    qw[j] = st.words[(size_t)j * st.capacity + k];
    qv[j] = st.vals[(size_t)j * st.capacity + k];
  }
  __syncthreads();
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= limit) return;
  const int len = st.len[e];
  int qp = 0;
  double acc = 0.0;
  bool found = false;
  for (int j = 0; j < len && qp < Q; j++) {
    const int w = st.words[(size_t)j * st.capacity + e];
    while (qp < Q && qw[qp] < w) qp++;
    if (qp < Q && qw[qp] == w) {
      const double d = st.vals[(size_t)j * st.capacity + e], q = qv[qp];
      const double value = fabs(q - d) - fabs(q) - fabs(d);
      acc = found ? acc + value : value;
      found = true;
    }
  }
  scores[(size_t)blockIdx.y * stride + e] = found ? acc : INFINITY;
}

struct DetectOut {
  int* loop_id;    // [n]
  int* n_ret;      // [n]
  int* ret_id;     // [n][max_results]
  double* ret_score;
};

// One workgroup per query: max_results rounds of the smallest (score, id) above the last one taken,
// then detectLoop's decision.
__global__ __launch_bounds__(kThreads) void k_bow_select(Decide D, int first, const double* __restrict__ scores, int stride,
                                                         int out0, DetectOut o) {
  __shared__ double rs[kThreads];
  __shared__ int ri[kThreads];
  __shared__ double top_s[kMaxResults];
  __shared__ int top_i[kMaxResults];
  const int k = first + blockIdx.x, out = out0 + blockIdx.x, tid = threadIdx.x;
  const int limit = query_limit(k, D.gap);
  const double* sc = scores + (size_t)blockIdx.x * stride;
  double last_s = 0.0;
  int last_i = -1, nret = 0;
  for (int r = 0; r < D.max_results; r++) {
    double bs = INFINITY;
    int bi = INT_MAX;
    for (int e = tid; e < limit; e += kThreads) {
      const double s = sc[e];
      if (s == INFINITY) continue;
      if (r > 0 && !(s > last_s || (s == last_s && e > last_i))) continue;
      if (s < bs || (s == bs && e < bi)) { bs = s; bi = e; }
    }
    rs[tid] = bs;
    ri[tid] = bi;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
      if (tid < h) {
        const double s2 = rs[tid + h];
        const int i2 = ri[tid + h];
        if (i2 != INT_MAX && (ri[tid] == INT_MAX || s2 < rs[tid] || (s2 == rs[tid] && i2 < ri[tid]))) {
          rs[tid] = s2;
          ri[tid] = i2;
        }
      }
      __syncthreads();
    }
    bs = rs[0];
    bi = ri[0];
    __syncthreads();
    if (bi == INT_MAX) break;  // uniform
    if (tid == 0) { top_s[r] = bs; top_i[r] = bi; }
    last_s = bs;
    last_i = bi;
    nret = r + 1;
  }
  if (tid != 0) return;
  const int R = D.max_results;
  for (int r = 0; r < R; r++) {
    o.ret_id[(size_t)out * R + r] = r < nret ? top_i[r] : -1;
    o.ret_score[(size_t)out * R + r] = r < nret ? -top_s[r] / 2.0 : 0.0;
  }
  o.n_ret[out] = nret;
  int loop = -1;
  if ((long long)k - D.gap >= 0) {
    bool find = false;
    if (nret >= 1 && -top_s[0] / 2.0 > D.th)
      for (int r = 1; r < nret; r++)
        if (-top_s[r] / 2.0 > D.th) find = true;
    if (find && k > D.min_frame) {
      int m = -1;
      for (int r = 0; r < nret; r++)
        if (m == -1 || (top_i[r] < m && -top_s[r] / 2.0 > D.index_th)) m = top_i[r];
      loop = m < D.index_bound ? m : -1;
    }
  }
  o.loop_id[out] = loop;
}

// L1Scoring::score(v1, v2): one lane per pair.
__global__ __launch_bounds__(kThreads) void k_bow_score(Store st, const int* __restrict__ a, const int* __restrict__ b, int n,
                                                        double* __restrict__ out) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= n) return;
  const int ea = a[t], eb = b[t];
  const int la = st.len[ea], lb = st.len[eb];
  int i = 0, j = 0;
  double score = 0;
  while (i < la && j < lb) {
    const int wa = st.words[(size_t)i * st.capacity + ea], wb = st.words[(size_t)j * st.capacity + eb];
    if (wa == wb) {
      const double vi = st.vals[(size_t)i * st.capacity + ea], wi = st.vals[(size_t)j * st.capacity + eb];
      score += fabs(vi - wi) - fabs(vi) - fabs(wi);
      i++;
      j++;
    } else if (wa < wb) {
      i++;
    } else {
      j++;
    }
  }
  out[t] = -score / 2.0;
}

__global__ __launch_bounds__(kThreads) void k_bow_gather(Store st, int e, int* __restrict__ w, double* __restrict__ v) {
  const int len = st.len[e];
  for (int j = blockIdx.x * kThreads + threadIdx.x; j < len; j += gridDim.x * kThreads) {
    w[j] = st.words[(size_t)j * st.capacity + e];
    v[j] = st.vals[(size_t)j * st.capacity + e];
  }
}

}  // namespace bow
}  // namespace lislam

using namespace lislam::bow;

struct lislam_bow {
  lislam_ctx* ctx = nullptr;
  Decide D{};
  int capacity = 0, F = 0, n = 0;
  int n_nodes = 0, n_words = 0, max_children = 0;
  Tree T{};
  Store st{};
  void* tree_nodes = nullptr;
  void* tree_desc = nullptr;
  void* tree_weight = nullptr;
  // grow-only staging: packed descriptors, their words, per-image (offset, count), results
  void* stage = nullptr;
  size_t stage_bytes = 0;
  void* wstage = nullptr;
  size_t wstage_bytes = 0;
  void* meta = nullptr;
  size_t meta_bytes = 0;
  void* res = nullptr;
  size_t res_bytes = 0;
};

namespace {

int bfail(lislam_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define BCHK(ctx, x)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) return bfail(ctx, LISLAM_ERR_DEVICE, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

int reserve(lislam_ctx* c, void** p, size_t* have, size_t want) {
  if (want <= *have) return LISLAM_OK;
  if (*p) {
    BCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
  }
  BCHK(c, hipMalloc(p, want));
  *have = want;
  return LISLAM_OK;
}

void free_bow(lislam_bow* p) {
  for (void* q : {p->tree_nodes, p->tree_desc, p->tree_weight, (void*)p->st.words, (void*)p->st.vals, (void*)p->st.len, p->stage,
                  p->wstage, p->meta, p->res})
    if (q) (void)hipFree(q);
  delete p;
}

// The descent of every descriptor of src into words (and weights), on the context stream.
void launch_words(lislam_bow* p, const Source& src, int* words, double* weights) {
  const long long slots = (long long)src.n_images * src.per_image;
  if (p->max_children <= 16) {
    const unsigned blocks = (unsigned)((slots * 16 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_bow_words<16>, dim3(blocks), dim3(kThreads), 0, p->ctx->stream, p->T, src, words, weights);
  } else {
    const unsigned blocks = (unsigned)((slots * 64 + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_bow_words<64>, dim3(blocks), dim3(kThreads), 0, p->ctx->stream, p->T, src, words, weights);
  }
}

// words + vector of the images of src into entries [p->n, p->n + src.n_images)
int add_images(lislam_bow* p, const Source& src) {
  lislam_ctx* c = p->ctx;
  int rc;
  if ((rc = reserve(c, &p->wstage, &p->wstage_bytes, (size_t)src.n_images * src.per_image * sizeof(int)))) return rc;
  int* words = static_cast<int*>(p->wstage);
  launch_words(p, src, words, nullptr);
  hipLaunchKernelGGL(k_bow_vector, dim3(src.n_images), dim3(kThreads), vector_lds(p->F), c->stream, p->T, src, words, p->st,
                     p->n, pow2_at_least(p->F));
  BCHK(c, hipGetLastError());
  p->n += src.n_images;
  return LISLAM_OK;
}

}  // namespace

extern "C" {

int lislam_bow_create(lislam_ctx* c, int32_t n_nodes, const int32_t* parent, const uint8_t* descriptor, const double* weight,
                      const lislam_bow_config* cfg, int32_t capacity, int32_t max_features, lislam_bow** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  lislam_bow_config d = {0.0155, 0.015, 50, 4, 5, 6};  // detectLoop's constants (loop_closure_handler.cpp:127-188)
  if (cfg) d = *cfg;
  if (!parent || !descriptor || !weight || n_nodes < 2 || n_nodes > (1 << 28))
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: a vocabulary needs its three arrays and at least two nodes");
  if (capacity < 1 || max_features < 1 || max_features > kMaxFeat || (int64_t)capacity * max_features > (1ll << 31) - 1)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: capacity >= 1, max_features 1..%d, capacity * max_features < 2^31", kMaxFeat);
  if (d.max_results < 1 || d.max_results > kMaxResults || d.min_loop_search_gap < 0 || !std::isfinite(d.min_loop_bow_threshold) ||
      !std::isfinite(d.index_score_threshold))
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: max_results 1..%d, min_loop_search_gap >= 0, finite thresholds", kMaxResults);
  // the tree: parents before children, <= 64 children per node, finite weights >= 0
  if (parent[0] != -1) return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: parent[0] = %d, the root's must be -1", parent[0]);
  std::vector<int> nchild(n_nodes, 0);
  for (int i = 1; i < n_nodes; i++) {
    if (parent[i] < 0 || parent[i] >= i)
      return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: parent[%d] = %d, want 0 <= parent < %d", i, parent[i], i);
    nchild[parent[i]]++;
  }
  int max_children = 0;
  for (int i = 0; i < n_nodes; i++) {
    if (nchild[i] > kMaxChildren)
      return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: node %d has %d children, at most %d", i, nchild[i], kMaxChildren);
    max_children = std::max(max_children, nchild[i]);
    if (!std::isfinite(weight[i]) || weight[i] < 0)
      return bfail(c, LISLAM_ERR_ARG, "lislam_bow_create: weight[%d] = %g, want a finite weight >= 0", i, weight[i]);
  }
  // children lists in ascending id (a counting sort by parent keeps the order)
  std::vector<int> cstart(n_nodes + 1, 0);
  for (int i = 0; i < n_nodes; i++) cstart[i + 1] = cstart[i] + nchild[i];
  std::vector<int> clist(n_nodes - 1), fill(cstart.begin(), cstart.end() - 1);
  for (int i = 1; i < n_nodes; i++) clist[fill[parent[i]]++] = i;
  // word ids: the rank among leaves in ascending node id (createWords)
  std::vector<int> word(n_nodes, -1);
  int n_words = 0;
  for (int i = 0; i < n_nodes; i++)
    if (nchild[i] == 0) word[i] = n_words++;
  // breadth-first layout: the children of a node contiguous, in ascending id
  std::vector<int> order(n_nodes), where(n_nodes), depth_of(n_nodes, 0);
  order[0] = 0;
  where[0] = 0;
  int placed = 1, depth = 0;
  std::vector<int2> nodes(n_nodes);
  for (int q = 0; q < n_nodes; q++) {
    const int old = order[q];
    if (nchild[old] == 0) {
      nodes[q] = make_int2(word[old], 0);
      depth = std::max(depth, depth_of[old]);
      continue;
    }
    nodes[q] = make_int2(placed, nchild[old]);
    for (int k = cstart[old]; k < cstart[old + 1]; k++) {
      const int ch = clist[k];
      depth_of[ch] = depth_of[old] + 1;
      where[ch] = placed;
      order[placed++] = ch;
    }
  }
  std::vector<uint8_t> desc((size_t)n_nodes * 32);
  std::vector<double> wweight(std::max(n_words, 1), 0.0);
  for (int q = 0; q < n_nodes; q++) {
    memcpy(&desc[(size_t)q * 32], descriptor + (size_t)order[q] * 32, 32);
    if (nchild[order[q]] == 0) wweight[word[order[q]]] = weight[order[q]];
  }
  hipSetDevice(c->device);
  lislam_bow* p = new lislam_bow();
  p->ctx = c;
  p->D = Decide{d.min_loop_bow_threshold, d.index_score_threshold, d.min_loop_search_gap, d.max_results, d.min_frame_index,
                d.loop_index_bound};
  p->capacity = capacity;
  p->F = max_features;
  p->n_nodes = n_nodes;
  p->n_words = n_words;
  p->max_children = max_children;
  const size_t cells = (size_t)capacity * max_features;
  const bool ok = hipMalloc(&p->tree_nodes, (size_t)n_nodes * sizeof(int2)) == hipSuccess &&
                  hipMalloc(&p->tree_desc, (size_t)n_nodes * 32) == hipSuccess &&
                  hipMalloc(&p->tree_weight, wweight.size() * sizeof(double)) == hipSuccess &&
                  hipMalloc(&p->st.words, cells * sizeof(int)) == hipSuccess &&
                  hipMalloc(&p->st.vals, cells * sizeof(double)) == hipSuccess &&
                  hipMalloc(&p->st.len, (size_t)capacity * sizeof(int)) == hipSuccess &&
                  hipMemcpyAsync(p->tree_nodes, nodes.data(), (size_t)n_nodes * sizeof(int2), hipMemcpyHostToDevice, c->stream) ==
                      hipSuccess &&
                  hipMemcpyAsync(p->tree_desc, desc.data(), desc.size(), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                  hipMemcpyAsync(p->tree_weight, wweight.data(), wweight.size() * sizeof(double), hipMemcpyHostToDevice,
                                 c->stream) == hipSuccess &&
                  hipMemsetAsync(p->st.len, 0, (size_t)capacity * sizeof(int), c->stream) == hipSuccess &&
                  hipStreamSynchronize(c->stream) == hipSuccess;  // the host vectors leave scope
  if (!ok) {
    (void)hipGetLastError();
    free_bow(p);
    return bfail(c, LISLAM_ERR_DEVICE, "lislam_bow_create: device allocation failed");
  }
  p->st.capacity = capacity;
  p->T = Tree{static_cast<const int2*>(p->tree_nodes), static_cast<const uint4*>(p->tree_desc),
              static_cast<const double*>(p->tree_weight), depth};
  *out = p;
  return LISLAM_OK;
}

int lislam_bow_destroy(lislam_bow* p) {
  if (!p) return LISLAM_ERR_ARG;
  hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  free_bow(p);
  return LISLAM_OK;
}

int lislam_bow_size(lislam_bow* p, int32_t* n) {
  if (!p || !n) return LISLAM_ERR_ARG;
  *n = p->n;
  return LISLAM_OK;
}

// Stages n_images packed descriptor sets (host or device memory) and their offsets / counts.
static int stage_packed(lislam_bow* p, const char* who, const void* desc, const int32_t* counts, int n_images, Source* src) {
  lislam_ctx* c = p->ctx;
  int64_t total = 0;
  int max_count = 0;
  for (int k = 0; k < n_images; k++) {
    if (counts[k] < 0 || counts[k] > p->F)
      return bfail(c, LISLAM_ERR_ARG, "%s: counts[%d] = %d, want 0..max_features (%d)", who, k, counts[k], p->F);
    total += counts[k];
    max_count = std::max(max_count, counts[k]);
  }
  if (total > 0 && !desc) return bfail(c, LISLAM_ERR_ARG, "%s: null descriptors", who);
  hipSetDevice(c->device);
  int rc;
  if ((rc = reserve(c, &p->stage, &p->stage_bytes, (size_t)std::max<int64_t>(total, 1) * 32))) return rc;
  if ((rc = reserve(c, &p->meta, &p->meta_bytes, (size_t)n_images * (sizeof(long long) + sizeof(int))))) return rc;
  std::vector<long long> off(n_images);
  long long run = 0;
  for (int k = 0; k < n_images; k++) { off[k] = run; run += counts[k]; }
  long long* d_off = static_cast<long long*>(p->meta);
  int* d_cnt = reinterpret_cast<int*>(d_off + n_images);
  // pageable sources: these copies have read them when they return
  BCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)n_images * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  BCHK(c, hipMemcpyAsync(d_cnt, counts, (size_t)n_images * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (total) BCHK(c, hipMemcpyAsync(p->stage, desc, (size_t)total * 32, hipMemcpyDefault, c->stream));
  *src = Source{static_cast<const uint4*>(p->stage), d_off, d_cnt, 0, n_images, std::max(max_count, 1), p->F};
  return LISLAM_OK;
}

int lislam_bow_add(lislam_bow* p, const void* desc, const int32_t* counts, int32_t n_images) {
  if (!p || n_images < 0 || (n_images > 0 && !counts)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n_images == 0) return LISLAM_OK;
  if ((int64_t)p->n + n_images > p->capacity)
    return bfail(c, LISLAM_ERR_CAPACITY, "lislam_bow_add: %d + %d entries exceed the capacity %d", p->n, n_images, p->capacity);
  Source src{};
  int rc;
  if ((rc = stage_packed(p, "lislam_bow_add", desc, counts, n_images, &src))) return rc;
  if ((rc = add_images(p, src))) return rc;
  BCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_add_batch(lislam_bow* p, lislam_batch* b, int32_t first_scan, int32_t n_scans) {
  if (!p || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (b->ctx != c) return bfail(c, LISLAM_ERR_ARG, "lislam_bow_add_batch: the batch belongs to another context");
  if (first_scan < 0 || n_scans < 0 || (int64_t)first_scan + n_scans > b->max_scans)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_add_batch: scans [%d, %d + %d) out of range", first_scan, first_scan, n_scans);
  const uint8_t* desc = nullptr;
  const int* counts = nullptr;
  int cap = 0, nfeatures = 0, ran = 0;
  const int rc = lislam_orb_batch_descriptors(b, &desc, &counts, &cap, &nfeatures, &ran);
  if (rc == LISLAM_ERR_STATE || (rc == LISLAM_OK && first_scan + n_scans > ran))
    return bfail(c, LISLAM_ERR_STATE, "lislam_bow_add_batch: run lislam_batch_intensity_odometry over %d scans first",
                 first_scan + n_scans);
  if (rc) return rc;
  if (nfeatures > p->F)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_add_batch: the batch detects %d features, max_features is %d", nfeatures, p->F);
  if ((int64_t)p->n + n_scans > p->capacity)
    return bfail(c, LISLAM_ERR_CAPACITY, "lislam_bow_add_batch: %d + %d entries exceed the capacity %d", p->n, n_scans,
                 p->capacity);
  if (n_scans == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  // a scan keeps at most nfeatures keypoints; max_count bounds the rows read whatever the count says
  Source src{reinterpret_cast<const uint4*>(desc + (size_t)first_scan * cap * 32), nullptr, counts + first_scan, cap, n_scans,
             std::min(nfeatures, cap), std::min(nfeatures, cap)};
  return add_images(p, src);
}

int lislam_bow_detect(lislam_bow* p, int32_t first, int32_t n, int32_t* loop_id, int32_t* n_ret, int32_t* ret_id,
                      double* ret_score) {
  if (!p || n < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (first < 0 || (int64_t)first + n > p->n)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_detect: keyframes [%d, %d + %d) out of range (size %d)", first, first, n, p->n);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n, R = (size_t)p->D.max_results;
  const int stride = std::max(first + n, 1);  // a query sees fewer entries than its own index
  const int chunk = std::min(n, kQueryChunk);
  int rc;
  // [ret_score double N R][scores double chunk stride][loop_id N][n_ret N][ret_id N R]
  if ((rc = reserve(c, &p->res, &p->res_bytes, N * R * 8 + (size_t)chunk * stride * 8 + N * 8 + N * R * 4))) return rc;
  double* d_score = static_cast<double*>(p->res);
  double* d_acc = d_score + N * R;
  int* d_loop = reinterpret_cast<int*>(d_acc + (size_t)chunk * stride);
  int* d_nret = d_loop + N;
  int* d_id = d_nret + N;
  const DetectOut o{d_loop, d_nret, d_id, d_score};
  for (int q0 = 0; q0 < n; q0 += chunk) {
    const int m = std::min(chunk, n - q0);
    const int tiles = (stride + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_bow_query, dim3(tiles, m), dim3(kThreads), query_lds(p->F), c->stream, p->st, p->D, first + q0, d_acc,
                       stride, p->F);
    hipLaunchKernelGGL(k_bow_select, dim3(m), dim3(kThreads), 0, c->stream, p->D, first + q0, d_acc, stride, q0, o);
  }
  BCHK(c, hipGetLastError());
  if (loop_id) BCHK(c, hipMemcpyAsync(loop_id, d_loop, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (n_ret) BCHK(c, hipMemcpyAsync(n_ret, d_nret, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (ret_id) BCHK(c, hipMemcpyAsync(ret_id, d_id, N * R * 4, hipMemcpyDeviceToHost, c->stream));
  if (ret_score) BCHK(c, hipMemcpyAsync(ret_score, d_score, N * R * 8, hipMemcpyDeviceToHost, c->stream));
  BCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_score(lislam_bow* p, const int32_t* a, const int32_t* b, int32_t n_pairs, double* score) {
  if (!p || n_pairs < 0 || (n_pairs > 0 && (!a || !b))) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  for (int k = 0; k < n_pairs; k++)
    if (a[k] < 0 || a[k] >= p->n || b[k] < 0 || b[k] >= p->n)
      return bfail(c, LISLAM_ERR_ARG, "lislam_bow_score: pair %d = (%d, %d) out of range (size %d)", k, a[k], b[k], p->n);
  if (n_pairs == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  int rc;
  const size_t N = (size_t)n_pairs;
  if ((rc = reserve(c, &p->res, &p->res_bytes, N * 16))) return rc;
  double* d_score = static_cast<double*>(p->res);
  int* d_a = reinterpret_cast<int*>(d_score + N);
  int* d_b = d_a + N;
  BCHK(c, hipMemcpyAsync(d_a, a, N * 4, hipMemcpyHostToDevice, c->stream));
  BCHK(c, hipMemcpyAsync(d_b, b, N * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_bow_score, dim3((n_pairs + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, p->st, d_a, d_b,
                     n_pairs, d_score);
  BCHK(c, hipGetLastError());
  if (score) BCHK(c, hipMemcpyAsync(score, d_score, N * 8, hipMemcpyDeviceToHost, c->stream));
  BCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_transform(lislam_bow* p, const void* desc, int32_t n, int32_t* word_id, double* weight) {
  if (!p || n < 0 || (n > 0 && !desc)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n > (1 << 24)) return bfail(c, LISLAM_ERR_CAPACITY, "lislam_bow_transform: at most %d descriptors a call", 1 << 24);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  int rc;
  const size_t N = (size_t)n;
  if ((rc = reserve(c, &p->stage, &p->stage_bytes, N * 32))) return rc;
  if ((rc = reserve(c, &p->meta, &p->meta_bytes, 16))) return rc;
  if ((rc = reserve(c, &p->res, &p->res_bytes, N * 12))) return rc;
  double* d_wt = static_cast<double*>(p->res);
  int* d_word = reinterpret_cast<int*>(d_wt + N);
  int* d_cnt = static_cast<int*>(p->meta);
  const int cnt = n;
  BCHK(c, hipMemcpyAsync(d_cnt, &cnt, 4, hipMemcpyHostToDevice, c->stream));
  BCHK(c, hipMemcpyAsync(p->stage, desc, N * 32, hipMemcpyDefault, c->stream));
  const Source src{static_cast<const uint4*>(p->stage), nullptr, d_cnt, 0, 1, n, n};
  launch_words(p, src, d_word, d_wt);
  BCHK(c, hipGetLastError());
  if (word_id) BCHK(c, hipMemcpyAsync(word_id, d_word, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (weight) BCHK(c, hipMemcpyAsync(weight, d_wt, N * 8, hipMemcpyDeviceToHost, c->stream));
  BCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_download(lislam_bow* p, int32_t what, int32_t index, void* dst, int32_t cap, int32_t* n) {
  if (!p || !dst || cap < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (index < 0 || index >= p->n)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_download: index %d out of range (size %d)", index, p->n);
  if (what != LISLAM_BOW_WORDS && what != LISLAM_BOW_VALUES)
    return bfail(c, LISLAM_ERR_ARG, "lislam_bow_download: unknown output %d", what);
  hipSetDevice(c->device);
  int cnt = 0;
  BCHK(c, hipMemcpyAsync(&cnt, p->st.len + index, 4, hipMemcpyDeviceToHost, c->stream));
  BCHK(c, hipStreamSynchronize(c->stream));
  if (n) *n = cnt;
  if (cap < cnt) return bfail(c, LISLAM_ERR_CAPACITY, "lislam_bow_download: %d elements, capacity %d", cnt, cap);
  if (cnt == 0) return LISLAM_OK;
  int rc;
  if ((rc = reserve(c, &p->res, &p->res_bytes, (size_t)p->F * 12))) return rc;
  double* d_v = static_cast<double*>(p->res);
  int* d_w = reinterpret_cast<int*>(d_v + p->F);
  hipLaunchKernelGGL(k_bow_gather, dim3((cnt + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, p->st, index, d_w, d_v);
  BCHK(c, hipGetLastError());
  if (what == LISLAM_BOW_WORDS) BCHK(c, hipMemcpyAsync(dst, d_w, (size_t)cnt * 4, hipMemcpyDeviceToHost, c->stream));
  else BCHK(c, hipMemcpyAsync(dst, d_v, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->stream));
  BCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

}  // extern "C"
