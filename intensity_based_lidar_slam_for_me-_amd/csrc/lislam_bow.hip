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
#include "lislam_host.hpp"

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

// lislam_bow_add_batch_scans: image k = scan scans[k] of a batch, as the packed form's (offset, count) pair.
__global__ __launch_bounds__(kThreads) void k_bow_scan_list(const int* __restrict__ scans, int n, const int* __restrict__ counts,
                                                            int cap, long long* __restrict__ off, int* __restrict__ cnt) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const int s = scans[k];
  off[k] = (long long)s * cap;
  cnt[k] = counts[s];
}

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
using namespace lislam;

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
  DBuf stage, wstage, meta, res;
};

namespace {

void free_bow(lislam_bow* p) {
  for (void* q : {p->tree_nodes, p->tree_desc, p->tree_weight, (void*)p->st.words, (void*)p->st.vals, (void*)p->st.len})
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
  LISLAM_HIPCHK(c, p->wstage.reserve((size_t)src.n_images * src.per_image * sizeof(int), c->stream));
  int* words = p->wstage.as<int>();
  launch_words(p, src, words, nullptr);
  hipLaunchKernelGGL(k_bow_vector, dim3(src.n_images), dim3(kThreads), vector_lds(p->F), c->stream, p->T, src, words, p->st,
                     p->n, pow2_at_least(p->F));
  LISLAM_HIPCHK(c, hipGetLastError());
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
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: a vocabulary needs its three arrays and at least two nodes");
  if (capacity < 1 || max_features < 1 || max_features > kMaxFeat || (int64_t)capacity * max_features > (1ll << 31) - 1)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: capacity >= 1, max_features 1..%d, capacity * max_features < 2^31", kMaxFeat);
  if (d.max_results < 1 || d.max_results > kMaxResults || d.min_loop_search_gap < 0 || !std::isfinite(d.min_loop_bow_threshold) ||
      !std::isfinite(d.index_score_threshold))
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: max_results 1..%d, min_loop_search_gap >= 0, finite thresholds", kMaxResults);
  // the tree: parents before children, <= 64 children per node, finite weights >= 0
  if (parent[0] != -1) return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: parent[0] = %d, the root's must be -1", parent[0]);
  std::vector<int> nchild(n_nodes, 0);
  for (int i = 1; i < n_nodes; i++) {
    if (parent[i] < 0 || parent[i] >= i)
      return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: parent[%d] = %d, want 0 <= parent < %d", i, parent[i], i);
    nchild[parent[i]]++;
  }
  int max_children = 0;
  for (int i = 0; i < n_nodes; i++) {
    if (nchild[i] > kMaxChildren)
      return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: node %d has %d children, at most %d", i, nchild[i], kMaxChildren);
    max_children = std::max(max_children, nchild[i]);
    if (!std::isfinite(weight[i]) || weight[i] < 0)
      return fail(c, LISLAM_ERR_ARG, "lislam_bow_create: weight[%d] = %g, want a finite weight >= 0", i, weight[i]);
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
    return fail(c, LISLAM_ERR_DEVICE, "lislam_bow_create: device allocation failed");
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
      return fail(c, LISLAM_ERR_ARG, "%s: counts[%d] = %d, want 0..max_features (%d)", who, k, counts[k], p->F);
    total += counts[k];
    max_count = std::max(max_count, counts[k]);
  }
  if (total > 0 && !desc) return fail(c, LISLAM_ERR_ARG, "%s: null descriptors", who);
  hipSetDevice(c->device);
  LISLAM_HIPCHK(c, p->stage.reserve((size_t)std::max<int64_t>(total, 1) * 32, c->stream));
  LISLAM_HIPCHK(c, p->meta.reserve((size_t)n_images * (sizeof(long long) + sizeof(int)), c->stream));
  std::vector<long long> off(n_images);
  long long run = 0;
  for (int k = 0; k < n_images; k++) { off[k] = run; run += counts[k]; }
  long long* d_off = p->meta.as<long long>();
  int* d_cnt = reinterpret_cast<int*>(d_off + n_images);
  // pageable sources: these copies have read them when they return
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)n_images * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_cnt, counts, (size_t)n_images * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (total) LISLAM_HIPCHK(c, hipMemcpyAsync(p->stage.p, desc, (size_t)total * 32, hipMemcpyDefault, c->stream));
  *src = Source{p->stage.as<const uint4>(), d_off, d_cnt, 0, n_images, std::max(max_count, 1), p->F};
  return LISLAM_OK;
}

int lislam_bow_add(lislam_bow* p, const void* desc, const int32_t* counts, int32_t n_images) {
  if (!p || n_images < 0 || (n_images > 0 && !counts)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n_images == 0) return LISLAM_OK;
  if ((int64_t)p->n + n_images > p->capacity)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_bow_add: %d + %d entries exceed the capacity %d", p->n, n_images, p->capacity);
  Source src{};
  int rc;
  if ((rc = stage_packed(p, "lislam_bow_add", desc, counts, n_images, &src))) return rc;
  if ((rc = add_images(p, src))) return rc;
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_add_batch(lislam_bow* p, lislam_batch* b, int32_t first_scan, int32_t n_scans) {
  if (!p || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  const char* who = "lislam_bow_add_batch";
  LISLAM_RC(check_same_context(c, who, b));
  LISLAM_RC(check_scan_range(c, who, b, first_scan, n_scans));
  OrbDescriptors o;
  LISLAM_RC(orb_descriptors(c, who, b, first_scan + n_scans, &o));
  if (o.nfeatures > p->F)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_add_batch: the batch detects %d features, max_features is %d", o.nfeatures, p->F);
  LISLAM_RC(check_capacity(c, who, p->n, n_scans, "entries", p->capacity));
  if (n_scans == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  // a scan keeps at most nfeatures keypoints; max_count bounds the rows read whatever the count says
  Source src{reinterpret_cast<const uint4*>(o.desc + (size_t)first_scan * o.cap * 32), nullptr, o.counts + first_scan, o.cap,
             n_scans, std::min(o.nfeatures, o.cap), std::min(o.nfeatures, o.cap)};
  return add_images(p, src);
}

int lislam_bow_add_batch_scans(lislam_bow* p, lislam_batch* b, const int32_t* scans, int32_t n) {
  if (!p || !b || n < 0 || (n > 0 && !scans)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  const char* who = "lislam_bow_add_batch_scans";
  LISLAM_RC(check_same_context(c, who, b));
  OrbDescriptors o;
  LISLAM_RC(orb_descriptors(c, who, b, -1, &o));
  LISLAM_RC(check_index(c, who, "scans", scans, n, o.ran, false));
  if (o.nfeatures > p->F)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_add_batch_scans: the batch detects %d features, max_features is %d", o.nfeatures,
                p->F);
  LISLAM_RC(check_capacity(c, who, p->n, n, "entries", p->capacity));
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  // [offsets long long n][counts int n][scans int n]
  LISLAM_HIPCHK(c, p->meta.reserve((size_t)n * (sizeof(long long) + 2 * sizeof(int)), c->stream));
  long long* d_off = p->meta.as<long long>();
  int* d_cnt = reinterpret_cast<int*>(d_off + n);
  int* d_scans = d_cnt + n;
  // pageable source: the copy has read it when it returns
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_scans, scans, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_bow_scan_list, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, d_scans, n, o.counts,
                     o.cap, d_off, d_cnt);
  // as the range form: max_count bounds the rows read whatever the count says
  Source src{reinterpret_cast<const uint4*>(o.desc), d_off, d_cnt, 0, n, std::min(o.nfeatures, o.cap),
             std::min(o.nfeatures, o.cap)};
  return add_images(p, src);
}

int lislam_bow_detect(lislam_bow* p, int32_t first, int32_t n, int32_t* loop_id, int32_t* n_ret, int32_t* ret_id,
                      double* ret_score) {
  if (!p || n < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (first < 0 || (int64_t)first + n > p->n)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_detect: keyframes [%d, %d + %d) out of range (size %d)", first, first, n, p->n);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n, R = (size_t)p->D.max_results;
  const int stride = std::max(first + n, 1);  // a query sees fewer entries than its own index
  const int chunk = std::min(n, kQueryChunk);
  // [ret_score double N R][scores double chunk stride][loop_id N][n_ret N][ret_id N R]
  LISLAM_HIPCHK(c, p->res.reserve(N * R * 8 + (size_t)chunk * stride * 8 + N * 8 + N * R * 4, c->stream));
  double* d_score = p->res.as<double>();
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
  LISLAM_HIPCHK(c, hipGetLastError());
  if (loop_id) LISLAM_HIPCHK(c, hipMemcpyAsync(loop_id, d_loop, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (n_ret) LISLAM_HIPCHK(c, hipMemcpyAsync(n_ret, d_nret, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (ret_id) LISLAM_HIPCHK(c, hipMemcpyAsync(ret_id, d_id, N * R * 4, hipMemcpyDeviceToHost, c->stream));
  if (ret_score) LISLAM_HIPCHK(c, hipMemcpyAsync(ret_score, d_score, N * R * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_score(lislam_bow* p, const int32_t* a, const int32_t* b, int32_t n_pairs, double* score) {
  if (!p || n_pairs < 0 || (n_pairs > 0 && (!a || !b))) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  for (int k = 0; k < n_pairs; k++)
    if (a[k] < 0 || a[k] >= p->n || b[k] < 0 || b[k] >= p->n)
      return fail(c, LISLAM_ERR_ARG, "lislam_bow_score: pair %d = (%d, %d) out of range (size %d)", k, a[k], b[k], p->n);
  if (n_pairs == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n_pairs;
  LISLAM_HIPCHK(c, p->res.reserve(N * 16, c->stream));
  double* d_score = p->res.as<double>();
  int* d_a = reinterpret_cast<int*>(d_score + N);
  int* d_b = d_a + N;
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_a, a, N * 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_b, b, N * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_bow_score, dim3((n_pairs + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, p->st, d_a, d_b,
                     n_pairs, d_score);
  LISLAM_HIPCHK(c, hipGetLastError());
  if (score) LISLAM_HIPCHK(c, hipMemcpyAsync(score, d_score, N * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_transform(lislam_bow* p, const void* desc, int32_t n, int32_t* word_id, double* weight) {
  if (!p || n < 0 || (n > 0 && !desc)) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (n > (1 << 24)) return fail(c, LISLAM_ERR_CAPACITY, "lislam_bow_transform: at most %d descriptors a call", 1 << 24);
  if (n == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  const size_t N = (size_t)n;
  LISLAM_HIPCHK(c, p->stage.reserve(N * 32, c->stream));
  LISLAM_HIPCHK(c, p->meta.reserve(16, c->stream));
  LISLAM_HIPCHK(c, p->res.reserve(N * 12, c->stream));
  double* d_wt = p->res.as<double>();
  int* d_word = reinterpret_cast<int*>(d_wt + N);
  int* d_cnt = p->meta.as<int>();
  const int cnt = n;
  LISLAM_HIPCHK(c, hipMemcpyAsync(d_cnt, &cnt, 4, hipMemcpyHostToDevice, c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(p->stage.p, desc, N * 32, hipMemcpyDefault, c->stream));
  const Source src{p->stage.as<const uint4>(), nullptr, d_cnt, 0, 1, n, n};
  launch_words(p, src, d_word, d_wt);
  LISLAM_HIPCHK(c, hipGetLastError());
  if (word_id) LISLAM_HIPCHK(c, hipMemcpyAsync(word_id, d_word, N * 4, hipMemcpyDeviceToHost, c->stream));
  if (weight) LISLAM_HIPCHK(c, hipMemcpyAsync(weight, d_wt, N * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

int lislam_bow_download(lislam_bow* p, int32_t what, int32_t index, void* dst, int32_t cap, int32_t* n) {
  if (!p || !dst || cap < 0) return LISLAM_ERR_ARG;
  lislam_ctx* c = p->ctx;
  if (index < 0 || index >= p->n)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_download: index %d out of range (size %d)", index, p->n);
  if (what != LISLAM_BOW_WORDS && what != LISLAM_BOW_VALUES)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_download: unknown output %d", what);
  hipSetDevice(c->device);
  int cnt = 0;
  LISLAM_HIPCHK(c, hipMemcpyAsync(&cnt, p->st.len + index, 4, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n) *n = cnt;
  if (cap < cnt) return fail(c, LISLAM_ERR_CAPACITY, "lislam_bow_download: %d elements, capacity %d", cnt, cap);
  if (cnt == 0) return LISLAM_OK;
  LISLAM_HIPCHK(c, p->res.reserve((size_t)p->F * 12, c->stream));
  double* d_v = p->res.as<double>();
  int* d_w = reinterpret_cast<int*>(d_v + p->F);
  hipLaunchKernelGGL(k_bow_gather, dim3((cnt + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, p->st, index, d_w, d_v);
  LISLAM_HIPCHK(c, hipGetLastError());
  if (what == LISLAM_BOW_WORDS) LISLAM_HIPCHK(c, hipMemcpyAsync(dst, d_w, (size_t)cnt * 4, hipMemcpyDeviceToHost, c->stream));
  else LISLAM_HIPCHK(c, hipMemcpyAsync(dst, d_v, (size_t)cnt * 8, hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  return LISLAM_OK;
}

}  // extern "C"

// ================================================================================================
// Vocabulary training (lislam_bow_trainer_*, lislam_bow_train): DBoW3's Vocabulary::create for binary
// descriptors, restated from the published library (rmsalinas/DBoW3 Vocabulary.cpp: HKmeansStep,
// initiateClustersKMpp, createWords, setNodeWeights; DescManip::meanValue).  Unpinned against the
// library like the rest of this file; tests/restate_bow_train.py is the same text in Python and the
// kernels are pinned against it by equality of bytes.
//
//   k_bowt_ingest     descriptors of a batch's scans into the trainer, image ids
//   k_bowt_locate     position -> node of the level (binary search over the segment starts)
//   k_bowt_seed       initiateClustersKMpp, one workgroup per node
//   k_bowt_assign     every descriptor to the first nearest centre of its node; counts the changes
//   k_bowt_means      meanValue: bit counts per (node, slot), one thread per bit plane and row group
//   k_bowt_majority   the threshold for nodes wider than one tile
//   k_bowt_tilecount / k_bowt_offsets / k_bowt_scatter   the stable partition of every segment by slot
//   k_bowt_ni         the images a word occurs in (setNodeWeights), deduplicated by a bitmap
//
// Semantics pinned here:
//  * HKmeansStep works on a node's descriptors in their original order (image, then row); every
//    partition below is stable.  <= k descriptors: each its own child, duplicates not merged.
//    Otherwise k-means++, then assign, then (means, assign) until an assignment equals the previous.
//  * Assignment: the first centre with the smallest Hamming distance, the minimum over the key
//    (distance << 8 | slot) as in k_bow_words.
//  * Mean: bit b is set iff at least n / 2 + n % 2 of the cluster's n descriptors have it set.
//  * k-means++: the first centre is the descriptor at a uniform index; each round min_d[i] =
//    min(min_d[i], d(i, newest centre)) where min_d[i] > 0, S = sum of min_d (plain distances, not
//    squares, as DBoW does); S == 0 stops with fewer than k centres; otherwise r uniform in [1, S] and
//    the first index whose inclusive prefix sum reaches r.  All integers (S < 2^31 for <= 2^23
//    descriptors), so the sums are exact in any order and a parallel scan gives the sequential answer.
//  * Children are created for every cluster, empty ones too; a child is clustered in turn if it holds
//    more than one descriptor and its level is below L.
//  * Node ids in DBoW3's order: a step appends all its children, then recurses into child 0, 1, ...
//    The renumbering from level order runs on the host (the tree is small).
//  * weight = log(N / Ni) in double, by the host's libm over the device's integer Ni.
// Ours, where DBoW3 cannot be followed:
//  * DBoW3 draws with rand() in depth-first visiting order, which a level-parallel trainer cannot
//    replay.  Draws here come from splitmix64 keyed by the node (include/lislam.h has the constants):
//    key(root) = splitmix64(seed), key(child c) = splitmix64(key ^ (c + 1)), draw j =
//    splitmix64(key + j * golden), reduced to [0, n) as ((x >> 32) * n) >> 32.
//  * An empty cluster keeps its centre (DBoW3's meanValue releases the Mat: undefined).
//  * A node stops after max_iterations assignments, the seeding's being the first (DBoW3 has no
//    limit; a device loop on a shared machine needs one).
//  * A converged node is a fixed point of (means, assign), so all nodes of a level iterate together
//    until none changes, and that equals the per-node loops.
#include <chrono>
#include <utility>

namespace lislam {
namespace bowt {

using bow::kThreads;
using bow::popc4;
constexpr int kTile = 2048;        // positions per tile of k_bowt_means and of the partition
constexpr int kSlotPass = 32;      // slots whose bit counts k_bowt_means holds in LDS at once (32 KB)
constexpr int kMeansThreads = 1024; // k_bowt_means: 4 row groups x 256 bit planes
constexpr int kStageRows = 512;    // rows k_bowt_means stages in LDS at a time
constexpr int kSeedWide = 16384;   // a level with a node above this many descriptors seeds with 1024 threads
constexpr size_t kBitmapBytes = 64u << 20;

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + kGolden;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t draw(uint64_t key, int j) { return splitmix64(key + (uint64_t)j * kGolden); }
__host__ __device__ inline uint32_t reduce_to(uint64_t x, uint32_t n) { return (uint32_t)(((x >> 32) * (uint64_t)n) >> 32); }

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// The nodes of one level that are clustered (A of them, in the order of their segments).
struct Level {
  const int* start;      // [A] first position of the node's segment in perm
  const int* cnt;        // [A] its descriptors (>= 1)
  const uint64_t* key;   // [A] generator key
  const int* coff;       // [A] first centre row: sum of min(cnt, k) of the nodes before
  const int* tile0;      // [A] first tile
  const int* big;        // [A] index of the global bit counters (cnt > kTile and > k), else -1
  int* ncent;            // [A] out: centres = children
  int* last;             // [A] out: the last iteration whose assignment changed (0: no k-means)
  uint32_t* centre;      // [rows][8]
  int A, k;
};
struct Work {
  const uint4* desc;     // [n][2] the trainer's descriptors, original order
  const int* perm;       // [n] descriptor index, segmented by node
  int* perm_out;
  uint8_t* slot;         // [n] by position
  int* mind;             // [n] by position
  int* node_of;          // [n] by position: node of the level or -1
  int n;
};
struct Tiles {
  const int2* tile;      // [T] (node, offset inside its segment)
  const int* toff;       // [T] first row of the tile's slot counts
  int* tcount;           // [rows] per tile and slot: members, then (k_bowt_offsets) output offsets
  int* childcnt;         // by coff: members per (node, slot)
  int T;
};

// One workgroup per image: its id for rows [dst_off[k], dst_off[k + 1]) and, from a batch (src: image k's
// rows start at row k * src_stride), the rows themselves.
__global__ __launch_bounds__(kThreads) void k_bowt_ingest(const uint4* __restrict__ src, long long src_stride,
                                                          const int* __restrict__ dst_off, int image0,
                                                          uint4* __restrict__ desc, int* __restrict__ img_of) {
  const int k = blockIdx.x;
  const int off = dst_off[k], c = dst_off[k + 1] - off;
  for (int i = threadIdx.x; i < c; i += kThreads) img_of[off + i] = image0 + k;
  if (!src) return;
  const uint4* s = src + (size_t)k * src_stride * 2;
  for (int i = threadIdx.x; i < c * 2; i += kThreads) desc[(size_t)off * 2 + i] = s[i];
}

__global__ __launch_bounds__(kThreads) void k_bowt_locate(Level lv, Work w) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= w.n) return;
  int lo = 0, hi = lv.A;  // the last node with start <= p
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (lv.start[mid] <= p) lo = mid; else hi = mid;
  }
  const int s = lv.start[lo];
  w.node_of[p] = (p >= s && p < s + lv.cnt[lo]) ? lo : -1;
}

// One workgroup per node.  Wave v owns a contiguous range of the segment and reads it lane by lane
// (coalesced); the waves' sums, scanned over the workgroup, name the wave in whose range the inclusive
// prefix reaches r, and that wave walks its range 64 positions at a time with a wave scan and a ballot
// for the first such index.  Integers throughout: the same index as the sequential prefix sum.
template <int T>
__global__ __launch_bounds__(T) void k_bowt_seed(Level lv, Work w) {
  constexpr int kWaves = T / 64;
  __shared__ int wsum[kWaves];
  __shared__ int pick_s;
  const int a = blockIdx.x, tid = threadIdx.x, k = lv.k;
  const int s = lv.start[a], n = lv.cnt[a];
  uint4* cen = reinterpret_cast<uint4*>(lv.centre) + (size_t)lv.coff[a] * 2;
  if (n <= k) {  // each descriptor its own child
    for (int i = tid; i < n; i += T) {
      const size_t row = (size_t)w.perm[s + i];
      cen[i * 2] = w.desc[row * 2];
      cen[i * 2 + 1] = w.desc[row * 2 + 1];
      w.slot[s + i] = (uint8_t)i;
    }
    if (tid == 0) { lv.ncent[a] = n; lv.last[a] = 0; }
    return;
  }
  const uint64_t key = lv.key[a];
  const int lane = lane_id(), wv = tid >> 6;
  const int per_wave = ((n + kWaves - 1) / kWaves + 63) & ~63;
  const int lo = min(wv * per_wave, n), hi = min(lo + per_wave, n);
  int idx = (int)reduce_to(draw(key, 0), (uint32_t)n);
  int nc = 0;
  for (;;) {  // uniform over the workgroup
    const size_t crow = (size_t)w.perm[s + idx];
    const uint4 c0 = w.desc[crow * 2], c1 = w.desc[crow * 2 + 1];
    if (tid == 0) { cen[nc * 2] = c0; cen[nc * 2 + 1] = c1; }
    nc++;
    if (nc == k) break;
    int local = 0;
#pragma unroll 4
    for (int p = lo + lane; p < hi; p += 64) {
      const size_t row = (size_t)w.perm[s + p];
      const int d = popc4(w.desc[row * 2], c0) + popc4(w.desc[row * 2 + 1], c1);
      int m = d;
      if (nc > 1) {
        m = w.mind[s + p];
        if (m > 0) m = min(m, d);
      }
      w.mind[s + p] = m;
      local += m;
    }
    const int mine = __shfl(wave_inclusive_sum(local), 63);  // this wave's sum
    if (lane == 0) wsum[wv] = mine;
    __syncthreads();
    int base = 0, S = 0;
#pragma unroll
    for (int q = 0; q < kWaves; q++) {
      const int v = wsum[q];
      if (q < wv) base += v;
      S += v;
    }
    if (S == 0) break;
    const int r = 1 + (int)reduce_to(draw(key, nc), (uint32_t)S);
    if (base < r && r <= base + mine) {  // exactly one wave, all its lanes
      int run = base;
      for (int p0 = lo; p0 < hi; p0 += 64) {
        const int p = p0 + lane;
        const int inc = wave_inclusive_sum(p < hi ? w.mind[s + p] : 0);
        const uint64_t hit = __ballot(run + inc >= r);
        if (hit != 0) {
          if (lane == 0) pick_s = p0 + __ffsll((unsigned long long)hit) - 1;
          break;
        }
        run += __shfl(inc, 63);
      }
    }
    __syncthreads();
    idx = pick_s;
    __syncthreads();  // wsum and pick_s are written again in the next round
  }
  if (tid == 0) { lv.ncent[a] = nc; lv.last[a] = 1; }
}

// One lane per position: the descriptor in 8 registers, the node's centres through the cache (a wave
// mostly lies inside one node, so its lanes read the same rows).
__global__ __launch_bounds__(kThreads) void k_bowt_assign(Level lv, Work w, int iteration, int* __restrict__ changed) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  bool ch = false;
  int a = -1;
  if (p < w.n) {
    a = w.node_of[p];
    if (a >= 0 && lv.cnt[a] > lv.k) {
      const size_t row = (size_t)w.perm[p];
      const uint4 d0 = w.desc[row * 2], d1 = w.desc[row * 2 + 1];
      const uint4* cen = reinterpret_cast<const uint4*>(lv.centre) + (size_t)lv.coff[a] * 2;
      const int nc = lv.ncent[a];
      uint32_t best = 0xffffffffu;
      for (int c = 0; c < nc; c++)
        best = min(best, ((uint32_t)(popc4(d0, cen[c * 2]) + popc4(d1, cen[c * 2 + 1])) << 8) | (uint32_t)c);
      const uint8_t sl = (uint8_t)(best & 0xffu);
      ch = iteration > 1 && w.slot[p] != sl;
      w.slot[p] = sl;
    }
  }
  // one atomic per wave for the level's count, one per node the wave's changed lanes lie in
  const uint64_t m = __ballot(ch);
  if (m == 0) return;
  const int lane = lane_id();
  if (lane == __ffsll((unsigned long long)m) - 1) atomicAdd(changed, __popcll(m));
  uint64_t rest = m;
  while (rest != 0) {  // wave-uniform
    const int leader = __ffsll((unsigned long long)rest) - 1;
    const int a0 = __shfl(a, leader);
    if (lane == leader) atomicMax(&lv.last[a0], iteration);
    rest &= ~__ballot(ch && a == a0);
  }
}

// Bit b of centre (row) <- counts[b] >= N2, threads 0..255: a wave's ballot is two words of the row.
__device__ __forceinline__ void majority_row(uint32_t* centre_row, uint32_t count_b, uint32_t members) {
  const uint32_t n2 = members / 2 + members % 2;
  const uint64_t m = __ballot(count_b >= n2);
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    centre_row[wv * 2] = (uint32_t)m;
    centre_row[wv * 2 + 1] = (uint32_t)(m >> 32);
  }
}

// One workgroup of 1,024 threads per tile of <= kTile positions of one node: thread (g, b) owns bit plane
// b of the rows q = g mod 4.  The tile's descriptors are staged 512 at a time in LDS; a thread reads row
// q's slot and the word that holds its bit (both broadcasts) and adds the bit to counter [slot][b] with
// an LDS integer add that returns nothing, so nothing waits for it; only the four row groups ever meet
// on a counter.  Integer sums: exact in any order.  A node of one tile takes its majority here; a wider
// one adds its counters to the node's global ones (integer atomics) and k_bowt_majority finishes it.
__global__ __launch_bounds__(kMeansThreads) void k_bowt_means(Level lv, Work w, Tiles tl, uint32_t* __restrict__ gcount) {
  __shared__ uint32_t cnt[kSlotPass][kThreads];
  __shared__ uint32_t stage[kStageRows][9];  // 8 words + 1: the staging writes spread over the banks
  __shared__ int sl[kStageRows];
  __shared__ uint32_t members[kSlotPass];
  const int2 t = tl.tile[blockIdx.x];
  const int a = t.x, k = lv.k, tid = threadIdx.x, b = tid & (kThreads - 1), g = tid / kThreads;
  const int n = lv.cnt[a];
  if (n <= k) return;  // uniform
  const int s = lv.start[a] + t.y, m = min(kTile, n - t.y), nc = lv.ncent[a], big = lv.big[a];
  const int wi = b >> 5, bit = b & 31;
  for (int s0 = 0; s0 < nc; s0 += kSlotPass) {
    for (int q = g; q < kSlotPass; q += kMeansThreads / kThreads) cnt[q][b] = 0;
    if (tid < kSlotPass) members[tid] = 0;
    uint32_t mine = 0;  // rows of slot s0 + b among this thread's
    for (int j0 = 0; j0 < m; j0 += kStageRows) {
      __syncthreads();
      const int j = j0 + tid;
      if (tid < kStageRows && j < m) {
        const size_t row = (size_t)w.perm[s + j];
        const uint4 d0 = w.desc[row * 2], d1 = w.desc[row * 2 + 1];
        stage[tid][0] = d0.x; stage[tid][1] = d0.y; stage[tid][2] = d0.z; stage[tid][3] = d0.w;
        stage[tid][4] = d1.x; stage[tid][5] = d1.y; stage[tid][6] = d1.z; stage[tid][7] = d1.w;
        sl[tid] = (int)w.slot[s + j] - s0;
      }
      __syncthreads();
      const int lim = min(kStageRows, m - j0);
#pragma unroll 8
      for (int q = g; q < lim; q += kMeansThreads / kThreads) {
        const int sq = sl[q];
        const bool in_pass = (unsigned)sq < (unsigned)kSlotPass;  // no branch: a row of another pass adds 0
        const uint32_t v = in_pass ? (stage[q][wi] >> bit) & 1u : 0u;
        __hip_atomic_fetch_add(&cnt[in_pass ? sq : 0][b], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        mine += sq == b ? 1u : 0u;
      }
    }
    if (b < kSlotPass && mine) atomicAdd(&members[b], mine);
    __syncthreads();
    const int ns = min(kSlotPass, nc - s0);
    if (g == 0) {  // four whole waves
      if (big < 0) {
        for (int q = 0; q < ns; q++)
          if (members[q] > 0)  // an empty cluster keeps its centre
            majority_row(lv.centre + ((size_t)lv.coff[a] + s0 + q) * 8, cnt[q][b], members[q]);
      } else {
        uint32_t* gc = gcount + ((size_t)big * k + s0) * (kThreads + 1);
        for (int q = 0; q < ns; q++)
          if (cnt[q][b]) atomicAdd(&gc[(size_t)q * (kThreads + 1) + b], cnt[q][b]);
        if (b < ns && members[b]) atomicAdd(&gc[(size_t)b * (kThreads + 1) + kThreads], members[b]);
      }
    }
    __syncthreads();
  }
}

// grid (k, wide nodes)
__global__ __launch_bounds__(kThreads) void k_bowt_majority(Level lv, const int* __restrict__ big_node,
                                                            const uint32_t* __restrict__ gcount) {
  const int a = big_node[blockIdx.y], c = blockIdx.x;
  if (c >= lv.ncent[a]) return;
  const uint32_t* g = gcount + ((size_t)blockIdx.y * lv.k + c) * (kThreads + 1);
  const uint32_t members = g[kThreads];
  if (members == 0) return;
  majority_row(lv.centre + ((size_t)lv.coff[a] + c) * 8, g[threadIdx.x], members);
}

// ---- the stable partition of every segment by slot: members per (tile, slot); per node the output
// offset of every (tile, slot), slot-major; per tile the ranks in order.
__global__ __launch_bounds__(kThreads) void k_bowt_tilecount(Level lv, Work w, Tiles tl) {
  __shared__ int hist[64];
  const int2 t = tl.tile[blockIdx.x];
  const int a = t.x, n = lv.cnt[a];
  const int s = lv.start[a] + t.y, m = min(kTile, n - t.y), kk = min(n, lv.k);
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += kThreads) atomicAdd(&hist[w.slot[s + j] & 63], 1);
  __syncthreads();
  if ((int)threadIdx.x < kk) tl.tcount[tl.toff[blockIdx.x] + threadIdx.x] = hist[threadIdx.x];
}

// One wave per node, lane = slot.
__global__ __launch_bounds__(64) void k_bowt_offsets(Level lv, Tiles tl) {
  const int a = blockIdx.x, c = threadIdx.x, n = lv.cnt[a];
  const int kk = min(n, lv.k), nt = (n + kTile - 1) / kTile, t0 = lv.tile0[a];
  int total = 0;
  if (c < kk)
    for (int t = 0; t < nt; t++) total += tl.tcount[tl.toff[t0 + t] + c];
  int run = wave_inclusive_sum(total) - total;  // the members of the slots before
  if (c < kk) {
    tl.childcnt[lv.coff[a] + c] = total;
    for (int t = 0; t < nt; t++) {
      const int i = tl.toff[t0 + t] + c, v = tl.tcount[i];
      tl.tcount[i] = run;
      run += v;
    }
  }
}

// One workgroup per tile: thread c walks the tile's slots in order and numbers the members of slot c.
__global__ __launch_bounds__(kThreads) void k_bowt_scatter(Level lv, Work w, Tiles tl) {
  __shared__ uint8_t sl[kTile];
  __shared__ int rank[kTile];
  const int2 t = tl.tile[blockIdx.x];
  const int a = t.x, n = lv.cnt[a];
  const int s0 = lv.start[a], s = s0 + t.y, m = min(kTile, n - t.y), kk = min(n, lv.k);
  for (int j = threadIdx.x; j < m; j += kThreads) sl[j] = w.slot[s + j];
  __syncthreads();
  if ((int)threadIdx.x < kk) {
    int run = tl.tcount[tl.toff[blockIdx.x] + threadIdx.x];
    for (int j = 0; j < m; j++)
      if (sl[j] == threadIdx.x) rank[j] = run++;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += kThreads) w.perm_out[s0 + rank[j]] = w.perm[s + j];
}

// Ni: descriptor i of image img_of[i] in [m0, m1) sets bit (image, word); the first to set it counts.
__global__ __launch_bounds__(kThreads) void k_bowt_ni(const int* __restrict__ words, const int* __restrict__ img_of, int i0,
                                                      int i1, int m0, int row_words, uint32_t* __restrict__ bitmap,
                                                      int* __restrict__ ni) {
  const int i = i0 + blockIdx.x * kThreads + threadIdx.x;
  if (i >= i1) return;
  const int wd = words[i];
  if (wd < 0) return;
  const uint32_t bit = 1u << (wd & 31);
  const uint32_t old = atomicOr(&bitmap[(size_t)(img_of[i] - m0) * row_words + (wd >> 5)], bit);
  if (!(old & bit)) atomicAdd(&ni[wd], 1);
}

}  // namespace bowt
}  // namespace lislam

using namespace lislam::bowt;

namespace {
struct HostNode {  // level order: the children of a node are consecutive, in slot order
  int parent, first_child = 0, n_child = 0;
  uint8_t desc[32];
};
}  // namespace

struct lislam_bow_trainer {
  lislam_ctx* ctx = nullptr;
  int cap_images = 0, cap_desc = 0, n_images = 0, n_desc = 0;
  std::vector<int> img_off{0};  // [n_images + 1] first descriptor of every image
  void* desc = nullptr;         // [cap_desc][32]
  void* img_of = nullptr;       // [cap_desc] int
  DBuf meta, perm, slot, mind, node_of, lvl, centre, tiles, tcount, childcnt, gcount, scalars, tree, words, bitmap;
  bool trained = false;
  std::vector<int32_t> parent;
  std::vector<uint8_t> descriptor;
  std::vector<double> weight;
};

namespace {

void free_trainer(lislam_bow_trainer* t) {
  if (t->desc) (void)hipFree(t->desc);
  if (t->img_of) (void)hipFree(t->img_of);
  delete t;
}

// Room for n_images more images of `total` descriptors?
int check_room(lislam_bow_trainer* t, const char* who, int n_images, int64_t total) {
  if ((int64_t)t->n_images + n_images > t->cap_images)
    return fail(t->ctx, LISLAM_ERR_CAPACITY, "%s: %d + %d images exceed the capacity %d", who, t->n_images, n_images,
                t->cap_images);
  if ((int64_t)t->n_desc + total > t->cap_desc)
    return fail(t->ctx, LISLAM_ERR_CAPACITY, "%s: %d + %lld descriptors exceed the capacity %d", who, t->n_desc,
                (long long)total, t->cap_desc);
  return LISLAM_OK;
}

// Image ids (and, from src, the rows) of n_images images of the given clamped counts, appended.
int ingest(lislam_bow_trainer* t, const uint4* src, long long src_stride, const std::vector<int>& counts) {
  lislam_ctx* c = t->ctx;
  const int n_images = (int)counts.size();
  std::vector<int> off(n_images + 1);
  off[0] = t->n_desc;
  for (int k = 0; k < n_images; k++) off[k + 1] = off[k] + counts[k];
  LISLAM_HIPCHK(c, t->meta.reserve((size_t)(n_images + 1) * sizeof(int), c->stream));
  LISLAM_HIPCHK(c, hipMemcpyAsync(t->meta.p, off.data(), (size_t)(n_images + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_bowt_ingest, dim3(n_images), dim3(kThreads), 0, c->stream, src, src_stride,
                     static_cast<const int*>(t->meta.p), t->n_images, static_cast<uint4*>(t->desc), static_cast<int*>(t->img_of));
  LISLAM_HIPCHK(c, hipGetLastError());
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));  // off leaves scope; the next call may reuse meta
  for (int k = 0; k < n_images; k++) t->img_off.push_back(off[k + 1]);
  t->n_images += n_images;
  t->n_desc = off[n_images];
  return LISLAM_OK;
}

}  // namespace

extern "C" {

int lislam_bow_trainer_create(lislam_ctx* c, int32_t cap_images, int32_t cap_descriptors, lislam_bow_trainer** out) {
  if (!c || !out) return LISLAM_ERR_ARG;
  *out = nullptr;
  if (cap_images < 1 || cap_descriptors < 1)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_trainer_create: cap_images >= 1 and cap_descriptors >= 1");
  if (cap_descriptors > LISLAM_BOW_TRAIN_MAX_DESCRIPTORS)
    return fail(c, LISLAM_ERR_CAPACITY, "lislam_bow_trainer_create: at most %d descriptors", LISLAM_BOW_TRAIN_MAX_DESCRIPTORS);
  hipSetDevice(c->device);
  lislam_bow_trainer* t = new lislam_bow_trainer();
  t->ctx = c;
  t->cap_images = cap_images;
  t->cap_desc = cap_descriptors;
  if (hipMalloc(&t->desc, (size_t)cap_descriptors * 32) != hipSuccess ||
      hipMalloc(&t->img_of, (size_t)cap_descriptors * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    free_trainer(t);
    return fail(c, LISLAM_ERR_DEVICE, "lislam_bow_trainer_create: device allocation failed");
  }
  *out = t;
  return LISLAM_OK;
}

int lislam_bow_trainer_destroy(lislam_bow_trainer* t) {
  if (!t) return LISLAM_ERR_ARG;
  hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  free_trainer(t);
  return LISLAM_OK;
}

int lislam_bow_trainer_size(lislam_bow_trainer* t, int32_t* n_images, int32_t* n_descriptors) {
  if (!t) return LISLAM_ERR_ARG;
  if (n_images) *n_images = t->n_images;
  if (n_descriptors) *n_descriptors = t->n_desc;
  return LISLAM_OK;
}

int lislam_bow_trainer_add(lislam_bow_trainer* t, const void* desc, const int32_t* counts, int32_t n_images) {
  if (!t || n_images < 0 || (n_images > 0 && !counts)) return LISLAM_ERR_ARG;
  lislam_ctx* c = t->ctx;
  if (n_images == 0) return LISLAM_OK;
  int64_t total = 0;
  for (int k = 0; k < n_images; k++) {
    if (counts[k] < 0) return fail(c, LISLAM_ERR_ARG, "lislam_bow_trainer_add: counts[%d] = %d", k, counts[k]);
    total += counts[k];
  }
  if (total > 0 && !desc) return fail(c, LISLAM_ERR_ARG, "lislam_bow_trainer_add: null descriptors");
  int rc;
  if ((rc = check_room(t, "lislam_bow_trainer_add", n_images, total))) return rc;
  hipSetDevice(c->device);
  if (total)
    LISLAM_HIPCHK(c, hipMemcpyAsync(static_cast<uint8_t*>(t->desc) + (size_t)t->n_desc * 32, desc, (size_t)total * 32, hipMemcpyDefault,
                                    c->stream));
  return ingest(t, nullptr, 0, std::vector<int>(counts, counts + n_images));
}

int lislam_bow_trainer_add_batch(lislam_bow_trainer* t, lislam_batch* b, int32_t first_scan, int32_t n_scans) {
  if (!t || !b) return LISLAM_ERR_ARG;
  lislam_ctx* c = t->ctx;
  const char* who = "lislam_bow_trainer_add_batch";
  LISLAM_RC(check_same_context(c, who, b));
  LISLAM_RC(check_scan_range(c, who, b, first_scan, n_scans));
  OrbDescriptors o;
  LISLAM_RC(orb_descriptors(c, who, b, first_scan + n_scans, &o));
  if (n_scans == 0) return LISLAM_OK;
  hipSetDevice(c->device);
  // the counts decide how much room the scans take: read them (a scan keeps at most nfeatures rows)
  std::vector<int> cnt(n_scans);
  LISLAM_HIPCHK(c, hipMemcpyAsync(cnt.data(), o.counts + first_scan, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  int64_t total = 0;
  for (int& v : cnt) {
    v = std::max(0, std::min(v, std::min(o.nfeatures, o.cap)));
    total += v;
  }
  LISLAM_RC(check_room(t, who, n_scans, total));
  return ingest(t, reinterpret_cast<const uint4*>(o.desc + (size_t)first_scan * o.cap * 32), o.cap, cnt);
}

int lislam_bow_train(lislam_bow_trainer* t, const lislam_bow_train_config* cfg, int32_t* n_nodes_out,
                     lislam_bow_train_stats* stats) {
  if (!t) return LISLAM_ERR_ARG;
  lislam_ctx* c = t->ctx;
  lislam_bow_train_config d = {10, 5, 100, 0};
  if (cfg) d = *cfg;
  if (d.k < 2 || d.k > kMaxChildren || d.L < 1 || d.L > LISLAM_BOW_TRAIN_MAX_L || d.max_iterations < 1)
    return fail(c, LISLAM_ERR_ARG, "lislam_bow_train: k 2..%d, L 1..%d, max_iterations >= 1 (got %d, %d, %d)", kMaxChildren,
                LISLAM_BOW_TRAIN_MAX_L, d.k, d.L, d.max_iterations);
  hipSetDevice(c->device);
  using clk = std::chrono::steady_clock;
  const auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  lislam_bow_train_stats st{};
  const auto t_call = clk::now();
  const bool profile = stats && stats->profile;
  st.profile = profile;
  const int n = t->n_desc, k = d.k;
  std::vector<HostNode> nodes(1);
  nodes[0].parent = -1;
  memset(nodes[0].desc, 0, 32);
  int rc;
  // never a null buffer, whatever the size
  const auto room = [c](DBuf& b, size_t want) { return b.reserve(std::max<size_t>(want, 16), c->stream); };
  LISLAM_HIPCHK(c, room(t->perm, (size_t)n * 2 * sizeof(int)));
  LISLAM_HIPCHK(c, room(t->slot, (size_t)n));
  LISLAM_HIPCHK(c, room(t->mind, (size_t)n * sizeof(int)));
  LISLAM_HIPCHK(c, room(t->node_of, (size_t)n * sizeof(int)));
  LISLAM_HIPCHK(c, room(t->scalars, 16));
  int* perm_a = static_cast<int*>(t->perm.p);
  int* perm_b = perm_a + n;
  int* d_changed = static_cast<int*>(t->scalars.p);
  {
    std::vector<int> iota(n);
    for (int i = 0; i < n; i++) iota[i] = i;
    if (n) LISLAM_HIPCHK(c, hipMemcpyAsync(perm_a, iota.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // the nodes to cluster at this level, in the order of their segments
  std::vector<int> a_start, a_cnt, a_node;
  std::vector<uint64_t> a_key;
  if (n > 0) {
    a_start.push_back(0);
    a_cnt.push_back(n);
    a_node.push_back(0);
    a_key.push_back(splitmix64(d.seed));
  }
  int depth = 0;
  for (int level = 1; level <= d.L && !a_start.empty(); level++) {
    const auto t_level = clk::now();
    auto t_phase = clk::now();
    const auto phase = [&](int which) -> int {  // with profile: wait, and book the time since the last phase ended
      if (!profile) return LISLAM_OK;
      LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
      st.phase_ms[level - 1][which] += ms_since(t_phase);
      t_phase = clk::now();
      return LISLAM_OK;
    };
    const int A = (int)a_start.size();
    depth = level;
    // per node: centre rows, tiles, wide-node counters
    std::vector<int> coff(A + 1, 0), tile0(A), big(A, -1), big_node, toff;
    std::vector<int2> tile;
    int n_kmeans = 0, max_cnt = 0;
    for (int a = 0; a < A; a++) {
      const int kk = std::min(a_cnt[a], k);
      coff[a + 1] = coff[a] + kk;
      tile0[a] = (int)tile.size();
      for (int o = 0; o < a_cnt[a]; o += kTile) {
        toff.push_back(toff.empty() ? 0 : toff.back() + std::min(a_cnt[tile.back().x], k));
        tile.push_back(make_int2(a, o));
      }
      if (a_cnt[a] > k) {
        n_kmeans++;
        if (a_cnt[a] > kTile) {
          big[a] = (int)big_node.size();
          big_node.push_back(a);
        }
      }
      max_cnt = std::max(max_cnt, a_cnt[a]);
    }
    const int T = (int)tile.size(), rows = coff[A], B = (int)big_node.size();
    const size_t trows = (size_t)toff.back() + std::min(a_cnt[tile.back().x], k);
    // the level's arrays in one buffer: key | start cnt coff tile0 big ncent last big_node toff | tile
    const size_t lvl_bytes = (size_t)A * 8 + ((size_t)A * 7 + B + T) * 4 + (size_t)T * 8 + 64;
    const size_t gbytes = (size_t)B * k * (kThreads + 1) * sizeof(uint32_t);
    LISLAM_HIPCHK(c, room(t->lvl, lvl_bytes));
    LISLAM_HIPCHK(c, room(t->centre, (size_t)rows * 32));
    LISLAM_HIPCHK(c, room(t->tcount, trows * sizeof(int)));
    LISLAM_HIPCHK(c, room(t->childcnt, (size_t)rows * sizeof(int)));
    LISLAM_HIPCHK(c, room(t->gcount, gbytes));
    uint64_t* d_key = static_cast<uint64_t*>(t->lvl.p);
    int2* d_tile = reinterpret_cast<int2*>(d_key + A);
    int* d_start = reinterpret_cast<int*>(d_tile + T);
    int *d_cnt = d_start + A, *d_coff = d_cnt + A, *d_tile0 = d_coff + A, *d_big = d_tile0 + A, *d_ncent = d_big + A,
        *d_last = d_ncent + A, *d_big_node = d_last + A, *d_toff = d_big_node + B;
    const auto up = [&](void* dst, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    LISLAM_HIPCHK(c, up(d_key, a_key.data(), (size_t)A * 8));
    LISLAM_HIPCHK(c, up(d_tile, tile.data(), (size_t)T * 8));
    LISLAM_HIPCHK(c, up(d_start, a_start.data(), (size_t)A * 4));
    LISLAM_HIPCHK(c, up(d_cnt, a_cnt.data(), (size_t)A * 4));
    LISLAM_HIPCHK(c, up(d_coff, coff.data(), (size_t)A * 4));
    LISLAM_HIPCHK(c, up(d_tile0, tile0.data(), (size_t)A * 4));
    LISLAM_HIPCHK(c, up(d_big, big.data(), (size_t)A * 4));
    LISLAM_HIPCHK(c, up(d_big_node, big_node.data(), (size_t)B * 4));
    LISLAM_HIPCHK(c, up(d_toff, toff.data(), (size_t)T * 4));
    const Level lv{d_start, d_cnt, d_key, d_coff, d_tile0, d_big, d_ncent, d_last, static_cast<uint32_t*>(t->centre.p), A, k};
    const Work w{static_cast<const uint4*>(t->desc), perm_a, perm_b, static_cast<uint8_t*>(t->slot.p), static_cast<int*>(t->mind.p),
                 static_cast<int*>(t->node_of.p), n};
    const Tiles tl{d_tile, d_toff, static_cast<int*>(t->tcount.p), static_cast<int*>(t->childcnt.p), T};
    const dim3 flat((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_bowt_locate, flat, dim3(kThreads), 0, c->stream, lv, w);
    if (max_cnt > kSeedWide) hipLaunchKernelGGL(k_bowt_seed<1024>, dim3(A), dim3(1024), 0, c->stream, lv, w);
    else hipLaunchKernelGGL(k_bowt_seed<kThreads>, dim3(A), dim3(kThreads), 0, c->stream, lv, w);
    LISLAM_HIPCHK(c, hipGetLastError());
    if ((rc = phase(LISLAM_BOW_PHASE_SEED))) return rc;
    if (n_kmeans) {
      hipLaunchKernelGGL(k_bowt_assign, flat, dim3(kThreads), 0, c->stream, lv, w, 1, d_changed);
      if ((rc = phase(LISLAM_BOW_PHASE_ASSIGN))) return rc;
      for (int it = 2; it <= d.max_iterations; it++) {  // bounded by the cap; the host reads the level's "changed" word
        LISLAM_HIPCHK(c, hipMemsetAsync(d_changed, 0, sizeof(int), c->stream));
        if (B) LISLAM_HIPCHK(c, hipMemsetAsync(t->gcount.p, 0, gbytes, c->stream));
        hipLaunchKernelGGL(k_bowt_means, dim3(T), dim3(kMeansThreads), 0, c->stream, lv, w, tl, static_cast<uint32_t*>(t->gcount.p));
        if (B)
          hipLaunchKernelGGL(k_bowt_majority, dim3(k, B), dim3(kThreads), 0, c->stream, lv, d_big_node,
                             static_cast<const uint32_t*>(t->gcount.p));
        if ((rc = phase(LISLAM_BOW_PHASE_MEANS))) return rc;
        hipLaunchKernelGGL(k_bowt_assign, flat, dim3(kThreads), 0, c->stream, lv, w, it, d_changed);
        LISLAM_HIPCHK(c, hipGetLastError());
        int changed = 0;
        LISLAM_HIPCHK(c, hipMemcpyAsync(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = phase(LISLAM_BOW_PHASE_ASSIGN))) return rc;
        if (changed == 0) break;
      }
    }
    hipLaunchKernelGGL(k_bowt_tilecount, dim3(T), dim3(kThreads), 0, c->stream, lv, w, tl);
    hipLaunchKernelGGL(k_bowt_offsets, dim3(A), dim3(64), 0, c->stream, lv, tl);
    hipLaunchKernelGGL(k_bowt_scatter, dim3(T), dim3(kThreads), 0, c->stream, lv, w, tl);
    LISLAM_HIPCHK(c, hipGetLastError());
    // only the segments clustered at this level are written to the other buffer: every later level reads
    // inside them, never the positions of a node that is finished
    std::vector<int> ncent(A), last(A), childcnt(rows);
    std::vector<uint8_t> centre((size_t)rows * 32);
    LISLAM_HIPCHK(c, hipMemcpyAsync(ncent.data(), d_ncent, (size_t)A * 4, hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipMemcpyAsync(last.data(), d_last, (size_t)A * 4, hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipMemcpyAsync(childcnt.data(), t->childcnt.p, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipMemcpyAsync(centre.data(), t->centre.p, (size_t)rows * 32, hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = phase(LISLAM_BOW_PHASE_PARTITION))) return rc;
    std::swap(perm_a, perm_b);
    std::vector<int> n_start, n_cnt, n_node;
    std::vector<uint64_t> n_key;
    st.level_steps[level - 1] = A;
    st.level_clustered[level - 1] = n_kmeans;
    for (int a = 0; a < A; a++) {
      if (a_cnt[a] > k) {
        st.level_iterations[level - 1] = std::max(st.level_iterations[level - 1], std::min(last[a] + 1, d.max_iterations));
        st.level_capped[level - 1] += last[a] == d.max_iterations;
      }
      nodes[a_node[a]].first_child = (int)nodes.size();
      nodes[a_node[a]].n_child = ncent[a];
      int at = a_start[a];
      for (int s = 0; s < ncent[a]; s++) {
        HostNode hn;
        hn.parent = a_node[a];
        memcpy(hn.desc, &centre[((size_t)coff[a] + s) * 32], 32);
        const int cc = childcnt[coff[a] + s];
        if (level < d.L && cc > 1) {
          n_start.push_back(at);
          n_cnt.push_back(cc);
          n_node.push_back((int)nodes.size());
          n_key.push_back(splitmix64(a_key[a] ^ (uint64_t)(s + 1)));
        }
        at += cc;
        nodes.push_back(hn);
      }
    }
    a_start.swap(n_start);
    a_cnt.swap(n_cnt);
    a_node.swap(n_node);
    a_key.swap(n_key);
    st.level_ms[level - 1] = ms_since(t_level);
    st.n_levels = level;
  }
  // DBoW3's ids: a step appends all its children, then recurses into child 0, child 1, ...
  const int N = (int)nodes.size();
  std::vector<int> new_id(N, 0), order;  // order: level-order index by new id
  order.reserve(N);
  order.push_back(0);
  {
    std::vector<std::pair<int, int>> stack;  // (node, next child to recurse into)
    const auto append = [&](int q) {
      for (int s = 0; s < nodes[q].n_child; s++) {
        new_id[nodes[q].first_child + s] = (int)order.size();
        order.push_back(nodes[q].first_child + s);
      }
      stack.emplace_back(q, 0);
    };
    append(0);
    while (!stack.empty()) {
      auto& top = stack.back();
      if (top.second >= nodes[top.first].n_child) {
        stack.pop_back();
        continue;
      }
      const int ch = nodes[top.first].first_child + top.second++;
      if (nodes[ch].n_child) append(ch);
    }
  }
  t->trained = false;  // until the weights are in
  t->parent.assign(N, -1);
  t->descriptor.assign((size_t)N * 32, 0);
  t->weight.assign(N, 0.0);
  for (int i = 0; i < N; i++) {
    const HostNode& hn = nodes[order[i]];
    t->parent[i] = hn.parent < 0 ? -1 : new_id[hn.parent];
    memcpy(&t->descriptor[(size_t)i * 32], hn.desc, 32);
  }
  // createWords: a leaf's word id is its rank among leaves in ascending id
  std::vector<int> word_node;  // new id of every word
  std::vector<int> word_of(N, -1);
  for (int i = 0; i < N; i++)
    if (nodes[order[i]].n_child == 0) {
      word_of[order[i]] = (int)word_node.size();
      word_node.push_back(i);
    }
  const int n_words = N > 1 ? (int)word_node.size() : 0;
  st.n_nodes = N;
  st.n_words = n_words;
  const auto t_weights = clk::now();
  if (N > 1) {
    // setNodeWeights: the descent of every training descriptor (k_bow_words over the tree in level order,
    // where the children of a node are contiguous already), then Ni per word
    std::vector<int2> tn(N);
    std::vector<uint8_t> td((size_t)N * 32);
    int max_children = 0;
    for (int q = 0; q < N; q++) {
      tn[q] = nodes[q].n_child ? make_int2(nodes[q].first_child, nodes[q].n_child) : make_int2(word_of[q], 0);
      memcpy(&td[(size_t)q * 32], nodes[q].desc, 32);
      max_children = std::max(max_children, nodes[q].n_child);
    }
    const size_t tree_bytes = (size_t)N * 40 + (size_t)n_words * 8 + 16;
    LISLAM_HIPCHK(c, room(t->tree, tree_bytes));
    LISLAM_HIPCHK(c, room(t->words, ((size_t)n + n_words) * sizeof(int)));
    uint4* d_td = static_cast<uint4*>(t->tree.p);
    int2* d_tn = reinterpret_cast<int2*>(d_td + (size_t)N * 2);
    double* d_tw = reinterpret_cast<double*>(d_tn + N);
    int* d_n = reinterpret_cast<int*>(d_tw + n_words);
    int* d_words = static_cast<int*>(t->words.p);
    int* d_ni = d_words + n;
    LISLAM_HIPCHK(c, hipMemcpyAsync(d_td, td.data(), td.size(), hipMemcpyHostToDevice, c->stream));
    LISLAM_HIPCHK(c, hipMemcpyAsync(d_tn, tn.data(), (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    LISLAM_HIPCHK(c, hipMemsetAsync(d_tw, 0, (size_t)n_words * 8, c->stream));
    LISLAM_HIPCHK(c, hipMemcpyAsync(d_n, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    LISLAM_HIPCHK(c, hipMemsetAsync(d_ni, 0, (size_t)n_words * sizeof(int), c->stream));
    const Tree tree{d_tn, d_td, d_tw, depth};
    const Source src{static_cast<const uint4*>(t->desc), nullptr, d_n, 0, 1, n, n};
    if (max_children <= 16)
      hipLaunchKernelGGL(k_bow_words<16>, dim3((unsigned)(((long long)n * 16 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                         c->stream, tree, src, d_words, (double*)nullptr);
    else
      hipLaunchKernelGGL(k_bow_words<64>, dim3((unsigned)(((long long)n * 64 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                         c->stream, tree, src, d_words, (double*)nullptr);
    LISLAM_HIPCHK(c, hipGetLastError());
    // the bitmap holds (images of a pass) x (words) bits
    const int row_words = (n_words + 31) / 32;
    const int per_pass = (int)std::max<size_t>(1, std::min<size_t>((size_t)t->n_images, kBitmapBytes / 4 / (size_t)row_words));
    LISLAM_HIPCHK(c, room(t->bitmap, (size_t)per_pass * row_words * 4));
    for (int m0 = 0; m0 < t->n_images; m0 += per_pass) {
      const int m1 = std::min(t->n_images, m0 + per_pass);
      const int i0 = t->img_off[m0], i1 = t->img_off[m1];
      if (i1 == i0) continue;
      LISLAM_HIPCHK(c, hipMemsetAsync(t->bitmap.p, 0, (size_t)(m1 - m0) * row_words * 4, c->stream));
      hipLaunchKernelGGL(k_bowt_ni, dim3((i1 - i0 + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, d_words,
                         static_cast<const int*>(t->img_of), i0, i1, m0, row_words, static_cast<uint32_t*>(t->bitmap.p), d_ni);
    }
    LISLAM_HIPCHK(c, hipGetLastError());
    std::vector<int> ni(n_words);
    LISLAM_HIPCHK(c, hipMemcpyAsync(ni.data(), d_ni, (size_t)n_words * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LISLAM_HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int wd = 0; wd < n_words; wd++) {
      if (ni[wd] > 0) t->weight[word_node[wd]] = std::log((double)t->n_images / (double)ni[wd]);
      st.n_zero_words += t->weight[word_node[wd]] == 0.0;
    }
  }
  st.weights_ms = ms_since(t_weights);
  st.total_ms = ms_since(t_call);
  t->trained = true;
  if (n_nodes_out) *n_nodes_out = N;
  if (stats) *stats = st;
  return LISLAM_OK;
}

int lislam_bow_trainer_vocabulary(lislam_bow_trainer* t, int32_t cap_nodes, int32_t* parent, uint8_t* descriptor,
                                  double* weight) {
  if (!t) return LISLAM_ERR_ARG;
  if (!t->trained) return fail(t->ctx, LISLAM_ERR_STATE, "lislam_bow_trainer_vocabulary: run lislam_bow_train first");
  const size_t N = t->parent.size();
  if (cap_nodes < 0 || (size_t)cap_nodes < N)
    return fail(t->ctx, LISLAM_ERR_CAPACITY, "lislam_bow_trainer_vocabulary: %zu nodes, capacity %d", N, cap_nodes);
  if (parent) memcpy(parent, t->parent.data(), N * sizeof(int32_t));
  if (descriptor) memcpy(descriptor, t->descriptor.data(), N * 32);
  if (weight) memcpy(weight, t->weight.data(), N * sizeof(double));
  return LISLAM_OK;
}

}  // extern "C"
