// mapOptimization's ORB keyframe sliding window (lislam_mapwin.hip): the device entry points the
// mapOptimization step (lislam_map.hip) composes.  Everything here is enqueued on the context's
// stream; nothing synchronizes.
#pragma once
#include "lislam_ctx.hpp"

struct lislam_mapwin;

namespace lislam {
namespace mapwin {

constexpr int kMaxWindow = 16;      // window_size
constexpr int kMaxFeatures = 4096;  // feature_capacity: a query / train index fits 12 bits
constexpr int kMaxKeep = 820;       // G <= ceil(4096 * 0.2)

lislam_ctx* context(lislam_mapwin* w);
int window_size(lislam_mapwin* w);
int feature_capacity(lislam_mapwin* w);

// The current keyframe's descriptors and sensor-frame points (host or device) into the ring's free
// slot, where the matching reads them and a push leaves them.
int stage(lislam_mapwin* w, const uint8_t* desc, const float* p3d, int n);
// The free slot itself (device, feature_capacity rows), for a producer that writes features in
// place; stage() of these pointers then only records the count.
uint8_t* stage_desc(lislam_mapwin* w);
float* stage_p3d(lislam_mapwin* w);
// mapOptimization.cpp:295-361 for the staged keyframe at the device pose `pose` (q, t): kind-3
// records [0, *count) of rec() / kind(), info() rows and pairs().  Room for `plane_cap` more
// records is reserved behind them.
int records(lislam_mapwin* w, const double* pose, int plane_cap);
// The plane records (n at most, *ncount of them) behind the feature records; *total() = both.
int append(lislam_mapwin* w, const double* rec, const int* kind, const int* ncount, int n);
double* rec(lislam_mapwin* w);
int* kind(lislam_mapwin* w);
int* total(lislam_mapwin* w);
int* info(lislam_mapwin* w);  // [window][6], then the feature-record count and the keyframes used
int* pairs(lislam_mapwin* w);
int capacity_records(lislam_mapwin* w);  // feature-record rows of rec()
// :481-493: emplace_back of the staged keyframe with the device pose `pose`, pop_front beyond the size.
int push_staged(lislam_mapwin* w, const double* pose);

}  // namespace mapwin
}  // namespace lislam
