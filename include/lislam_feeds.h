/* lislam_feeds.h - the back end's feeds for a list of scans.
 *
 * include/lislam.h feeds the keyframe pool, Scan Context, the bag of words and the pose graph from a
 * contiguous range of a batch's scans.  After keyframe selection (lislam_keysel_*) the scans to feed are
 * a list; these are the forms that take one.  They live in the library (liblislam.so) like everything
 * else and return the same status codes.
 */
#ifndef LISLAM_FEEDS_H_
#define LISLAM_FEEDS_H_

#include "lislam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The list form of lislam_keyframes_add_batch: scans[n] (host, any order, repeats allowed) names scans of
 * one batch, and the pool ends as the n calls lislam_keyframes_add_batch(kf, b, scans[k], 1) in that order would leave it, from one
 * gather launch.  Every precondition is checked before anything is added: scans[k] outside
 * [0, extracted scans) is LISLAM_ERR_ARG and lislam_last_error names k; capacity, context and state
 * errors as the range form.  n == 0 is a no-op.  lislam_place_add_batch_scans and
 * lislam_bow_add_batch_scans follow the same rules against their own range forms. */
int lislam_keyframes_add_batch_scans(lislam_keyframes* kf, lislam_batch* b, const int32_t* scans, int32_t n);

/* The list form of lislam_place_add_batch (rules as lislam_keyframes_add_batch_scans): entry size + k =
 * scan scans[k]. */
int lislam_place_add_batch_scans(lislam_place* p, lislam_batch* b, const int32_t* scans, int32_t n);

/* The list form of lislam_bow_add_batch (rules as lislam_keyframes_add_batch_scans): entry size + k = scan
 * scans[k]; the valid indices are [0, scans the last lislam_batch_intensity_odometry covered).  Asynchronous. */
int lislam_bow_add_batch_scans(lislam_bow* p, lislam_batch* b, const int32_t* scans, int32_t n);

/* mapOdomHandle (:395-514) for n keyframes picked out of one trajectory pose7[n_poses][7] (host or
 * device memory, every pose in one frame): node k gets pose7[index[k]] as its initial estimate (:456-462,
 * :500-509), byte for byte, and edge (k - 1, k) measures pose7[index[k-1]]^-1 pose7[index[k]] with var6
 * (NULL: odometryNoise_, :472-497).  When the graph is not empty, keyframe 0 gets an edge from the graph's
 * last node, measured from the pose that node was ADDED with (graph_prev_rotation_ / graph_prev_translation_,
 * :513-514), not from its current estimate: the graph keeps that pose, and lislam_pgo_add_nodes and
 * lislam_pgo_add_batch record it too.  index[n] (host) must be strictly increasing within [0, n_poses),
 * otherwise LISLAM_ERR_ARG; capacity errors as lislam_pgo_add_batch; nothing is added on an error.
 * n == 0 is a no-op.  This is the form for non-consecutive keyframes: lislam_pgo_add_batch(first = i,
 * n = 1) takes its edge from scan i - 1, the reference's BetweenFactor runs from the previous keyframe. */
int lislam_pgo_add_keyframes(lislam_pgo* p, const double* pose7, int32_t n_poses, const int32_t* index, int32_t n,
                             const double* var6);
/* The same with pose7 = the LISLAM_OUT_POSE rows of a batch whose odometry has run, read where they lie
 * on the device; scans[n] strictly increasing within [0, extracted scans).  A batch's LISLAM_OUT_POSE
 * starts again at the identity with every batch: a stream that spans several batches hands in one
 * continuous trajectory through lislam_pgo_add_keyframes instead (lislam_odom_fuse's output, say). */
int lislam_pgo_add_batch_scans(lislam_pgo* p, lislam_batch* batch, const int32_t* scans, int32_t n, const double* var6);

#ifdef __cplusplus
}
#endif
#endif /* LISLAM_FEEDS_H_ */
