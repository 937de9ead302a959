// Host-side plumbing shared by the ABI translation units: the error formatter, the HIP-check and
// return-if-not-OK macros, the grow-only device buffer, and the argument checks of the batch feeds.
// Inline code only; no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "lislam_batch.hpp"
#include "lislam_ctx.hpp"

namespace lislam {

// Formats the context's error text (at most 511 characters) and returns code; a null context only
// returns the code.
__attribute__((format(printf, 3, 4))) inline int fail(lislam_ctx* c, int code, const char* fmt, ...) {
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

#define LISLAM_HIPCHK(ctx, x)                                                                                 \
  do {                                                                                                        \
    hipError_t e_ = (x);                                                                                      \
    if (e_ != hipSuccess) return lislam::fail(ctx, LISLAM_ERR_DEVICE, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

#define LISLAM_RC(x)                  \
  do {                                \
    int rc_ = (x);                    \
    if (rc_ != LISLAM_OK) return rc_; \
  } while (0)

// Growable device buffer.  Growing frees the old allocation: pass the stream whose queued work may
// still read it as `sync` and it is synchronised first (its error is returned and nothing is freed).
struct DBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t b, hipStream_t sync = nullptr) {
    if (b <= bytes) return hipSuccess;
    if (p) {
      if (sync) {
        const hipError_t e = hipStreamSynchronize(sync);
        if (e != hipSuccess) return e;
      }
      (void)hipFree(p);
    }
    p = nullptr;
    bytes = 0;
    const size_t nb = std::max<size_t>(b, 256) + b / 4;
    hipError_t e = hipMalloc(&p, nb);
    if (e == hipSuccess) bytes = nb;
    return e;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// ---------------------------------------------------------------- the batch feeds' argument checks
// `who` is the entry point's name, the prefix of its messages.  Each returns LISLAM_OK or the status
// it left in the context's error text; the callers keep their own order of checks.

inline int check_same_context(lislam_ctx* c, const char* who, const lislam_batch* b) {
  if (b->ctx != c) return fail(c, LISLAM_ERR_ARG, "%s: the batch belongs to another context", who);
  return LISLAM_OK;
}

// scans [first, first + n) within the batch's max_scans
inline int check_scan_range(lislam_ctx* c, const char* who, const lislam_batch* b, int first, int n) {
  if (first < 0 || n < 0 || (int64_t)first + n > b->max_scans)
    return fail(c, LISLAM_ERR_ARG, "%s: scans [%d, %d + %d) out of range", who, first, first, n);
  return LISLAM_OK;
}

inline int check_cloud_track(lislam_ctx* c, const char* who, const lislam_batch* b) {
  if (!b->fa.track) return fail(c, LISLAM_ERR_STATE, "%s: cloud_track not materialized (want_images=0)", who);
  return LISLAM_OK;
}

// the range feeds: scans [first, first + n) have been extracted (after check_scan_range)
inline int check_extracted(lislam_ctx* c, const char* who, const lislam_batch* b, int first, int n) {
  if (first + n > b->extracted) return fail(c, LISLAM_ERR_STATE, "%s: extract %d scans first", who, first + n);
  return LISLAM_OK;
}

// the list feeds: a non-empty list needs an extracted batch
inline int check_extracted_any(lislam_ctx* c, const char* who, const lislam_batch* b, int n) {
  if (n > 0 && b->extracted < 1) return fail(c, LISLAM_ERR_STATE, "%s: extract the batch first", who);
  return LISLAM_OK;
}

// every name[k] in [0, bound); with `increasing`, also name[k] > name[k - 1]
inline int check_index(lislam_ctx* c, const char* who, const char* name, const int32_t* index, int n, int bound,
                       bool increasing) {
  for (int k = 0; k < n; k++) {
    if (index[k] < 0 || index[k] >= bound)
      return fail(c, LISLAM_ERR_ARG, "%s: %s[%d] = %d outside [0, %d)", who, name, k, index[k], bound);
    if (increasing && k > 0 && index[k] <= index[k - 1])
      return fail(c, LISLAM_ERR_ARG, "%s: %s[%d] = %d after %d: the list must be strictly increasing", who, name, k, index[k],
                  index[k - 1]);
  }
  return LISLAM_OK;
}

// room for `add` more of `noun` ("entries", "keyframes") beside the `have` held
inline int check_capacity(lislam_ctx* c, const char* who, int have, int add, const char* noun, int capacity) {
  if ((int64_t)have + add > capacity)
    return fail(c, LISLAM_ERR_CAPACITY, "%s: %d + %d %s exceed the capacity %d", who, have, add, noun, capacity);
  return LISLAM_OK;
}

// The ORB descriptors of a batch for a feed (lislam_orb_batch_descriptors; a device-decided cascade's
// verdict is final after it).  LISLAM_ERR_STATE before lislam_batch_intensity_odometry, or when it ran
// fewer than `need` scans (need < 0, the list feeds: any number will do, *ran bounds the list); any
// other error is passed through.
struct OrbDescriptors {
  const uint8_t* desc = nullptr;
  const int* counts = nullptr;
  int cap = 0, nfeatures = 0, ran = 0;
};
inline int orb_descriptors(lislam_ctx* c, const char* who, lislam_batch* b, int need, OrbDescriptors* o) {
  const int rc = lislam_orb_batch_descriptors(b, &o->desc, &o->counts, &o->cap, &o->nfeatures, &o->ran);
  if (need < 0) {
    if (rc == LISLAM_ERR_STATE) return fail(c, LISLAM_ERR_STATE, "%s: run lislam_batch_intensity_odometry first", who);
  } else if (rc == LISLAM_ERR_STATE || (rc == LISLAM_OK && need > o->ran)) {
    return fail(c, LISLAM_ERR_STATE, "%s: run lislam_batch_intensity_odometry over %d scans first", who, need);
  }
  return rc;
}

}  // namespace lislam
