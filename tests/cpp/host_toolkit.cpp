// The host toolkit of the ABI translation units (csrc/lislam_host.hpp) on its own: the formatter and the
// batch feeds' argument checks against the statuses and the exact texts they must leave, over a context
// and a batch built on the stack.  No HIP call is made, so it runs without a GPU;
// tests/test_host_toolkit_cpu.py builds it with the address and undefined-behaviour sanitizers.
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>

#include "lislam_host.hpp"

// the one symbol of the library the header's helpers call: the batch "ran" g_ran scans
static int g_rc = LISLAM_OK, g_ran = 0;
int lislam_orb_batch_descriptors(lislam_batch*, const uint8_t** desc, const int** counts, int* cap, int* nfeatures, int* n_scans) {
  *desc = nullptr;
  *counts = nullptr;
  *cap = 1000;
  *nfeatures = 1000;
  *n_scans = g_ran;
  return g_rc;
}

static int failures = 0;

static void expect(const char* what, const lislam_ctx& c, int rc, int want_rc, const std::string& want_err) {
  if (rc == want_rc && c.err == want_err) return;
  failures++;
  std::printf("%s: status %d, text \"%s\"; want %d, \"%s\"\n", what, rc, c.err.c_str(), want_rc, want_err.c_str());
}

int main() {
  using namespace lislam;
  lislam_ctx c, other;
  lislam_batch b;
  b.ctx = &c;
  b.max_scans = 4;
  b.extracted = 2;
  P4 track{};
  b.fa.track = &track;
  const std::string untouched = "untouched";
  const auto reset = [&] { c.err = untouched; };

  // fail: a null context only returns the code; 600 characters are cut to 511
  reset();
  expect("fail(null)", c, fail(nullptr, LISLAM_ERR_STATE, "lost %d", 1), LISLAM_ERR_STATE, untouched);
  const std::string longs(600, 'x');
  expect("fail(600)", c, fail(&c, LISLAM_ERR_DEVICE, "%s", longs.c_str()), LISLAM_ERR_DEVICE, std::string(511, 'x'));
  expect("fail(fmt)", c, fail(&c, LISLAM_ERR_ARG, "%s: %d of %lld", "who", 3, 1ll << 40), LISLAM_ERR_ARG, "who: 3 of 1099511627776");

  // same context
  reset();
  expect("context ok", c, check_same_context(&c, "f", &b), LISLAM_OK, untouched);
  expect("context", other, check_same_context(&other, "lislam_place_add_batch", &b), LISLAM_ERR_ARG,
         "lislam_place_add_batch: the batch belongs to another context");

  // scan ranges against max_scans = 4
  expect("range ok", c, check_scan_range(&c, "f", &b, 0, 4), LISLAM_OK, untouched);
  expect("range empty ok", c, check_scan_range(&c, "f", &b, 4, 0), LISLAM_OK, untouched);
  expect("range (-1, 1)", c, check_scan_range(&c, "lislam_bow_add_batch", &b, -1, 1), LISLAM_ERR_ARG,
         "lislam_bow_add_batch: scans [-1, -1 + 1) out of range");
  expect("range (0, -1)", c, check_scan_range(&c, "lislam_bow_add_batch", &b, 0, -1), LISLAM_ERR_ARG,
         "lislam_bow_add_batch: scans [0, 0 + -1) out of range");
  expect("range (max, 1)", c, check_scan_range(&c, "lislam_bow_add_batch", &b, 4, 1), LISLAM_ERR_ARG,
         "lislam_bow_add_batch: scans [4, 4 + 1) out of range");
  expect("range (INT32_MAX, 1)", c, check_scan_range(&c, "lislam_bow_add_batch", &b, INT32_MAX, 1), LISLAM_ERR_ARG,
         "lislam_bow_add_batch: scans [2147483647, 2147483647 + 1) out of range");

  // cloud_track
  reset();
  expect("track ok", c, check_cloud_track(&c, "f", &b), LISLAM_OK, untouched);
  b.fa.track = nullptr;
  expect("track null", c, check_cloud_track(&c, "lislam_keyframes_add_batch", &b), LISLAM_ERR_STATE,
         "lislam_keyframes_add_batch: cloud_track not materialized (want_images=0)");
  b.fa.track = &track;

  // extracted = 2
  reset();
  expect("extracted ok", c, check_extracted(&c, "f", &b, 1, 1), LISLAM_OK, untouched);
  expect("extracted + 1", c, check_extracted(&c, "lislam_place_add_batch", &b, 1, 2), LISLAM_ERR_STATE,
         "lislam_place_add_batch: extract 3 scans first");
  reset();
  expect("extracted any ok", c, check_extracted_any(&c, "f", &b, 1), LISLAM_OK, untouched);
  b.extracted = 0;
  expect("extracted any empty ok", c, check_extracted_any(&c, "f", &b, 0), LISLAM_OK, untouched);
  expect("extracted any", c, check_extracted_any(&c, "lislam_place_add_batch_scans", &b, 1), LISLAM_ERR_STATE,
         "lislam_place_add_batch_scans: extract the batch first");
  b.extracted = 2;

  // lists against [0, extracted)
  const int32_t at_bound[] = {0, 2}, negative[] = {-1}, repeat[] = {1, 1}, falling[] = {1, 0}, fine[] = {0, 1};
  reset();
  expect("list ok", c, check_index(&c, "f", "scans", fine, 2, b.extracted, true), LISLAM_OK, untouched);
  expect("list null ok", c, check_index(&c, "f", "scans", nullptr, 0, b.extracted, true), LISLAM_OK, untouched);
  expect("list {1, 1} free ok", c, check_index(&c, "f", "scans", repeat, 2, b.extracted, false), LISLAM_OK, untouched);
  expect("list {1, 0} free ok", c, check_index(&c, "f", "scans", falling, 2, b.extracted, false), LISLAM_OK, untouched);
  expect("list {0, extracted}", c, check_index(&c, "lislam_place_add_batch_scans", "scans", at_bound, 2, b.extracted, false),
         LISLAM_ERR_ARG, "lislam_place_add_batch_scans: scans[1] = 2 outside [0, 2)");
  expect("list {-1}", c, check_index(&c, "lislam_pgo_add_keyframes", "index", negative, 1, 8, true), LISLAM_ERR_ARG,
         "lislam_pgo_add_keyframes: index[0] = -1 outside [0, 8)");
  expect("list {1, 1} increasing", c, check_index(&c, "lislam_pgo_add_batch_scans", "scans", repeat, 2, b.extracted, true),
         LISLAM_ERR_ARG, "lislam_pgo_add_batch_scans: scans[1] = 1 after 1: the list must be strictly increasing");
  expect("list {1, 0} increasing", c, check_index(&c, "lislam_pgo_add_batch_scans", "scans", falling, 2, b.extracted, true),
         LISLAM_ERR_ARG, "lislam_pgo_add_batch_scans: scans[1] = 0 after 1: the list must be strictly increasing");

  // capacity
  reset();
  expect("capacity full ok", c, check_capacity(&c, "f", 1, 1, "entries", 2), LISLAM_OK, untouched);
  expect("capacity entries", c, check_capacity(&c, "lislam_bow_add_batch", 1, 2, "entries", 2), LISLAM_ERR_CAPACITY,
         "lislam_bow_add_batch: 1 + 2 entries exceed the capacity 2");
  expect("capacity keyframes", c, check_capacity(&c, "lislam_keyframes_add_batch_scans", 2, 1, "keyframes", 2),
         LISLAM_ERR_CAPACITY, "lislam_keyframes_add_batch_scans: 2 + 1 keyframes exceed the capacity 2");
  expect("capacity INT32_MAX", c, check_capacity(&c, "f", INT32_MAX, INT32_MAX, "entries", INT32_MAX), LISLAM_ERR_CAPACITY,
         "f: 2147483647 + 2147483647 entries exceed the capacity 2147483647");

  // the ORB descriptors of a batch
  OrbDescriptors o;
  reset();
  g_rc = LISLAM_OK;
  g_ran = 2;
  expect("orb ok", c, orb_descriptors(&c, "f", &b, 2, &o), LISLAM_OK, untouched);
  if (o.ran != 2 || o.cap != 1000 || o.nfeatures != 1000) expect("orb outputs", c, -100, LISLAM_OK, untouched);
  expect("orb list ok", c, orb_descriptors(&c, "f", &b, -1, &o), LISLAM_OK, untouched);
  expect("orb ran fewer", c, orb_descriptors(&c, "lislam_keysel_step_batch", &b, 3, &o), LISLAM_ERR_STATE,
         "lislam_keysel_step_batch: run lislam_batch_intensity_odometry over 3 scans first");
  g_ran = 0;
  expect("orb ran == 0", c, orb_descriptors(&c, "lislam_bow_trainer_add_batch", &b, 1, &o), LISLAM_ERR_STATE,
         "lislam_bow_trainer_add_batch: run lislam_batch_intensity_odometry over 1 scans first");
  g_rc = LISLAM_ERR_STATE;
  expect("orb state", c, orb_descriptors(&c, "lislam_bow_add_batch", &b, 0, &o), LISLAM_ERR_STATE,
         "lislam_bow_add_batch: run lislam_batch_intensity_odometry over 0 scans first");
  expect("orb state, list", c, orb_descriptors(&c, "lislam_bow_add_batch_scans", &b, -1, &o), LISLAM_ERR_STATE,
         "lislam_bow_add_batch_scans: run lislam_batch_intensity_odometry first");
  reset();
  g_rc = LISLAM_ERR_DEVICE;  // any other error is passed through, the text as the callee left it
  expect("orb other", c, orb_descriptors(&c, "f", &b, 1, &o), LISLAM_ERR_DEVICE, untouched);
  expect("orb other, list", c, orb_descriptors(&c, "f", &b, -1, &o), LISLAM_ERR_DEVICE, untouched);

  if (failures) {
    std::printf("%d failed\n", failures);
    return 1;
  }
  std::printf("host toolkit ok\n");
  return 0;
}
