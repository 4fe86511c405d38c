// The debug ABI of libmvn_hip (mvn_debug_*, include/mvn_hip.h): the device-assertion registry
// and its self-test, the test-only knobs of the unprojection dispatch, and the occupancy query.
#include <atomic>

#include "unproject_common.hpp"
#include "x4_order.hpp"

namespace mvn {

std::vector<DassertReader>& dassert_registry() {
  static std::vector<DassertReader> r;
  return r;
}

namespace {
// one deliberately failing check per lane >= n (the mechanism's self-test)
__global__ void dassert_selftest(int n) { MVN_DASSERT(int(threadIdx.x) < n); }

std::atomic<int> g_lds_slots{0}, g_force_simple{0};
}  // namespace

int unproject_lds_slot_budget() { return g_lds_slots.load(std::memory_order_relaxed); }
bool unproject_force_simple() { return g_force_simple.load(std::memory_order_relaxed) == 1; }
bool unproject_force_generic() { return g_force_simple.load(std::memory_order_relaxed) == 2; }
bool unproject_force_wide_slots() { return g_force_simple.load(std::memory_order_relaxed) == 3; }

}  // namespace mvn

extern "C" int mvn_debug_unproject_occupancy(int bf16_maps) {
  return mvn::unproj::x4_blocks_per_cu(bf16_maps ? 1 : 0);
}

extern "C" int mvn_debug_x4_shape_occupancy(int shape, int* private_bytes, int* registers) {
  if ((shape != 0 && shape != 5) || !private_bytes || !registers) return MVN_ERR_ARG;
  return mvn::unproj::x4_shape_occupancy(shape, private_bytes, registers);
}

extern "C" int mvn_debug_x4_image_slots(int shape) {
  return shape < 0 || shape > 2 ? MVN_ERR_ARG : mvn::unproj::x4_image_slots(shape);
}

extern "C" int mvn_debug_x4_block_tiles(int order, int frames, int nTx, int nTy, int nTz, int* tiles) {
  const long long nb = (long long)frames * nTx * nTy * nTz;
  if (!tiles || frames < 1 || nTx < 1 || nTy < 1 || nTz < 1 || nb > INT_MAX) return MVN_ERR_ARG;
  if (order < -1 || order > mvn::unproj::kX4OrderCentre3D) return MVN_ERR_ARG;
  const int use = order < 0 ? mvn::unproj::x4_launch_order() : order;
  for (int i = 0; i < int(nb); ++i) tiles[i] = mvn::unproj::x4_block_tile(i, nTx, nTy, nTz, use);
  return MVN_OK;
}

extern "C" int mvn_debug_dassert_selftest(int n, void* stream) {
  if (n < 0 || n > 64) return MVN_ERR_ARG;
  mvn::dassert_selftest<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(n);
  return mvn::launch_ok() ? MVN_OK : MVN_ERR_LAUNCH;
}

extern "C" int mvn_debug_device_asserts(int* enabled, unsigned* count, unsigned* first_line) {
  if (!enabled || !count || !first_line) return MVN_ERR_ARG;
#ifdef MVN_DEVICE_ASSERTS
  *enabled = 1;
#else
  *enabled = 0;
#endif
  *count = 0;
  *first_line = 0;
  for (auto rd : mvn::dassert_registry()) {
    unsigned c = 0, l = 0;
    if (rd(&c, &l) != 0) return MVN_ERR_LAUNCH;
    if (c && !*count) *first_line = l;
    *count += c;
  }
  return MVN_OK;
}

extern "C" int mvn_debug_set_unproject(int lds_slots, int kernel) {
  if (lds_slots < 0 || kernel < 0 || kernel > 3) return MVN_ERR_ARG;
  mvn::g_lds_slots.store(lds_slots, std::memory_order_relaxed);
  mvn::g_force_simple.store(kernel, std::memory_order_relaxed);
  return MVN_OK;
}
