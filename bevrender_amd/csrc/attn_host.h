// Host side of the attention entry points: what every source's run() / launch() shares because it hides a policy or
// states a contract (DESIGN.md "Host layer of the attention entry points").  Nothing here runs on the device; LIST_HEAD is
// the one constant the kernels read too.
#pragma once
#include <mutex>
#include <type_traits>
#include "bevr_common.h"

// ---- precision dispatch -----------------------------------------------------------------------------------
// f(std::integral_constant<int, P>) for the P of PRECS that equals `precision`, tried in the order written;
// BEVR_E_PRECISION for a precision outside the list.  The list at the call IS the set the entry point accepts:
//   bevr_for_precision<BEVR_PREC_BF16, BEVR_PREC_F16>(d->precision, [&](auto P) { return launch<P()>(*d, ..., st); })
template <int P0, int... PRECS, typename F>
int bevr_for_precision(int precision, F&& f) {
  if (precision == P0) return f(std::integral_constant<int, P0>());
  if constexpr (sizeof...(PRECS) > 0) return bevr_for_precision<PRECS...>(precision, f);
  return BEVR_E_PRECISION;
}

// ---- device facts -----------------------------------------------------------------------------------------
// The CU count, a kernel's residency and its raised dynamic-LDS limit belong to a DEVICE, not to the process: a process
// that moves between devices (hipSetDevice, torch.cuda.device) must find each device's own.  One slot per device ordinal,
// filled under the slot's mutex by the first launch on that device; a query that fails is not cached and is asked again.
constexpr int BEVR_MAX_DEVICES = 64;
class BevrPerDevice {
  std::mutex lock_[BEVR_MAX_DEVICES];
  int value_[BEVR_MAX_DEVICES] = {};     // 0: not known yet
 public:
  // the current device's value: query(device) on first use, which returns it (> 0) or 0 for "failed"; 0 also for a device
  // ordinal outside the table
  template <typename F> int get(F&& query) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= BEVR_MAX_DEVICES) return 0;
    std::lock_guard<std::mutex> hold(lock_[dev]);
    if (value_[dev] == 0) value_[dev] = query(dev);
    return value_[dev];
  }
};

// compute units of the current device; 0: the query failed (static, as bevr_check_desc: nothing here is exported)
static inline int bevr_cu_count() {
  static BevrPerDevice cus;
  return cus.get([](int dev) {
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 0;
  });
}

// workgroups of KERN the current device holds at once: compute units x the kernel's residency; 0: a query failed.
// Cached per kernel: threads and lds are the ONE shape the kernel is launched with.
template <auto KERN>
int bevr_resident_workgroups(int threads, size_t lds) {
  static BevrPerDevice resident;
  return resident.get([&](int) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERN, threads, lds) != hipSuccess) return 0;
    return bevr_cu_count() * per_cu;
  });
}

// Raise KERN's dynamic-LDS limit to `bytes` (above the 64 KB a kernel gets unasked), once per device: the attribute is
// the kernel's ON that device.  0 or the runtime's error code.  Cached per kernel: `bytes` is the kernel's one limit.
template <auto KERN>
int bevr_raise_dynamic_lds(int bytes) {
  static BevrPerDevice raised;
  hipError_t e = hipErrorInvalidDevice;
  const int done = raised.get([&](int) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e == hipSuccess ? 1 : 0;
  });
  return done ? 0 : (int)e;
}

// ---- work list, host half ---------------------------------------------------------------------------------
// A list launch's workspace is int [LIST_HEAD + n units]: [0] the count of listed units, [1] the claim counter of a list
// kernel that hands items out, [LIST_HEAD + i] the units.  The main launch fills it and the list launch, next on the
// stream, runs what it holds (attn_bwd_k.hip, attn_tap_bwd_k.hip: the device half).
constexpr int LIST_HEAD = 4;
static inline size_t bevr_list_bytes(size_t n_units) { return (LIST_HEAD + n_units) * sizeof(int); }
// before the main launch: an empty list
static inline int bevr_list_clear(int* list, hipStream_t st) { return (int)hipMemsetAsync(list, 0, LIST_HEAD * sizeof(int), st); }
// grid of the list launch: what the device holds of KERN, or the caller's max_workgroups if that is set and smaller;
// 0: the device could not be asked
template <auto KERN>
int bevr_list_workgroups(int max_workgroups, int threads, size_t lds) {
  const int resident = bevr_resident_workgroups<KERN>(threads, lds);
  return max_workgroups > 0 && max_workgroups < resident ? max_workgroups : resident;
}
