// Phase stamps of the attention kernels: the one place that knows about them.
//   make PROF=1 OUTDIR=../lib_prof   defines BEVR_PROF;  tools/prof_phases.py <tag> reads the counters.
// A wave sums s_memtime differences (and event counts) of its phases in registers and adds them once, at its end, to a
// per-kernel __device__ array that bevr_debug_prof_<tag>(out, reset) copies out or clears.  Without BEVR_PROF every
// macro below expands to nothing, and so it does in the VARIANT translation units (BEVR_DROP, BEVR_TAP_X3,
// BEVR_GATHER_ROWS, BEVR_SLAB_ROWS: a kernel's source compiled a second time), which would define the array and its reader
// again (BEVR_SLAB_X3 is not one of them: attn_slab_bwd_q_x3.hip has a kernel body of its own and its own tag, slab_x3).
// Include it after those four have their defaults (bevr_common.h, attn_tap.h, attn_gather_fwd.hip,
// attn_slab.h).
//
//   BEVR_PROF_DEFINE(tag, n)      file scope: the n counters and their reader
//   PROF_ACC(n)                   kernel body: the wave's accumulator
//   PROF_T*(var ...)              a stamp (below: they differ in what they wait for)
//   PROF_SET(var, v)              carry a stamp into the next iteration
//   PROF_ADD(i, v)                accumulator slot i += a difference of stamps or a count
//   PROF_FLUSH(tag, base, cond)   where `cond` holds (say lane 0 of wave 0): counters[base + i] += slot i
#pragma once
#include "bevr_common.h"

#if defined(BEVR_PROF) && !(BEVR_DROP || BEVR_TAP_X3 || BEVR_GATHER_ROWS || BEVR_SLAB_ROWS)

// PROF_T: memory counters drained, and `dep` (a value of the work just done) as an operand: the stamp cannot be hoisted
// above that work.  The query-stationary region kernels.
__device__ __forceinline__ unsigned long long prof_now(float dep) {
  unsigned long long t;
  asm volatile("s_nop 0\n s_waitcnt vmcnt(0) lgkmcnt(0)\n s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
  return t;
}
// PROF_T_LGKM: as PROF_T, but global loads stay in flight (the key-side backward prefetches table columns across phases).
__device__ __forceinline__ unsigned long long prof_now_lgkm(float dep) {
  unsigned long long t;
  asm volatile("s_nop 0\n s_waitcnt lgkmcnt(0)\n s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
  return t;
}
// PROF_T_DRAIN: memory counters drained, no operand (the slab kernel: its phases end in barriers).
__device__ __forceinline__ unsigned long long prof_now_drain() {
  unsigned long long t;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
// PROF_T_FREE: waits for nothing but its own result (the gather forward: the prefetches are meant to stay in flight).
__device__ __forceinline__ unsigned long long prof_now_free() {
  unsigned long long t;
  asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}

#define BEVR_PROF_DEFINE(tag, n)                                                                              \
  __device__ unsigned long long bevr_prof_##tag[n];                                                           \
  extern "C" int bevr_debug_prof_##tag(unsigned long long* out, int reset) {                                  \
    unsigned long long z[n] = {0};                                                                            \
    if (reset) return (int)hipMemcpyToSymbol(HIP_SYMBOL(bevr_prof_##tag), z, sizeof(z));                      \
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(bevr_prof_##tag), sizeof(z));                             \
  }
#define PROF_ACC(n) unsigned long long prof_acc[n] = {0}
#define PROF_T(var, dep) unsigned long long var = prof_now(dep)
#define PROF_T_LGKM(var, dep) unsigned long long var = prof_now_lgkm(dep)
#define PROF_T_DRAIN(var) unsigned long long var = prof_now_drain()
#define PROF_T_FREE(var) unsigned long long var = prof_now_free()
#define PROF_SET(var, v) var = (v)
#define PROF_ADD(i, v) prof_acc[i] += (v)
#define PROF_FLUSH(tag, base, cond)                                                                           \
  do {                                                                                                        \
    if (cond)                                                                                                 \
      for (int i_ = 0; i_ < (int)(sizeof(prof_acc) / sizeof(prof_acc[0])); ++i_)                              \
        atomicAdd(&bevr_prof_##tag[(base) + i_], prof_acc[i_]);                                               \
  } while (0)

#else

#define BEVR_PROF_DEFINE(tag, n)
#define PROF_ACC(n)
#define PROF_T(var, dep)
#define PROF_T_LGKM(var, dep)
#define PROF_T_DRAIN(var)
#define PROF_T_FREE(var)
#define PROF_SET(var, v)
#define PROF_ADD(i, v)
#define PROF_FLUSH(tag, base, cond) do { } while (0)

#endif
