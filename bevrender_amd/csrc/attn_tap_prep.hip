// Key preparation of the tap kernels (attn_tap.h): per key the clamped rpe-table coordinates and the sampling position
// in feature pixels (TapRec), per 32-key tile the box of its live keys (StepBox).  One wave per 64 keys, once per call.
#include "attn_tap.h"

namespace {

__global__ __launch_bounds__(256) void attn_tap_prep_kernel(bevr_attn_desc d, const float* __restrict__ key_a,
                                                            const float* __restrict__ key_b, const float* __restrict__ key_y,
                                                            const float* __restrict__ key_x, TapRec* __restrict__ rec_out,
                                                            StepBox* __restrict__ box_out,
#if BEVR_TAP_G2
                                                            TapPos1* __restrict__ pos1_out,
#endif
                                                            int n_wave_total) {
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);   // global wave = prob * n_step + step (two groups: prob = key row)
  if (gw >= n_wave_total) return;
  const int lane = threadIdx.x & 63;
  const int n_step = d.Np / KT;
  const int prob = gw / n_step, step = gw % n_step;
  const size_t idx = (size_t)prob * d.Np + (size_t)step * KT + lane;
  const bool live = step * KT + lane < d.N;
  const KeyClamp kc = key_clamp(key_a[idx], key_b[idx], d);
  const float a = kc.a, b = kc.b;
  const int A = (int)kc.af;
  const int amin = lanes_min<32>(live ? A : 0x7fffffff), amax = lanes_max<32>(live ? A : (int)0x80000000);
  const float bmin = lanes_min<32>(live ? b : 3.0e38f), bmax = lanes_max<32>(live ? b : -3.0e38f);
  TapRec r;
  r.a = live ? a : (amax >= amin ? (float)amin : 0.f);
  r.b = live ? b : (amax >= amin ? bmin : 0.f);
  // NaN positions sample nothing (every hat() of a NaN is 0 through fmaxf)
#if BEVR_TAP_G2
  // key_y, key_x [row][2][Np]: plane 0 the position of group 0 (the record's), plane 1 of group 1
  const size_t idx0 = idx + (size_t)prob * d.Np;
  r.ys = live ? key_y[idx0] : TAP_YS_DEAD;
  r.xs = live ? key_x[idx0] : 0.f;
  TapPos1 r1;
  r1.ys = live ? key_y[idx0 + d.Np] : TAP_YS_DEAD;
  r1.xs = live ? key_x[idx0 + d.Np] : 0.f;
  BEVR_ASSERT(!(live && (r1.ys >= (float)(TAP_R - 1) || r1.xs >= (float)(TAP_C - 1))));
  pos1_out[idx] = r1;
#else
  r.ys = live ? key_y[idx] : TAP_YS_DEAD;
  r.xs = live ? key_x[idx] : 0.f;
#endif
  // the tap contract (attn_tap.h): a live key samples inside feature rows 0..3 x columns 0..2.  A key beyond them would
  // silently lose the taps the 12-pixel grid does not hold; the bounds-checking build traps (NaN positions sample nothing
  // and compare false)
  BEVR_ASSERT(!(live && (r.ys >= (float)(TAP_R - 1) || r.xs >= (float)(TAP_C - 1))));
  rec_out[idx] = r;
  if ((lane & 31) == 0) {
    StepBox sb;
    sb.amin = amin; sb.amax = amax; sb.bmin = bmin; sb.bmax = bmax;
    box_out[2 * gw + (lane >> 5)] = sb;
  }
}

}  // namespace

#if BEVR_TAP_G2
// this translation unit is attn_tap_prep_g2.hip: the preparation for two channel groups
extern "C" size_t bevr_attn_tap_g2_ws_bytes(const bevr_attn_desc* d) {
  if (bevr_check_desc(d)) return 0;
  return tap_ws_pos1_offset(*d) + tap_ws_rows(*d) * d->Np * sizeof(TapPos1);
}

extern "C" int bevr_attn_tap_g2_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const float* key_y,
                                     const float* key_x, void* tap_ws, void* stream) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!key_a || !key_b || !key_y || !key_x || !tap_ws) return BEVR_E_NULL;
  if (d->groups != 2 || (d->heads & 1)) return BEVR_E_SHAPE;
  if (!bevr_aligned16(tap_ws)) return BEVR_E_ALIGN;
  const int n_wave = (int)tap_ws_rows(*d) * (d->Np / KT);
  TapRec* rec = reinterpret_cast<TapRec*>(tap_ws);
  StepBox* box = reinterpret_cast<StepBox*>(reinterpret_cast<char*>(tap_ws) + tap_ws_box_offset(*d));
  TapPos1* pos1 = reinterpret_cast<TapPos1*>(reinterpret_cast<char*>(tap_ws) + tap_ws_pos1_offset(*d));
  hipLaunchKernelGGL(attn_tap_prep_kernel, dim3((n_wave + 3) / 4), dim3(256), 0, (hipStream_t)stream, *d, key_a, key_b,
                     key_y, key_x, rec, box, pos1, n_wave);
  return (int)hipGetLastError();
}
#else
extern "C" size_t bevr_attn_tap_ws_bytes(const bevr_attn_desc* d) {
  if (bevr_check_desc(d)) return 0;
  return tap_ws_box_offset(*d) + (size_t)d->n_prob * (d->Np / 32) * sizeof(StepBox);
}

extern "C" int bevr_attn_tap_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const float* key_y,
                                  const float* key_x, void* tap_ws, void* stream) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!key_a || !key_b || !key_y || !key_x || !tap_ws) return BEVR_E_NULL;
  if (d->groups != 1) return BEVR_E_SHAPE;
  if (!bevr_aligned16(tap_ws)) return BEVR_E_ALIGN;
  const int n_wave = d->n_prob * (d->Np / KT);
  TapRec* rec = reinterpret_cast<TapRec*>(tap_ws);
  StepBox* box = reinterpret_cast<StepBox*>(reinterpret_cast<char*>(tap_ws) + tap_ws_box_offset(*d));
  hipLaunchKernelGGL(attn_tap_prep_kernel, dim3((n_wave + 3) / 4), dim3(256), 0, (hipStream_t)stream, *d, key_a, key_b,
                     key_y, key_x, rec, box, n_wave);
  return (int)hipGetLastError();
}
#endif
