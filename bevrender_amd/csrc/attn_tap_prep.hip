// Key preparation of the tap kernels (attn_tap.h): per key the clamped rpe-table coordinates and the sampling position
// in feature pixels (TapRec), per 32-key tile the box of its live keys (StepBox).  One wave per 64 keys, once per call.
#include "attn_tap.h"

namespace {

__global__ __launch_bounds__(256) void attn_tap_prep_kernel(bevr_attn_desc d, const float* __restrict__ key_a,
                                                            const float* __restrict__ key_b, const float* __restrict__ key_y,
                                                            const float* __restrict__ key_x, TapRec* __restrict__ rec_out,
                                                            StepBox* __restrict__ box_out, int n_wave_total) {
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);   // global wave = prob * n_step + step
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
  r.ys = live ? key_y[idx] : TAP_YS_DEAD;
  r.xs = live ? key_x[idx] : 0.f;
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
