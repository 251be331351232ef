// Forward of the tap kernels (attn_tap.h): R[slot][q] = sum_n w_slot(n) exp2(S[n][q] - mref[q]) over a key segment whose
// keys sample inside the top-left TAP_R x TAP_C feature pixels,
//     S[n][q] = sum_t w_t(n) G[t][q] + Gb[q] + bias[n][q]          (model/SCA_deform_attn.py:331-402 of the reference),
// row TAP_ONE of R = the softmax denominator.  No K / V operand exists: the caller forms G = scale Kpix Q^T before and
// O = R Vpix after the launch (two thin GEMMs) and merges the result with the other key segment of the same softmax.
//
// Work split: workgroup = ONE BEV column j of one (problem, head); wave w owns the 16-row blocks [w NB, (w + 1) NB) of the
// column, the LAST wave is the PRODUCER.  Per emission (two 32-key tiles) the producer turns the keys' records into the A
// operand ([12 tap weights, 0, 0, dead, 1 | 16 bias-cell weights] per key, 64 B) in LDS, and, when a tile's chunk origin
// differs from the previous one, the table side Tsh[cell][row] of that chunk for every BEV row of the column into a ring of
// four LDS images: the row-block waves never touch global memory inside the loop.  One barrier per emission.
//
// ANY key set is handled: a tile whose taps do not fit one 4 x 4 chunk for this column is emitted several times, each
// time with the keys of one chunk live and the others masked (at least one key per pass); a cell-sorted segment
// (ops.cell_order) needs that for ~0.1 % of its tiles.
//
// Softmax reference: STATIC.  mref[q] is given by the caller (an upper bound of the row's logits minus a headroom, so
// that no weight can overflow); the loop carries no running maximum, no rescale and no row sum.  A row whose weights
// all underflowed against that reference (bound looser than ~190 binades: exploding activations) is flagged per column
// and recomputed by the EXACT instantiation (online maximum), which overwrites R and mref of the flagged columns.
// fp16 flags a column sooner, as soon as a row's sum is under Np 2^-14 (the epilogue): under it the weights are fp16
// subnormals whose rounding no longer averages out of the sum.
#include "attn_tap.h"
#include "attn_host.h"

#if BEVR_DROP
#define BEVR_TAP_FWD_DROP_PARAMS , float* lsum TAP_DROP_PARAMS
#define BEVR_TAP_FWD_DROP_ARGS , lsum TAP_DROP_ARGS
#else
#define BEVR_TAP_FWD_DROP_PARAMS
#define BEVR_TAP_FWD_DROP_ARGS
#endif

namespace {

// NB: 16-row blocks per row-block wave (at most 7 row-block waves + the producer: fewer, fatter waves beat one wave per
// block by 1.5x -- the barrier is cheaper and the A operand is read once per wave).  EXACT: online maximum (the recompute
// pass of flagged columns).
#if BEVR_DROP
// (the eight keep hashes of a tile are in flight together: NB = 2 needs more than the 80 registers of 6 waves per SIMD)
#define TAP_FWD_WAVES(NB_) ((NB_) == 1 ? 6 : 4)
#else
#define TAP_FWD_WAVES(NB_) ((NB_) == 4 ? 4 : 6)
#endif
// (split mode: every operand twice -- 4 waves per SIMD, the fat NB = 4 instantiation 2; with the keep mask NB = 2 spills
// ~100 bytes a lane at the 128 registers of 4 waves: 3)
constexpr int tap_fwd_waves(int prec, int nb) {
  // (two groups: one more B operand, A operand and accumulator per row block -- as the split mode)
  return tap_split(prec) || BEVR_TAP_G2 ? (nb == 4 ? 2 : BEVR_DROP && nb == 2 ? 3 : 4) : TAP_FWD_WAVES(nb);
}
template <int PREC, int NB, bool EXACT>
__global__ __launch_bounds__(512, tap_fwd_waves(PREC, NB)) void attn_tap_fwd_kernel(
    bevr_attn_desc d, const char* __restrict__ G, const char* __restrict__ tap_ws,
    const char* __restrict__ table_pair, float* __restrict__ mref, float* __restrict__ R, int* __restrict__ flags
#if BEVR_DROP
    , float* __restrict__ lsum TAP_DROP_PARAMS
#endif
    ) {
  typedef LdsTp<PREC> L;
  constexpr int NP = tap_np<PREC>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int n_ph = d.n_prob * d.heads;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int ph = (slot / d.S) * 8 + xcd;
  if (ph >= n_ph) return;
  const int j = slot % d.S;
  if constexpr (EXACT) {
    if (flags[ph * d.S + j] == 0) return;
  }
  const int prob = ph / d.heads, hd = ph % d.heads;
  const int tid = threadIdx.x, n_wave = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int li = lane & 15, kg = lane >> 4;
  const int Mp = d.S * d.Sp;
  const int nblk = (d.S + QB - 1) / QB;
  const int rows_img = nblk * QB;
  const int img_bytes = rows_img * 32 * NP;
  char* ring = smem + 2 * L::BUF;
  const char* tbl = table_pair + (size_t)hd * d.Wp * d.Hp * 8;
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const float jrx = (float)j * rx;

  if (wave == n_wave - 1) {
    const int krow = tap_key_row(d, prob, hd);
    const TapRec* recs = reinterpret_cast<const TapRec*>(tap_ws) + (size_t)krow * d.Np;
    const StepBox* box = reinterpret_cast<const StepBox*>(tap_ws + tap_ws_box_offset(d)) + (size_t)krow * (d.Np / 32);
#if BEVR_TAP_G2
    const TapPos1* pos1 = reinterpret_cast<const TapPos1*>(tap_ws + tap_ws_pos1_offset(d)) + (size_t)krow * d.Np;
    tap_producer<PREC>(d, smem, ring, img_bytes, rows_img, recs, box, pos1, tbl, jrx, lane);
#else
    tap_producer<PREC>(d, smem, ring, img_bytes, rows_img, recs, box, tbl, jrx, lane);
#endif
    return;
  }

  // ---- row-block waves ------------------------------------------------------------------------------------
  const int blk0 = wave * NB;
  // B operand: lanes 0..31 G[q][8 kg ..] (constant), lanes 32..63 the chunk's table side (per origin)
  TapOp<NP> bop[NB];
  f32x4 r[NB];        // R[slot 4 kg + e][q]
  float sh[NB];       // EXACT: the running maximum relative to mref
  size_t mqv[NB];
#if BEVR_TAP_G2
  TapOp<NP> bop2[NB];  // group 1: lanes 0..31 G[q][16 + 8 kg ..], lanes 32..63 zero (the A operand there is finite)
  f32x4 r1[NB];        // R[slot 16 + 4 kg + e][q]
#endif
  const size_t g_lo = (size_t)n_ph * Mp * TAP_SLOTS * 2;     // G's lo plane
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int blk = min(blk0 + nb, nblk - 1);
    const size_t mq = (size_t)ph * Mp + (size_t)j * d.Sp + blk * QB + li;
    mqv[nb] = mq;
    bop[nb] = TapOp<NP>{};
    if (kg < 2) bop[nb] = tap_ld<NP>(G + (mq * TAP_ROW + 8 * kg) * 2, g_lo);
#if BEVR_TAP_G2
    bop2[nb] = TapOp<NP>{};
    if (kg < 2) bop2[nb] = tap_ld<NP>(G + (mq * TAP_ROW + TAP_SLOTS + 8 * kg) * 2, g_lo);
    r1[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#endif
    r[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    sh[nb] = -3.0e38f;
  }
#if BEVR_DROP
  uint32_t hrow[NB];  // the row part of the keep hash, out of the key loop
  float ls[NB];       // this lane's share of the row sum of ALL weights (R's slot TAP_ONE holds the kept mass)
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    hrow[nb] = bevr_drop_row(drop_seed, (uint32_t)ph, (uint32_t)(j * d.Sp + min(blk0 + nb, nblk - 1) * QB + li));
    ls[nb] = 0.f;
  }
#endif
  // this lane's LDS addresses inside a buffer
  const int a_off = (kg < 2 ? L::OFF_TAPS : L::OFF_CELLS) + li * 32 + (kg & 1) * 16;     // + tile * 1024 + sub * 512
  const int t_off = L::OFF_TAPS + (4 * kg + (li >> 2)) * 32 + (lane & 3) * 8;             // + tile * 1024, second block + 512
  const int i_off = li * 32 + (kg & 1) * 16;                                             // in a table image, + block * 512
#if BEVR_TAP_G2
  const int a1_off = L::OFF_TAPS1 + li * 32 + (kg & 1) * 16;                             // group 1's image, as a_off / t_off
  const int t1_off = L::OFF_TAPS1 + (4 * kg + (li >> 2)) * 32 + (lane & 3) * 8;
#endif
  // the B operand exists once per tile slot of an emission (their chunk origins may differ); lanes 0..31 of both hold G
  TapOp<NP> bop1[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bop1[nb] = bop[nb];
  int have0 = 0, have1 = 0;      // allocation numbers of the table images in bop / bop1 (0: the zeroed image)

  // one 32-key tile against one row block: S^T (two 16-key sub-tiles) -> weights -> R += w^T P
  // (kh: the tile's key hash, dropout builds)
#if BEVR_TAP_G2
  // (c0, c1, wt1: group 1's A operands of the two sub-tiles and its w^T)
  auto tile = [&](const TapOp<NP>& a0, const TapOp<NP>& a1, const TapOp<NP>& wt, const TapOp<NP>& b, int nb,
                  [[maybe_unused]] uint32_t kh, const TapOp<NP>& c0, const TapOp<NP>& c1, const TapOp<NP>& wt1) {
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 s0 = tap_mm<PREC, true>(a0, b, tap_mm<PREC, true>(c0, bop2[nb], z4));
    f32x4 s1 = tap_mm<PREC, true>(a1, b, tap_mm<PREC, true>(c1, bop2[nb], z4));
#else
  auto tile = [&](const TapOp<NP>& a0, const TapOp<NP>& a1, const TapOp<NP>& wt, const TapOp<NP>& b, int nb,
                  [[maybe_unused]] uint32_t kh) {
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 s0 = tap_mm<PREC, true>(a0, b, z4);
    f32x4 s1 = tap_mm<PREC, true>(a1, b, z4);
#endif
    if constexpr (EXACT) {
      float tm = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
      tm = fmaxf(tm, __shfl_xor(tm, 16));
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float mn = fmaxf(sh[nb], tm);
      const float al2 = fast_exp2(sh[nb] - mn);
      r[nb] *= al2;
#if BEVR_TAP_G2
      r1[nb] *= al2;
#endif
#if BEVR_DROP
      ls[nb] *= al2;
#endif
      sh[nb] = mn;
      s0 -= mn;
      s1 -= mn;
    }
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = fast_exp2(k < 4 ? s0[k & 3] : s1[k & 3]);
#if BEVR_DROP
    ls[nb] += ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      p[k] = tap_drop_keep8(hrow[nb], kh, k, drop_thr) ? p[k] : 0.f;
      // (the select stays on the float: moved behind the conversion it splits every v_cvt_pk into two conversions and a
      // v_perm, one more instruction per pair)
      asm("" : "+v"(p[k]));
    }
#endif
#if BEVR_TAP_G2
    const TapOp<NP> p8 = tap_pack8<PREC>(p);
    r[nb] = tap_mm<PREC>(wt, p8, r[nb]);
    r1[nb] = tap_mm<PREC>(wt1, p8, r1[nb]);
#else
    r[nb] = tap_mm<PREC>(wt, tap_pack8<PREC>(p), r[nb]);
#endif
  };
  // a chunk's table side out of ring image `al` (lanes 32..63)
  auto ring_load = [&](TapOp<NP> (&b)[NB], int al) {
    if (kg < 2) return;
    const char* img = ring + (al & (L::RING - 1)) * img_bytes + i_off;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) b[nb] = tap_ld<NP>(img + min(blk0 + nb, nblk - 1) * 512, rows_img * 32);
  };

  for (int e = 0;; ++e) {
    __syncthreads();
    const char* base = smem + (e & 1) * L::BUF;
    const u32x4 ct = *reinterpret_cast<const u32x4*>(base + L::OFF_CT);
    const int fl = __builtin_amdgcn_readfirstlane((int)ct[0]);
    if (fl & 4) break;
    const int al0 = __builtin_amdgcn_readfirstlane((int)ct[1]), al1 = __builtin_amdgcn_readfirstlane((int)ct[2]);
    if (al0 != have0) {   // uniform, rare: another chunk origin
      have0 = al0;
      ring_load(bop, al0);
    }
    if (al1 != have1) {
      have1 = al1;
      ring_load(bop1, al1);
    }
    // both tile slots, unconditionally: a slot without live keys holds masked keys only (weight 0)
    TapOp<NP> a[4], wt[2];     // A of sub-tile k = 2 tile + sub, w^T of tile 0 / 1
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = tap_ld<NP>(base + a_off + 512 * k, L::OFF_LO);
#pragma unroll
    for (int t = 0; t < 2; ++t) wt[t] = tap_ld_tr<NP>(base + t_off + 1024 * t, 512, L::OFF_LO);
#if BEVR_TAP_G2
    TapOp<NP> c[4], wt1[2];    // the same of group 1
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = tap_ld<NP>(base + a1_off + 512 * k, L::OFF_LO);
#pragma unroll
    for (int t = 0; t < 2; ++t) wt1[t] = tap_ld_tr<NP>(base + t1_off + 1024 * t, 512, L::OFF_LO);
#endif
#if BEVR_DROP
    const uint32_t kh0 = tap_drop_key0(key0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)ct[3]), kg);
    const uint32_t kh1 = kh0 + 32u * 0xC2B2AE3Du;
#else
    const uint32_t kh0 = 0u, kh1 = 0u;
#endif
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (NB > 1 && blk0 + nb >= nblk) continue;
#if BEVR_TAP_G2
      tile(a[0], a[1], wt[0], bop[nb], nb, kh0, c[0], c[1], wt1[0]);
      tile(a[2], a[3], wt[1], bop1[nb], nb, kh1, c[2], c[3], wt1[1]);
#else
      tile(a[0], a[1], wt[0], bop[nb], nb, kh0);
      tile(a[2], a[3], wt[1], bop1[nb], nb, kh1);
#endif
    }
  }

  // ---- epilogue: R[q][4 kg .. 4 kg + 3]; flag the column if a row's mass is not a healthy number -----------------
  // fp16: the weights 2^(S - mref) are rounded to fp16 before the R product -- under 2^-14 with an absolute error of up to
  // 2^-25 (zero under 2^-25), so Np keys move a row's sum by up to Np 2^-25: a row whose sum is under Np 2^-14 (the
  // error could exceed 2^-11 of it) flags its column as an underflowed row does.  The exact pass keeps its weights <= 1
  // against the running maximum.  (bf16 and the split mode: 8 exponent bits, the float's own underflow is the limit)
  const float l_min = PREC == BEVR_PREC_F16 ? (float)d.Np * 6.103515625e-05f : 7.9e-31f;
  bool bad = false;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (blk0 + nb >= nblk) continue;
    *reinterpret_cast<f32x4*>(R + mqv[nb] * TAP_ROW + 4 * kg) = r[nb];
#if BEVR_TAP_G2
    *reinterpret_cast<f32x4*>(R + mqv[nb] * TAP_ROW + TAP_SLOTS + 4 * kg) = r1[nb];
#endif
    const int row = (blk0 + nb) * QB + li;
#if BEVR_DROP
    float lall = ls[nb];     // one cross-lane reduction: the four lane groups hold four keys of every 16 each
    lall += __shfl_xor(lall, 16);
    lall += __shfl_xor(lall, 32);
    if (kg == 0) lsum[mqv[nb]] = lall;
#endif
    if constexpr (EXACT) {
      if (kg == 0) mref[mqv[nb]] += sh[nb];
    } else {
#if BEVR_DROP
      const float l = lall;  // the UNMASKED mass: a row whose kept keys are few is not an underflowed row
#else
      const float l = r[nb][3];
#endif
      if (kg == 3 && row < d.S && !(l >= l_min && l < 3.0e38f)) bad = true;
    }
  }
  if constexpr (!EXACT) {
    if (__any(bad) && lane == 0) flags[ph * d.S + j] = 1;
  }
}

template <int PREC>
int launch(const bevr_attn_desc& d, const void* G, const void* tap_ws, const float* table_pair,
           float* mref, float* R, int* flags, hipStream_t st BEVR_TAP_FWD_DROP_PARAMS) {
  typedef LdsTp<PREC> L;
  const int n_ph = d.n_prob * d.heads;
  const int grid = ((n_ph + 7) / 8) * 8 * d.S;
  const int nblk = (d.S + QB - 1) / QB;
  const size_t lds = 2 * L::BUF + (size_t)L::RING * nblk * QB * 32 * tap_np<PREC>;
  if (lds > 160 * 1024) return BEVR_E_SHAPE;
  const int nb = nblk <= 7 ? 1 : nblk <= 14 ? 2 : 4;      // row blocks per wave: at most 7 row-block waves + the producer
  if (nblk > 28) return BEVR_E_SHAPE;
  const int n_cw = (nblk + nb - 1) / nb;
  const dim3 block(64 * (n_cw + 1));
#define BEVR_TAP_LAUNCH(NB_, EX_)                                                                                     \
  hipLaunchKernelGGL((attn_tap_fwd_kernel<PREC, NB_, EX_>), dim3(grid), block, lds, st, d, (const char*)G,          \
                     (const char*)tap_ws, (const char*)table_pair, mref, R, flags BEVR_TAP_FWD_DROP_ARGS)
  for (int ex = 0; ex < 2; ++ex) {
    if (nb == 1) { if (ex) BEVR_TAP_LAUNCH(1, true); else BEVR_TAP_LAUNCH(1, false); }
    else if (nb == 2) { if (ex) BEVR_TAP_LAUNCH(2, true); else BEVR_TAP_LAUNCH(2, false); }
    else { if (ex) BEVR_TAP_LAUNCH(4, true); else BEVR_TAP_LAUNCH(4, false); }
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
#undef BEVR_TAP_LAUNCH
  return BEVR_OK;
}

// The contract of every tap forward entry point.  PRECS: the modes this translation unit holds the kernels of.
template <int... PRECS>
int run(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair, float* mref, float* R,
        int* flags, void* stream BEVR_TAP_FWD_DROP_PARAMS) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!G || !tap_ws || !table_pair || !mref || !R || !flags) return BEVR_E_NULL;
  if (d->groups != TAP_NG || (BEVR_TAP_G2 && (d->heads & 1))) return BEVR_E_SHAPE;
  if (!bevr_aligned16(G) || !bevr_aligned16(tap_ws) || !bevr_aligned16(table_pair) || !bevr_aligned16(R)) return BEVR_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
#if !BEVR_DROP && !BEVR_TAP_X3 && !BEVR_TAP_G2
  // the split mode's kernels are attn_tap_fwd_x3.hip's
  if (d->precision == BEVR_PREC_BF16X3) return bevr_tap_fwd_x3(*d, G, tap_ws, table_pair, mref, R, flags, st);
#endif
  return bevr_for_precision<PRECS...>(d->precision, [&](auto P) {
    return launch<P()>(*d, G, tap_ws, table_pair, mref, R, flags, st BEVR_TAP_FWD_DROP_ARGS);
  });
}

}  // namespace

#if BEVR_TAP_G2
// two channel groups: this translation unit is attn_tap_fwd_g2.hip, an entry point of its own (16-bit modes, no keep mask)
extern "C" int bevr_attn_tap_g2_fwd(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair,
                                    float* mref, float* R, int* flags, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, tap_ws, table_pair, mref, R, flags, stream);
}
#elif BEVR_TAP_X3 && !BEVR_DROP
// the split-mode instantiations: this translation unit is attn_tap_fwd_x3.hip, entered from bevr_attn_tap_fwd
int bevr_tap_fwd_x3(const bevr_attn_desc& d, const void* G, const void* tap_ws, const float* table_pair, float* mref,
                    float* R, int* flags, hipStream_t st) {
  return launch<BEVR_PREC_BF16X3>(d, G, tap_ws, table_pair, mref, R, flags, st);
}
#elif BEVR_TAP_X3
// the split-mode instantiations with the keep mask: this translation unit is attn_tap_fwd_x3_drop.hip, an entry point of
// its own
extern "C" int bevr_attn_tap_fwd_x3_dropout(const bevr_attn_desc* d, const void* G, const void* tap_ws,
                                            const float* table_pair, float* mref, float* R, float* lsum, int* flags,
                                            unsigned key0, unsigned drop_thr, unsigned drop_seed, void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  if (!lsum) return BEVR_E_NULL;
  return run<BEVR_PREC_BF16X3>(d, G, tap_ws, table_pair, mref, R, flags, stream BEVR_TAP_FWD_DROP_ARGS);
}
#elif BEVR_DROP
extern "C" int bevr_attn_tap_fwd_dropout(const bevr_attn_desc* d, const void* G, const void* tap_ws,
                                         const float* table_pair, float* mref, float* R, float* lsum, int* flags,
                                         unsigned key0, unsigned drop_thr, unsigned drop_seed, void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  if (!lsum) return BEVR_E_NULL;
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, tap_ws, table_pair, mref, R, flags, stream BEVR_TAP_FWD_DROP_ARGS);
}
#else
extern "C" int bevr_attn_tap_fwd(const bevr_attn_desc* d, const void* G, const void* tap_ws,
                                 const float* table_pair, float* mref, float* R, int* flags, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, tap_ws, table_pair, mref, R, flags, stream);
}
#endif
