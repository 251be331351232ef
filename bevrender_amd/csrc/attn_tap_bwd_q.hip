// Query-side backward of the tap kernels (attn_tap.h).  With P[n][q] = exp2(S[n][q] - LSE[q]) recomputed as in the forward,
//     dP[n][q] = dO_q . V_n = sum_t w_t(n) H[t][q] + Hb[q],         H[t][q] = Vpix_t . dO_q, Hb = bv . dO_q
//     dS[n][q] = ln2 P (dP - delta[q])                              (the caller folds ln2 and delta into H and Hc)
//     dG[k][q] = sum_n A[n][k] dS[n][q],    A = [w | Wc]:   rows 0..15 the gradient of G (row TAP_ONE: of Gb), rows 16..31
//                                                           the gradient of the chunk's 16 table cells shifted by q
// (reference: the backward of model/SCA_deform_attn.py:331-413 through autograd).  dQ and dKpix follow from dG by two thin
// GEMMs in the caller; dV needs nothing from here (dVpix = Rn^T dO with the forward's R).
//
// Same decomposition and key stream as attn_tap_fwd.hip (workgroup = one BEV column, row-block waves + the producer of
// attn_tap.h).  Per 32-key tile and 16-row block: S^T and dP^T (2 + 2 MFMAs, the SAME A operand), 8 exponentials, 8
// products, one conversion of dS to 16 bits that feeds both dG products (A = w^T and Wc^T through ds_read_b64_tr_b16
// from the images the producer wrote).  The cell half of dG lives in 4 registers per row block while the chunk origin
// stays and is flushed into the table gradient with float atomics when it changes (~1 tile in 30).
#include "attn_tap.h"
#include "attn_host.h"

namespace {

// (split mode: every operand twice -- the fat NB = 4 instantiation gets the registers of 2 waves per SIMD; with the keep
// mask NB = 2 spills 84 bytes a lane at the 128 registers of 4 waves: 3)
constexpr int tap_bwd_q_waves(int prec, int nb) {
  // (two groups: two more B operands and one more accumulator per row block -- the fat instantiation as the split mode's)
  // (NB = 2 with two groups spills 12 bytes a lane in fp16 at the 128 registers of 4 waves: 3)
  return (tap_split(prec) || BEVR_TAP_G2) && nb == 4 ? 2 : ((tap_split(prec) && BEVR_DROP) || BEVR_TAP_G2) && nb == 2 ? 3 : 4;
}
template <int PREC, int NB>
__global__ __launch_bounds__(512, tap_bwd_q_waves(PREC, NB)) void attn_tap_bwd_q_kernel(
    bevr_attn_desc d, const char* __restrict__ G, const char* __restrict__ H, const char* __restrict__ tap_ws, const char* __restrict__ table_pair,
    float* __restrict__ dG, float* __restrict__ dtable TAP_DROP_PARAMS) {
  typedef LdsTp<PREC> L;
  constexpr int NP = tap_np<PREC>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int n_ph = d.n_prob * d.heads;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int ph = (slot / d.S) * 8 + xcd;
  if (ph >= n_ph) return;
  const int j = slot % d.S;
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

  const int blk0 = wave * NB;
  TapOp<NP> bop[NB];     // lanes 0..31 G[q][8 kg ..], lanes 32..63 the chunk's table side
  TapOp<NP> hop[NB];     // lanes 0..31 H[q][8 kg ..], lanes 32..63 zero
  f32x4 ytap[NB], ycell[NB];
  size_t mqv[NB];
#if BEVR_TAP_G2
  TapOp<NP> bop2[NB], hop2[NB];     // group 1: lanes 0..31 G / H[q][16 + 8 kg ..], lanes 32..63 zero
  f32x4 ytap1[NB];
#endif
  const size_t g_lo = (size_t)n_ph * Mp * TAP_SLOTS * 2;     // the lo planes of G and H
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int blk = min(blk0 + nb, nblk - 1);
    const size_t mq = (size_t)ph * Mp + (size_t)j * d.Sp + blk * QB + li;
    mqv[nb] = mq;
    bop[nb] = hop[nb] = TapOp<NP>{};
    if (kg < 2) {
      bop[nb] = tap_ld<NP>(G + (mq * TAP_ROW + 8 * kg) * 2, g_lo);
      hop[nb] = tap_ld<NP>(H + (mq * TAP_ROW + 8 * kg) * 2, g_lo);
    }
#if BEVR_TAP_G2
    bop2[nb] = hop2[nb] = TapOp<NP>{};
    if (kg < 2) {
      bop2[nb] = tap_ld<NP>(G + (mq * TAP_ROW + TAP_SLOTS + 8 * kg) * 2, g_lo);
      hop2[nb] = tap_ld<NP>(H + (mq * TAP_ROW + TAP_SLOTS + 8 * kg) * 2, g_lo);
    }
    ytap1[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#endif
    ytap[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    ycell[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#if BEVR_DROP
  // dropout: dS = P (keep ? D dP : 0 - delta).  The MFMA gives x = D dP - delta (D dP = w . H + H[TAP_ONE], -delta in slots
  // TAP_CHI / TAP_CLO); a dropped pair keeps -delta alone, which every lane reads for its row once, with the row hash
  uint32_t hrow[NB];
  float ndel[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    hrow[nb] = bevr_drop_row(drop_seed, (uint32_t)ph, (uint32_t)(j * d.Sp + min(blk0 + nb, nblk - 1) * QB + li));
    const uint32_t c2 = *reinterpret_cast<const uint32_t*>(H + (mqv[nb] * TAP_ROW + TAP_CHI) * 2);
    ndel[nb] = TapHalf<PREC>::lo(c2) + TapHalf<PREC>::hi(c2);
    if constexpr (tap_split(PREC)) ndel[nb] = tap_drop_ndel4(c2, *reinterpret_cast<const uint32_t*>(H + g_lo + (mqv[nb] * TAP_ROW + TAP_CHI) * 2));
  }
#endif
  const int a_off = (kg < 2 ? L::OFF_TAPS : L::OFF_CELLS) + li * 32 + (kg & 1) * 16;     // + tile * 1024 + sub * 512
  const int t_off = (4 * kg + (li >> 2)) * 32 + (lane & 3) * 8;                           // transposed reads: + image, + tile * 1024
  const int i_off = li * 32 + (kg & 1) * 16;
  int have = 0, org_x = 0, org_a = 0;   // the chunk in bop / ycell: allocation number (0: none yet) and origin

  // table gradient of the chunk in ycell: cell (c = kg, r) of BEV row q is table entry (org_x + c, org_a + q + r)
  float* dth = dtable + (size_t)hd * d.Wp * (d.Hp + 1);
  // Rows q and q + 1 of a block overlap in three of their four cells: cell r of row q is table row org_a + q + r.  The four
  // contributions to one table row are summed across the block's lanes first (one atomic per lane instead of four; the
  // last three lanes add the rows past the block's sixteenth on their own): 2.9x fewer atomics
  auto flush = [&]() {
    const int xc = org_x + kg + d.x_off;
    const bool col_ok = xc >= 0 && xc < d.Wp;
    float* col = dth + (size_t)(col_ok ? xc : 0) * (d.Hp + 1);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (NB > 1 && blk0 + nb >= nblk) continue;       // uniform
      const f32x4 c = ycell[nb];
      float s = c[0];
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        const float up = __shfl_up(c[r], r, QB);        // cell r of the row r lanes below
        s += li >= r ? up : 0.f;
      }
      const int y0 = org_a + (blk0 + nb) * QB + li + d.y_off;
      if (col_ok) {
        if (y0 >= 0 && y0 <= d.Hp) atomicAdd(col + y0, s);
#pragma unroll
        for (int r = 1; r < 4; ++r) {                   // table rows past the block's sixteenth
          const int y = y0 + r;
          if (li + r >= QB && y >= 0 && y <= d.Hp) atomicAdd(col + y, c[r]);
        }
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) ycell[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  // one 32-key tile against the wave's row blocks (kh: the tile's key hash, dropout builds)
  auto tile = [&](const char* base, int t, [[maybe_unused]] uint32_t kh) {
    const TapOp<NP> a0 = tap_ld<NP>(base + a_off + t * 1024, L::OFF_LO);
    const TapOp<NP> a1 = tap_ld<NP>(base + a_off + t * 1024 + 512, L::OFF_LO);
    const TapOp<NP> wt = tap_ld_tr<NP>(base + L::OFF_TAPS + t_off + t * 1024, 512, L::OFF_LO);
    const TapOp<NP> wct = tap_ld_tr<NP>(base + L::OFF_CELLS + t_off + t * 1024, 512, L::OFF_LO);
#if BEVR_TAP_G2
    // group 1's image: plainly (lanes 32..63 read what lanes 0..31 do, against zeros) and transposed
    const TapOp<NP> c0 = tap_ld<NP>(base + L::OFF_TAPS1 + li * 32 + (kg & 1) * 16 + t * 1024, L::OFF_LO);
    const TapOp<NP> c1 = tap_ld<NP>(base + L::OFF_TAPS1 + li * 32 + (kg & 1) * 16 + t * 1024 + 512, L::OFF_LO);
    const TapOp<NP> wt1 = tap_ld_tr<NP>(base + L::OFF_TAPS1 + t_off + t * 1024, 512, L::OFF_LO);
#endif
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (NB > 1 && blk0 + nb >= nblk) continue;
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#if BEVR_TAP_G2
      const f32x4 s0 = tap_mm<PREC, true>(a0, bop[nb], tap_mm<PREC, true>(c0, bop2[nb], z4));
      const f32x4 s1 = tap_mm<PREC, true>(a1, bop[nb], tap_mm<PREC, true>(c1, bop2[nb], z4));
      const f32x4 p0 = tap_mm<PREC>(a0, hop[nb], tap_mm<PREC>(c0, hop2[nb], z4));
      const f32x4 p1 = tap_mm<PREC>(a1, hop[nb], tap_mm<PREC>(c1, hop2[nb], z4));
#else
      const f32x4 s0 = tap_mm<PREC, true>(a0, bop[nb], z4);
      const f32x4 s1 = tap_mm<PREC, true>(a1, bop[nb], z4);
      const f32x4 p0 = tap_mm<PREC>(a0, hop[nb], z4);
      const f32x4 p1 = tap_mm<PREC>(a1, hop[nb], z4);
#endif
      float ds[8];
#if BEVR_DROP
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ds[k] = fast_exp2(s0[k]) * (tap_drop_keep8(hrow[nb], kh, k, drop_thr) ? p0[k] : ndel[nb]);
        ds[4 + k] = fast_exp2(s1[k]) * (tap_drop_keep8(hrow[nb], kh, 4 + k, drop_thr) ? p1[k] : ndel[nb]);
      }
#else
#pragma unroll
      for (int k = 0; k < 8; ++k) ds[k] = fast_exp2(k < 4 ? s0[k & 3] : s1[k & 3]) * (k < 4 ? p0[k & 3] : p1[k & 3]);
#endif
      const TapOp<NP> ds8 = tap_pack8<PREC>(ds);
      ytap[nb] = tap_mm<PREC>(wt, ds8, ytap[nb]);
      ycell[nb] = tap_mm<PREC>(wct, ds8, ycell[nb]);
#if BEVR_TAP_G2
      ytap1[nb] = tap_mm<PREC>(wt1, ds8, ytap1[nb]);
#endif
    }
  };

  for (int e = 0;; ++e) {
    __syncthreads();
    const char* base = smem + (e & 1) * L::BUF;
    const u32x4 ct = *reinterpret_cast<const u32x4*>(base + L::OFF_CT);
    const u32x4 og = *reinterpret_cast<const u32x4*>(base + L::OFF_ORG);
    const int fl = __builtin_amdgcn_readfirstlane((int)ct[0]);
    if (fl & 4) break;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int al = __builtin_amdgcn_readfirstlane((int)ct[1 + t]);
      if (al != have) {   // uniform, rare: another chunk origin -- hand the old chunk's table gradient over first
        if (have != 0) flush();
        have = al;
        org_x = __builtin_amdgcn_readfirstlane((int)og[2 * t]);
        org_a = __builtin_amdgcn_readfirstlane((int)og[2 * t + 1]);
        if (kg >= 2) {
          const char* img = ring + (al & (L::RING - 1)) * img_bytes + i_off;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) bop[nb] = tap_ld<NP>(img + min(blk0 + nb, nblk - 1) * 512, rows_img * 32);
        }
      }
#if BEVR_DROP
      tile(base, t, tap_drop_key0(key0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)ct[3]) + 32u * t, kg));
#else
      tile(base, t, 0u);
#endif
    }
  }
  if (have != 0) flush();

#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (blk0 + nb >= nblk) continue;
    *reinterpret_cast<f32x4*>(dG + mqv[nb] * TAP_ROW + 4 * kg) = ytap[nb];
#if BEVR_TAP_G2
    *reinterpret_cast<f32x4*>(dG + mqv[nb] * TAP_ROW + TAP_SLOTS + 4 * kg) = ytap1[nb];
#endif
  }
}

template <int PREC>
int launch(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws,
           const float* table_pair, float* dG, float* dtable, hipStream_t st TAP_DROP_PARAMS) {
  typedef LdsTp<PREC> L;
  const int n_ph = d.n_prob * d.heads;
  const int grid = ((n_ph + 7) / 8) * 8 * d.S;
  const int nblk = (d.S + QB - 1) / QB;
  const size_t lds = 2 * L::BUF + (size_t)L::RING * nblk * QB * 32 * tap_np<PREC>;
  if (lds > 160 * 1024 || nblk > 28) return BEVR_E_SHAPE;
  const int nb = nblk <= 7 ? 1 : nblk <= 14 ? 2 : 4;
  const int n_cw = (nblk + nb - 1) / nb;
  const dim3 block(64 * (n_cw + 1));
#define BEVR_TAP_LAUNCH(NB_)                                                                                            \
  hipLaunchKernelGGL((attn_tap_bwd_q_kernel<PREC, NB_>), dim3(grid), block, lds, st, d, (const char*)G, (const char*)H,     \
                     (const char*)tap_ws, (const char*)table_pair, dG, dtable TAP_DROP_ARGS)
  if (nb == 1) BEVR_TAP_LAUNCH(1);
  else if (nb == 2) BEVR_TAP_LAUNCH(2);
  else BEVR_TAP_LAUNCH(4);
#undef BEVR_TAP_LAUNCH
  return (int)hipGetLastError();
}

// The contract of every tap bwd_q entry point.  PRECS: the modes this translation unit holds the kernels of.
template <int... PRECS>
int run(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws, const float* table_pair, float* dG,
        float* dtable, void* stream TAP_DROP_PARAMS) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!G || !H || !tap_ws || !table_pair || !dG || !dtable) return BEVR_E_NULL;
  if (d->groups != TAP_NG || (BEVR_TAP_G2 && (d->heads & 1))) return BEVR_E_SHAPE;
  if (!bevr_aligned16(G) || !bevr_aligned16(H) || !bevr_aligned16(tap_ws) || !bevr_aligned16(table_pair) || !bevr_aligned16(dG))
    return BEVR_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
#if !BEVR_DROP && !BEVR_TAP_X3 && !BEVR_TAP_G2
  // the split mode's kernels are attn_tap_bwd_q_x3.hip's
  if (d->precision == BEVR_PREC_BF16X3) return bevr_tap_bwd_q_x3(*d, G, H, tap_ws, table_pair, dG, dtable, st);
#endif
  return bevr_for_precision<PRECS...>(d->precision, [&](auto P) {
    return launch<P()>(*d, G, H, tap_ws, table_pair, dG, dtable, st TAP_DROP_ARGS);
  });
}

}  // namespace

#if BEVR_TAP_G2
// two channel groups: this translation unit is attn_tap_bwd_q_g2.hip, an entry point of its own (16-bit modes, no keep mask)
extern "C" int bevr_attn_tap_g2_bwd_q(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                      const float* table_pair, float* dG, float* dtable, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_pair, dG, dtable, stream);
}
#elif BEVR_TAP_X3 && !BEVR_DROP
// the split-mode instantiations: this translation unit is attn_tap_bwd_q_x3.hip, entered from bevr_attn_tap_bwd_q
int bevr_tap_bwd_q_x3(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws, const float* table_pair,
                      float* dG, float* dtable, hipStream_t st) {
  return launch<BEVR_PREC_BF16X3>(d, G, H, tap_ws, table_pair, dG, dtable, st);
}
#elif BEVR_TAP_X3
// the split-mode instantiations with the keep mask: this translation unit is attn_tap_bwd_q_x3_drop.hip, an entry point
// of its own
extern "C" int bevr_attn_tap_bwd_q_x3_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                              const float* table_pair, float* dG, float* dtable, unsigned key0,
                                              unsigned drop_thr, unsigned drop_seed, void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16X3>(d, G, H, tap_ws, table_pair, dG, dtable, stream TAP_DROP_ARGS);
}
#elif BEVR_DROP
extern "C" int bevr_attn_tap_bwd_q_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                           const float* table_pair, float* dG, float* dtable, unsigned key0,
                                           unsigned drop_thr, unsigned drop_seed, void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_pair, dG, dtable, stream TAP_DROP_ARGS);
}
#else
extern "C" int bevr_attn_tap_bwd_q(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                   const float* table_pair, float* dG, float* dtable, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_pair, dG, dtable, stream);
}
#endif
