// TAP kernels: attention over the key segment the projector PINS to feature pixel (0, 0), without K and V.
//
// Reference arithmetic (model/SCA_deform_attn.py:290-321, 331-413; model/bev_cmr_proj.py:76).  A pillar point outside a
// camera's image is projected to the normalised reference (-1, -1) = feature pixel (0, 0); its sampling position
// differs from that pixel only by the learned offset, tanh(.) * 5 / (Hk - 1) in y and 5 / (Wk - 1) in x, i.e. at most
// +-2.5 (Hi - 1) / (Hk - 1) x +-2.5 (Wi - 1) / (Wk - 1) feature pixels (+-1.6 x +-0.44 at the benchmark shape).  With
// zero padding outside the image EVERY such key samples inside the top-left TAP_R x TAP_C pixels f_t:
//     x_s(n) = sum_t w_t(n) f_t,      w_t(n) = hat(r_t - ys_n) hat(c_t - xs_n)        (bilinear weights, hat(u) = max(0, 1 - |u|))
//     K_n = Wk x_s(n) + bk = sum_t w_t(n) Kpix_t + bk,     V_n likewise        (proj_k / proj_v are 1x1 convolutions: linear)
// so for one (problem, head)
//     S[n][i]  = scale Q_i . K_n + bias = sum_t w_t(n) G[t][i] + Gb[i] + bias[n][i],    G[t][i] = scale Kpix_t . Q_i
//     O_i      = sum_n P[n][i] V_n      = sum_t R[t][i] Vpix_t + l_i bv,                R[t][i] = sum_n w_t(n) P[n][i]
// G is a (12 x M) GEMM and O = R Vpix a (M x 12) x (12 x c) one, both left to the caller (rocBLAS / torch autograd); what
// remains per (query, key) pair is ONE contraction over [12 taps | 16 bias cells] (attn_cell.h: the bias of a cell-sorted
// 32-key tile is a product with the 4 x 4 table chunk shifted by the query's BEV row), the exponential, and
// R += w^T P -- no K / V tile is staged or read, and the head width never enters.
//
// Matrix shapes: v_mfma_f32_16x16x32 (contraction 32 = 16 tap slots + 16 cells).  A tile is 16 keys x 16 BEV rows:
//   S^T[key][row]  = A[key][k] B[k][row],       A = [w | Wc] (lane = key), B = [G ; Tsh] (lane = BEV row); the row's offset
//                                                Gb - reference rides in two slots of G (hi + lo parts) against ones in w
//   R[slot][row]  += w^T[slot][key] P[key][row]  the accumulator of S^T (rows = keys) is the B operand as it stands; w^T
//                                                comes out of the SAME LDS image as A through ds_read_b64_tr_b16
// Slot TAP_ONE of w is the constant 1: row TAP_ONE of R is the softmax denominator (no VALU row sum); slot TAP_DEAD is 1
// for a masked key and G[TAP_DEAD][.] = -big: a masked key's weight is exp2(-big) = 0 with no compare in the loop.
#pragma once
#include "attn_cell.h"

constexpr int TAP_R = 4;        // feature rows 0..3 and
constexpr int TAP_C = 3;        // columns 0..2: slot t = r * TAP_C + c  (ys < 3, xs < 2: the caller checks the offset range)
constexpr int TAP_N = TAP_R * TAP_C;
constexpr int TAP_SLOTS = 16;   // 12 taps, TAP_CHI, TAP_CLO, TAP_DEAD, TAP_ONE
constexpr int TAP_CHI = 12;     // key side 1; query side the hi and lo 16-bit parts of the row's logit offset (Gb - reference):
constexpr int TAP_CLO = 13;     //   the MFMA adds it, no accumulator start registers
constexpr int TAP_DEAD = 14;
constexpr int TAP_ONE = 15;
constexpr int QB = 16;          // BEV rows per matrix tile

typedef __attribute__((ext_vector_type(4))) short s16x4;

// TWO CHANNEL GROUPS (attn_tap_*_g2.hip: #define BEVR_TAP_G2 1 and #include the kernel's source; 16-bit modes).  Group g'
// samples its C / 2 channels at its own position, proj_k / proj_v mix all channels and a head's bias follows its own
// group g, so for a head of group g
//     S[n][q] = sum_g' sum_t w_t^g'(n) G^g'[t][q] + Gb[q] + bias^g[n][q],     R^g'[t][q] = sum_n w_t^g'(n) P[n][q]
// 12 tap slots per group: G, H, R, dG are TAP_ROW = 32 slots wide, block 0 (slots 0..15) as with one group and group 0's
// taps, block 1 group 1's taps in its slots 0..11 and zeros behind them.  Softmax does not care about key order and a
// head needs (a, b) of its own group only, so every (problem, group) ROW p * 2 + g has its own key order (cell-sorted
// by group g's table coordinates): its records hold (a, b) of group g and the sampling positions of BOTH groups for the
// key at that index.  The second logit product is one more depth-32 matrix product, [w^1 | 0] against [G^1 ; 0]: the
// group's weights are a third LDS image of the first's shape, read plainly for S / dP and transposed for R / dG.
#ifndef BEVR_TAP_G2
#define BEVR_TAP_G2 0
#endif
constexpr int TAP_NG = BEVR_TAP_G2 ? 2 : 1;          // channel groups of this translation unit
constexpr int TAP_ROW = TAP_SLOTS * TAP_NG;         // slots of a row of G, H, R, dG
// sampling position of group 1 for the key of a record (group 0's is the record's)
struct TapPos1 { float ys, xs; };

// per key, written by bevr_attn_tap_prep: clamped table coordinates and the sampling position in feature pixels
// (a masked key: ys = TAP_YS_DEAD, every tap weight 0)
struct TapRec { float a, b, ys, xs; };
#define TAP_YS_DEAD (-100.0f)

// workspace layout: TapRec[rows][Np] | StepBox[rows][Np / 32] (| two groups: TapPos1[rows][Np]), rows = n_prob * TAP_NG
__host__ __device__ __forceinline__ size_t tap_ws_rows(const bevr_attn_desc& d) { return (size_t)d.n_prob * TAP_NG; }
__host__ __device__ __forceinline__ size_t tap_ws_box_offset(const bevr_attn_desc& d) {
  return tap_ws_rows(d) * d.Np * sizeof(TapRec);
}
__host__ __device__ __forceinline__ size_t tap_ws_pos1_offset(const bevr_attn_desc& d) {
  return tap_ws_box_offset(d) + tap_ws_rows(d) * (d.Np / 32) * sizeof(StepBox);
}
// the record row of (problem, head): with two groups the head's group picks it
__device__ __forceinline__ int tap_key_row(const bevr_attn_desc& d, int prob, int hd) {
  return BEVR_TAP_G2 ? prob * 2 + hd / (d.heads >> 1) : prob;
}

// BEVR_PREC_BF16X3 (bevr_common.h: split-bf16 products at f32 tolerance) on the tap kernels.  Every matrix operand is two
// bf16 IMAGES, hi = bf16(x) and lo = bf16(x - hi), of the 16-bit modes' shape and addressing, the lo image a fixed
// distance behind the hi image:
//   G, H (caller-split, ops.tap_split_rows):  [2 planes][n_prob * heads * Mp rows][16 slots] bf16, plane 1 = lo
//   A = [w | Wc] in LDS (the producer splits the f32 weights):  hi images as in LdsT, the lo images LdsTn<2>::OFF_LO behind
//   Tsh ring image:  [rows][16 cells] hi, then the same lo (from the f32 pair table)
//   P, dS: split in registers after exp2
// and a product is three v_mfma_f32_16x16x32_bf16, lo hi + hi lo + hi hi (mfma16s; the logit contraction adds lo lo: mfma16s4).  The row offset c (G: Gb - reference,
// H: -delta) is carried to FOUR bf16 parts with no further product: slot TAP_CHI holds parts 0 (hi plane) and 1 (lo plane),
// slot TAP_CLO parts 2 and 3, all against w = 1 (hi image 1, lo image 0), so that hi lo + hi hi adds p0 + p1 + p2 + p3 = c
// to the last bit of the float -- the logit's large constant part is exact, and the three-term product only has to carry
// the tap and bias terms (a convex combination of 4 + 4 entries each, as in the region kernels' split mode).
// The kernels are written ONCE over an operand of NP images (TapOp below: NP = 1 in the 16-bit modes, 2 in split mode);
// the split instantiations live in translation units of their own (attn_tap_*_x3.hip: #define BEVR_TAP_X3 1 and #include
// the kernel's source).
__host__ __device__ constexpr bool tap_split(int prec) { return prec == BEVR_PREC_BF16X3; }
// the 16-bit arithmetic (conversions, packing) an operand mode's images are made with
template <int PREC> using TapHalf = Half<tap_split(PREC) ? BEVR_PREC_BF16 : PREC>;
template <int PREC> constexpr int tap_np = tap_split(PREC) ? 2 : 1;
#ifndef BEVR_TAP_X3
#define BEVR_TAP_X3 0
#endif
// entry points of the split-mode translation units (attn_tap_{fwd,bwd_q,bwd_k}_x3.hip), called from bevr_attn_tap_*
int bevr_tap_fwd_x3(const bevr_attn_desc& d, const void* G, const void* tap_ws, const float* table_pair, float* mref,
                    float* R, int* flags, hipStream_t st);
int bevr_tap_bwd_q_x3(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws, const float* table_pair,
                      float* dG, float* dtable, hipStream_t st);
int bevr_tap_bwd_k_x3(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws, const float* table_t,
                      float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x, hipStream_t st);

template <int PREC> __device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mfma16<BEVR_PREC_BF16>(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mfma16<BEVR_PREC_F16>(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <> __device__ __forceinline__ f32x4 mfma16<BEVR_PREC_BF16X3>(bf16x8 a, bf16x8 b, f32x4 c) {   // one of the three
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// split product (a_hi + a_lo)(b_hi + b_lo) without the lo lo term, small terms first
__device__ __forceinline__ f32x4 mfma16s(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}
// the LOGIT contraction S = A . [G ; Tsh] takes the fourth term too: one G entry carries a whole Q . Kpix product, tens of
// binades at a large logit scale, and lo lo <= 2^-18 |w G| per tap is 2e-3 in log2 units at |G| ~ 600
// (tests/test_gpu_tap_x3.py, the flagged-column case: 3.3e-3 against the 2e-3 limit with three terms).  The matrix pipe
// has the room (the kernels are bound by VALU issue); dP, R, dG and Z keep three terms
__device__ __forceinline__ f32x4 mfma16s4(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bl, c, 0, 0, 0);
  return mfma16s(ah, al, bh, bl, c);
}
// two floats -> the packed bf16 pair of their hi parts and of their lo parts
struct Split2 { uint32_t h, l; };
__device__ __forceinline__ Split2 split2(float x0, float x1) {
  const uint32_t h = pack_bf16x2(x0, x1);
  return Split2{h, pack_bf16x2(x0 - __builtin_bit_cast(float, h << 16), x1 - __builtin_bit_cast(float, h & 0xffff0000u))};
}
#define TAP_SPLIT2(x0_, x1_, h_, l_) do { const Split2 sp_ = split2(x0_, x1_); (h_) = sp_.h; (l_) = sp_.l; } while (0)
// One matrix operand of an operand mode: p[0] the image the 16-bit modes have, p[1] (split mode) the lo image
template <int NP> struct TapOp { bf16x8 p[NP]; };
template <int PREC> using TapOpP = TapOp<tap_np<PREC>>;
// c += a b.  LOGIT: the contraction S = A . [G ; Tsh] (split mode: four terms)
template <int PREC, bool LOGIT = false>
__device__ __forceinline__ f32x4 tap_mm(const TapOpP<PREC>& a, const TapOpP<PREC>& b, f32x4 c) {
  if constexpr (!tap_split(PREC)) return mfma16<PREC>(a.p[0], b.p[0], c);
  else if constexpr (LOGIT) return mfma16s4(a.p[0], a.p[1], b.p[0], b.p[1], c);
  else return mfma16s(a.p[0], a.p[1], b.p[0], b.p[1], c);
}
// two floats -> dword k of every image (split mode: the pair's hi parts and lo parts)
template <int PREC> __device__ __forceinline__ void tap_pack2(float x0, float x1, int k, u32x4 (&w)[tap_np<PREC>]) {
  if constexpr (tap_split(PREC)) TAP_SPLIT2(x0, x1, w[0][k], w[1][k]);
  else w[0][k] = TapHalf<PREC>::pack2(x0, x1);
}
template <int NP> __device__ __forceinline__ TapOp<NP> tap_op(const u32x4 (&w)[NP]) {
  TapOp<NP> o;
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) o.p[pl] = __builtin_bit_cast(bf16x8, w[pl]);
  return o;
}
// eight floats (accumulator values of two 16-key sub-tiles, or eight weights) -> one operand register per image
template <int PREC> __device__ __forceinline__ TapOpP<PREC> tap_pack8(const float (&x)[8]) {
  u32x4 w[tap_np<PREC>];
#pragma unroll
  for (int k = 0; k < 4; ++k) tap_pack2<PREC>(x[2 * k], x[2 * k + 1], k, w);
  return tap_op(w);
}
// 16 bytes of every image at `p`, image pl `stride` bytes behind image pl - 1
template <int NP> __device__ __forceinline__ TapOp<NP> tap_ld(const char* p, size_t stride) {
  TapOp<NP> o;
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) o.p[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p + pl * stride));
  return o;
}
template <int NP> __device__ __forceinline__ void tap_st(char* p, size_t stride, const TapOp<NP>& o) {
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<u32x4*>(p + pl * stride) = __builtin_bit_cast(u32x4, o.p[pl]);
}

// two transposed LDS reads (4 rows x 16 columns of 16-bit each, rows 32 B apart in a [key][16] image): element e of
// the result = image[row r0 + e (e < 4) | r1 + e - 4][column lane & 15].  `p` is this lane's address in the first block
// (row r0 + ((lane & 15) >> 2), byte 8 (lane & 3)), `off2` the byte distance to the second block.
__device__ __forceinline__ bf16x8 lds_tr8(const char* p, int off2) {
  typedef s16x4 __attribute__((address_space(3)))* lp;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p + off2));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
template <int NP> __device__ __forceinline__ TapOp<NP> tap_ld_tr(const char* p, int off2, int stride) {
  TapOp<NP> o;
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) o.p[pl] = lds_tr8(p + pl * stride, off2);
  return o;
}

// the 16 tap slots of one key: t[0] slots 0..7, t[1] slots 8..15
template <int PREC> __device__ __forceinline__ void tap_weights(float ys, float xs, TapOpP<PREC> (&t)[2]) {
  float wy[TAP_R], wx[TAP_C], w[2][8];
#pragma unroll
  for (int r = 0; r < TAP_R; ++r) wy[r] = hat((float)r - ys);
#pragma unroll
  for (int c = 0; c < TAP_C; ++c) wx[c] = hat((float)c - xs);
#pragma unroll
  for (int r = 0; r < TAP_R; ++r)
#pragma unroll
    for (int c = 0; c < TAP_C; ++c) w[(r * TAP_C + c) >> 3][(r * TAP_C + c) & 7] = wy[r] * wx[c];
  w[1][TAP_CHI - 8] = 1.0f;
  w[1][TAP_CLO - 8] = 1.0f;
  w[1][TAP_DEAD - 8] = ys < -50.0f ? 1.0f : 0.f;
  w[1][TAP_ONE - 8] = 1.0f;
  t[0] = tap_pack8<PREC>(w[0]);
  t[1] = tap_pack8<PREC>(w[1]);
}

#if BEVR_TAP_G2
// the slot weights of group 1 for one key: the 12 taps alone (the constant slots ride in group 0's image)
template <int PREC> __device__ __forceinline__ void tap_weights1(float ys, float xs, TapOpP<PREC> (&t)[2]) {
  float wy[TAP_R], wx[TAP_C], w[2][8];
#pragma unroll
  for (int r = 0; r < TAP_R; ++r) wy[r] = hat((float)r - ys);
#pragma unroll
  for (int c = 0; c < TAP_C; ++c) wx[c] = hat((float)c - xs);
#pragma unroll
  for (int r = 0; r < TAP_R; ++r)
#pragma unroll
    for (int c = 0; c < TAP_C; ++c) w[(r * TAP_C + c) >> 3][(r * TAP_C + c) & 7] = wy[r] * wx[c];
#pragma unroll
  for (int k = TAP_N; k < TAP_SLOTS; ++k) w[1][k - 8] = 0.f;
  t[0] = tap_pack8<PREC>(w[0]);
  t[1] = tap_pack8<PREC>(w[1]);
}
#endif

// cells 8 hf .. 8 hf + 7 of the bias chunk for one key, the arithmetic and the order of cell_weights (attn_cell.h):
// element e = column 2 hf + (e >> 2), row e & 3
template <int PREC> __device__ __forceinline__ TapOpP<PREC> tap_cell_half(float tcol, float trow, int hf) {
  const float wx0 = hat((float)(2 * hf) - tcol), wx1 = hat((float)(2 * hf + 1) - tcol);
  float w[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float wy = hat((float)r - trow);
    w[r] = wx0 * wy;
    w[4 + r] = wx1 * wy;
  }
  return tap_pack8<PREC>(w);
}

// Attention dropout (bevr_common.h: bevr_drop_keep).  The dropout variants are separate translation units
// (attn_tap_*_drop.hip: #define BEVR_DROP 1 and #include the kernel's source), as the region kernels': the kernels
// without dropout stay what they were.  key0: index of the segment's first key in the caller's key order for the whole
// call -- the mask is hashed with n = key0 + (index inside the segment), so that the segments of one softmax share ONE
// mask (ops.py:dropout_keep_mask over all N keys).  Dropout acts on P after the softmax: R accumulates the kept weights
// (slot TAP_ONE: the kept mass), the row sum of ALL weights goes out on its own (lsum), and the logit gradient is
// dS = P (keep ? D dP : 0 - delta), the droppable part D dP = w . H + H[TAP_ONE] (the caller folds D into H), -delta in
// slots TAP_CHI / TAP_CLO of H as without dropout.
#if BEVR_DROP
#define TAP_DROP_PARAMS , unsigned key0, unsigned drop_thr, unsigned drop_seed
#define TAP_DROP_ARGS , key0, drop_thr, drop_seed
// The key part of the hash, n * 0xC2B2AE3D, for the 8 keys of a 32-key tile whose logits a lane of the query-stationary
// kernels holds (element k: key n0 + 4 kg + (k & 3) + 16 (k >> 2)): one register per tile (the first key's product), the
// other seven differ from it by constants (the product is linear modulo 2^32)
__device__ __forceinline__ uint32_t tap_drop_key0(uint32_t n0, int kg) { return (n0 + (uint32_t)(4 * kg)) * 0xC2B2AE3Du; }
__device__ __forceinline__ bool tap_drop_keep(uint32_t hrow, uint32_t kh, uint32_t thr16) {
#if defined(BEVR_VARIANT) && BEVR_VARIANT == 31
  // A/B timing only (make VARIANT=31): the mask without the mixing rounds (a WRONG mask) -- what is left of the dropout
  // kernels' extra time is not the hash's
  return ((hrow ^ kh) >> 16) >= thr16;
#else
  return (bevr_drop_mix(hrow ^ kh) >> 16) >= thr16;
#endif
}
__device__ __forceinline__ bool tap_drop_keep8(uint32_t hrow, uint32_t kh0, int k, uint32_t thr16) {
  return tap_drop_keep(hrow, kh0 + (uint32_t)(16 * (k >> 2) + (k & 3)) * 0xC2B2AE3Du, thr16);
}
// Split mode: what a DROPPED pair keeps of the H product, -delta, out of its four bf16 parts.  hi2 / lo2: the dword at
// slots TAP_CHI, TAP_CLO of the row's hi and lo image, (p0, p2) and (p1, p3); smallest parts first: the float they were
// split from, bit for bit (the kept pairs get the same four parts through the matrix product against w = 1).  In both
// modes slot TAP_ONE of H (the kept mass's cotangent, droppable) is not part of it; in split mode that slot holds a
// (hi, lo) pair like the tap slots, contracted with w = (1, 0) to hi + lo
__device__ __forceinline__ float tap_drop_ndel4(uint32_t hi2, uint32_t lo2) {
  typedef Half<BEVR_PREC_BF16> B;
  return ((B::hi(lo2) + B::hi(hi2)) + B::lo(lo2)) + B::lo(hi2);
}
#else
#define TAP_DROP_PARAMS
#define TAP_DROP_ARGS
#endif

// ---------------------------------------------------------------------------------------------------------------
// The key stream of the query-stationary tap kernels (forward, query-side backward): LDS layout and the producer wave.
// NP: images per operand (1; split mode 2: the lo images of taps and cells OFF_LO behind the hi images)
template <int NP> struct LdsTn {
  static constexpr int OFF_TAPS = 0;            // [64 keys][16 slots] 16-bit
  static constexpr int OFF_CELLS = 2048;        // [64 keys][16 cells] 16-bit
  static constexpr int OFF_LO = 4096;
  static constexpr int OFF_TAPS1 = 4096 * NP;   // two groups: [64 keys][16 slots] 16-bit, group 1's weights
  static constexpr int G2B = BEVR_TAP_G2 ? 2048 : 0;
  static constexpr int OFF_CT = 4096 * NP + G2B;   // u32x4: flags (bit 0 / 1: tile 0 / 1 live, bit 2: done), alloc0, alloc1, 0
                                                //        (dropout build: the 4th dword = record index of tile 0's first key)
  static constexpr int OFF_ORG = 4096 * NP + G2B + 16;   // i32x4: chunk origin of tile 0 (x0, a0), of tile 1 (x0, a0)
  static constexpr int BUF = 4096 * NP + G2B + 32;
  static constexpr int RING = 4;
};
typedef LdsTn<1> LdsT;
template <int PREC> using LdsTp = LdsTn<tap_np<PREC>>;

__device__ __forceinline__ bool box_fits(const StepBox& sb, float jrx) {
  const int x0 = (int)floorf(jrx + sb.bmin), x1 = (int)floorf(jrx + sb.bmax) + 1;
  return sb.amax >= sb.amin && (x1 - x0 < CELL_C) && (sb.amax + 1 - sb.amin < CELL_R);
}

// The producer wave of the query-stationary tap kernels.  Emits the key stream of (problem `prob`, column j) into the two
// LDS buffers at `smem` and the ring of table images behind them; one __syncthreads() per emission, a final one with the
// done flag.  rows_img = BEV rows covered by an image (16 x row blocks of the column).
template <int PREC>
__device__ __forceinline__ void tap_producer(const bevr_attn_desc& d, char* smem, char* ring, int img_bytes, int rows_img,
                                             const TapRec* __restrict__ recs, const StepBox* __restrict__ box,
#if BEVR_TAP_G2
                                             const TapPos1* __restrict__ pos1,
#endif
                                             const char* __restrict__ tbl, float jrx, int lane) {
  typedef LdsTp<PREC> L;
  const int hi = lane >> 5;
  const int n_step = d.Np / KT;
  int alloc = 0, tag_x = 1 << 30, tag_a = 1 << 30;
  int e = 0;
  // the producer is the workgroup's pacemaker: every other wave waits for its emission at the barrier, and it shares
  // its SIMD with row-block waves that would otherwise take most of the issue slots
  __builtin_amdgcn_s_setprio(3);
  // the table side of chunk origin (x0, a0): image[row][cell 4 c + r] = T2[x0 + c][a0 + row + r], 16-bit
  // (split mode: img_bytes covers the hi rows and, rows_img * 32 behind them, the lo rows)
  auto build_image = [&](char* img, int x0, int a0) {
    for (int row = lane; row < rows_img; row += 64) {
      const int yr0 = a0 + row + d.y_off;
      const int e0 = max(0, min(yr0, d.Hp - 1)), e2 = max(0, min(yr0 + 2, d.Hp - 1));
      float w[2][8];     // cells 0..7 | 8..15 of the row
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int xc = max(0, min(x0 + c + d.x_off, d.Wp - 1));
        const char* col = tbl + (size_t)xc * d.Hp * 8;
        const f32x2 p0 = *reinterpret_cast<const f32x2*>(col + (size_t)e0 * 8);
        const f32x2 p2 = *reinterpret_cast<const f32x2*>(col + (size_t)e2 * 8);
        w[c >> 1][4 * (c & 1)] = p0[0];
        w[c >> 1][4 * (c & 1) + 1] = p0[1];
        w[c >> 1][4 * (c & 1) + 2] = p2[0];
        w[c >> 1][4 * (c & 1) + 3] = p2[1];
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) tap_st(img + row * 32 + 16 * k, rows_img * 32, tap_pack8<PREC>(w[k]));
    }
  };
  // image 0 stands for "no chunk yet" (allocation numbers start at 1): finite values for the masked keys of a slot that
  // precedes every live tile
  for (int o = lane * 16; o < img_bytes; o += 64 * 16) *reinterpret_cast<u32x4*>(ring + o) = u32x4{0u, 0u, 0u, 0u};
  TapRec rc_n = recs[lane];
  StepBox sb_n = box[hi];
#if BEVR_TAP_G2
  TapPos1 p1_n = pos1[lane];
#endif
  for (int step = 0; step < n_step; ++step) {
    const TapRec rc = rc_n;
    const StepBox sb = sb_n;
#if BEVR_TAP_G2
    const TapPos1 p1 = p1_n;
    if (step + 1 < n_step) p1_n = pos1[(size_t)(step + 1) * KT + lane];
#endif
    if (step + 1 < n_step) {   // the next step's records are in flight while this one is emitted
      rc_n = recs[(size_t)(step + 1) * KT + lane];
      sb_n = box[2 * (step + 1) + hi];
    }
    bool rem = rc.ys > -50.0f;                       // keys of this lane's tile not emitted yet
    if (__ballot(rem) == 0ull) continue;             // a step of padding only: nothing to emit
    const int A = (int)floorf(rc.a);
    const float tx = jrx + rc.b;
    const float xf = floorf(tx);
    const int X = (int)xf;
    bool whole = box_fits(sb, jrx);                  // uniform over the half: the tile's own box fits one chunk
    do {
      int a0, x0;
      bool sel;
      if (whole) {
        a0 = sb.amin;
        x0 = (int)floorf(jrx + sb.bmin);
        sel = rem;
      } else {
        // one chunk's worth of the remaining keys: rows from the lowest remaining key, columns from the lowest key
        // among those (that key is always selected: progress)
        a0 = lanes_min<32>(rem ? A : 0x7fffffff);
        const bool rowok = rem && A < a0 + CELL_R - 1;
        x0 = lanes_min<32>(rowok ? X : 0x7fffffff);
        sel = rowok && X < x0 + CELL_C - 1;
      }
      whole = false;
      const unsigned long long selm = __ballot(sel);
      const int ok0 = (selm & 0xffffffffull) != 0ull, ok1 = (selm >> 32) != 0ull;
      char* bb = smem + (e & 1) * L::BUF;
      TapOpP<PREC> t[2];
      tap_weights<PREC>(sel ? rc.ys : TAP_YS_DEAD, rc.xs, t);
      const float tcol = sel ? (xf - (float)x0) + (tx - xf) : -8.0f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        tap_st(bb + L::OFF_TAPS + lane * 32 + 16 * k, L::OFF_LO, t[k]);
        tap_st(bb + L::OFF_CELLS + lane * 32 + 16 * k, L::OFF_LO, tap_cell_half<PREC>(tcol, rc.a - (float)a0, k));
      }
#if BEVR_TAP_G2
      tap_weights1<PREC>(sel ? p1.ys : TAP_YS_DEAD, p1.xs, t);
#pragma unroll
      for (int k = 0; k < 2; ++k) tap_st(bb + L::OFF_TAPS1 + lane * 32 + 16 * k, L::OFF_LO, t[k]);
#endif
      int al0 = alloc, al1 = alloc, ox0 = tag_x, oa0 = tag_a;
      if (ok0) {
        const int x = __builtin_amdgcn_readlane(x0, 0), a = __builtin_amdgcn_readlane(a0, 0);
        if (x != tag_x || a != tag_a) {
          ++alloc;
          build_image(ring + (alloc & (L::RING - 1)) * img_bytes, x, a);
          tag_x = x;
          tag_a = a;
        }
        al0 = alloc;
        ox0 = tag_x;
        oa0 = tag_a;
      }
      if (ok1) {
        const int x = __builtin_amdgcn_readlane(x0, 32), a = __builtin_amdgcn_readlane(a0, 32);
        if (x != tag_x || a != tag_a) {
          ++alloc;
          build_image(ring + (alloc & (L::RING - 1)) * img_bytes, x, a);
          tag_x = x;
          tag_a = a;
        }
        al1 = alloc;
      }
      if (lane == 0) {
#if BEVR_DROP
        // dropout: the record index of the emission's first slot (lane l is key step * KT + l of the segment in EVERY
        // masked pass of the step: one keep decision per key)
        *reinterpret_cast<u32x4*>(bb + L::OFF_CT) = u32x4{(unsigned)(ok0 | (ok1 << 1)), (unsigned)al0, (unsigned)al1, (unsigned)(step * KT)};
#else
        *reinterpret_cast<u32x4*>(bb + L::OFF_CT) = u32x4{(unsigned)(ok0 | (ok1 << 1)), (unsigned)al0, (unsigned)al1, 0u};
#endif
        *reinterpret_cast<u32x4*>(bb + L::OFF_ORG) = u32x4{(unsigned)ox0, (unsigned)oa0, (unsigned)tag_x, (unsigned)tag_a};
      }
      rem = rem && !sel;
      ++e;
      __syncthreads();
    } while (__ballot(rem) != 0ull);
  }
  if (lane == 0) *reinterpret_cast<u32x4*>(smem + (e & 1) * L::BUF + L::OFF_CT) = u32x4{4u, 0u, 0u, 0u};
  __syncthreads();
}

