// Key-side backward of the tap kernels (attn_tap.h): the gradient of every key's POSITION -- its rpe-table coordinates
// (a, b) through the bias and its sampling position (ys, xs) through the tap weights.  With P and dS as in
// attn_tap_bwd_q.hip (dS = P (w . H + Hc), ln2 and delta folded into H by the caller),
//     dw_t(n) = sum_q dS[n][q] G[t][q] + P[n][q] H[t][q] / ln2  (the logit path and the value path V_n = sum_t w_t Vpix_t)
//     Z[cell][n] = sum_q dS[n][q] Tsh[cell][q]                  per BEV column: the chunk's cells are a different part of the
//                                                                table for every column
//     d a_n = sum_c wx_c (Z[c][r0 + 1] - Z[c][r0]),   d b_n = sum_r wy_r (Z[c0 + 1][r] - Z[c0][r])     (bilinear derivative)
// (reference: autograd through model/SCA_deform_attn.py:290-301 and :365-394).  No dK / dV exists: the feature-map and
// projection-weight gradients follow from dG (bwd_q) and the forward's R by thin GEMMs in the caller.
//
// Key-stationary: a wave owns one 32-key tile (two 16-key matrix tiles), a workgroup 7 tiles + a PRODUCER wave that
// stages the query side -- the rows G[q][.], H[q][.] of two 32-row slabs of one BEV column per step -- through LDS; one
// barrier per step.  S[q][n] comes out with the key on the lane, so P and dS are the B operands of the Z products as they
// stand; the transposed query-side operands (G^T, H^T) come out of the staged rows through ds_read_b64_tr_b16.
// The table: per column the producer copies the 8 columns x (S + 16) rows the workgroup's chunks can touch into a SHARED
// LDS window (three of them in rotation, filled one column ahead in slices), as 16-bit hi and lo parts (Z is differenced
// in d a / d b: with the hi part alone the position gradient carries the table's 2^-9 rounding) and
// in two row-parity copies (4 consecutive rows are one aligned
// ds_read2_b32 for any first row).  A tile whose taps do not fit one chunk for a column takes the per-pair gather for
// that column (any key set is handled; a cell-sorted segment never does).
#include <type_traits>
#include "attn_tap.h"
#include "attn_host.h"

namespace {

constexpr int NKW = 7;                 // key waves per workgroup (A/B on the benchmark shape: 3, 5 and 9 are 27-45 % slower)
constexpr int NCW = 8;                 // table columns of the shared window (a chunk is 4 wide: origins may differ by 4 columns ...
constexpr int NRX = 8;                 // ... and by 8 rows inside one workgroup)
constexpr int SPB = 2;                 // 32-row slabs per step (= per barrier; one per barrier: 27.5 against 24.4 ms)
// NP: images per operand (1; split mode 2: the lo rows of G | H OFF_LO behind the hi rows)
template <int NP> struct LdsKn {
  static constexpr int OFF_G = 0;      // [32 rows][16 slots] 16-bit
  static constexpr int OFF_H = 1024;
  static constexpr int OFF_LO = 2048;
  static constexpr int OFF_G1 = 2048;       // two groups (NP = 1): the same two images of slots 16..31
  static constexpr int SLAB = 2048 * NP * TAP_NG;    // one slab's G | H rows
  static constexpr int BUF = SPB * SLAB;
};
typedef LdsKn<1> LdsK;
template <int PREC> using LdsKp = LdsKn<tap_np<PREC>>;
// (split mode: every operand twice -- the registers of 2 waves per SIMD)
// (two groups: the operands and accumulators of the second group's slots likewise)
constexpr int tap_bwd_k_waves(int prec) { return tap_split(prec) || BEVR_TAP_G2 ? 2 : 4; }
// dwords per (kind, parity, column) of a window: rows 0 .. Sp + NRX + 7, two rows per dword
__host__ __device__ __forceinline__ int win_dwords(int Sp) { return (Sp + NRX + 8) / 2; }

// does tile box `sb` take the matrix path in BEV column j?  Its taps fit one chunk, and the chunk lies inside the
// workgroup's window (origin row a0w, leftmost coordinate bminw)
__device__ __forceinline__ bool tile_fits(const StepBox& sb, float jrx, int a0w, float bminw) {
  const int da = sb.amin - a0w;
  const int dx = (int)floorf(jrx + sb.bmin) - (int)floorf(jrx + bminw);
  return sb.amax >= sb.amin && da >= 0 && da <= NRX && box_fits(sb, jrx) && dx >= 0 && dx <= NCW - CELL_C;
}

// The slow pairs have two dispatches.  MODE_SLOW launches the main grid again: every workgroup tests its tiles against
// every column and leaves if all fit; one that stays keeps the main launch's shape (producer, a barrier per step) through
// all S columns.  MODE_LIST takes them from a device work list: the main launch appends each tile that has an unfit
// column, and a fixed grid of waves runs (listed tile, range of BEV columns) items.  An item belongs to a WAVE, not to a
// workgroup: the tiles of a workgroup are unfit in different columns, so a shared producer would stage the union of
// their columns and every wave would wait at the barriers of columns it skips; a wave that stages the 2 KB of G | H rows
// of its own slab into its own LDS buffer stages exactly what it computes and meets no barrier at all.
constexpr int MODE_FIT = 0, MODE_SLOW = 1, MODE_LIST = 2;
// work list (attn_host.h): unit i = ph * (Np / 32) + tile; [1] is the list launch's claim counter
constexpr int LIST_WAVES = 4;          // waves per workgroup of the list launch (independent of each other)
// The shortest range of BEV columns of an item.  An item reads its 32 tap records, forms their weights and ends with 128
// float atomics, a few microseconds; an unfit column is nslab slabs of per-pair gathers at ~3.3 us each (measured on the
// full-grid launch: a tile unfit in all 200 columns of 7 slabs held its workgroup for 4.7 ms), 23 us at S = 200.  Eight
// columns keep the fixed part of a mostly unfit tile's item under 5 %.
constexpr int LIST_MIN_COLS = 8;
constexpr int LIST_ITEMS_PER_WAVE = 4; // items aimed at per resident wave: their cost varies with the unfit columns

// MODE_FIT: the (tile, column) pairs that take the matrix path; MODE_SLOW / MODE_LIST: the others, by the per-pair gather
// (MODE_SLOW: a workgroup without any leaves at once: every workgroup of a cell-sorted segment).  Separate launches: with
// both bodies in one loop the matrix path reloaded loop invariants from scratch on every slab.
// (ph, wg): the problem-head and the workgroup of NKW tiles of the main launch's grid -- the tile's window origin follows
// from it in every mode; tslot: the tile's place in it (MODE_FIT / MODE_SLOW: the wave); columns [j_first, j_end).
template <int PREC, int MODE>
__device__ __forceinline__ void tap_bwd_k_body(
    const bevr_attn_desc& d, const char* __restrict__ G, const char* __restrict__ H, const char* __restrict__ tap_ws,
    const float* __restrict__ table_t, float* __restrict__ dkey_a, float* __restrict__ dkey_b,
    float* __restrict__ dkey_y, float* __restrict__ dkey_x, char* smem, int ph, int wg, int tslot, int j_first, int j_end,
    int* __restrict__ slow_list TAP_DROP_PARAMS) {
  typedef LdsKp<PREC> L;
  constexpr bool SLOW = MODE != MODE_FIT;
  constexpr bool X3 = tap_split(PREC);
  constexpr int NP = tap_np<PREC>;

  [[maybe_unused]] const int n_ph = d.n_prob * d.heads;
  const int prob = ph / d.heads, hd = ph % d.heads;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int Mp = d.S * d.Sp;
  const int nslab = d.Sp / 32, nstep = (nslab + SPB - 1) / SPB;
  const int n_tiles = d.Np / 32;
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const int HpT = d.Hp + 1;                                   // rows of a column of the plain transposed table
  const float* tbl = table_t + (size_t)hd * d.Wp * HpT;
  const int krow = tap_key_row(d, prob, hd);                  // the record row: the problem; two groups: (problem, head's group)
  const StepBox* box = reinterpret_cast<const StepBox*>(tap_ws + tap_ws_box_offset(d)) + (size_t)krow * (d.Np / 32);
  const int NRWD = win_dwords(d.Sp);
  const int win_bytes = 4 * NCW * NRWD * 4;                   // [kind hi / lo][row parity][NCW columns][NRWD dwords]
  char* win_base = smem + 2 * L::BUF;
  // the key waves' records live in LDS between their uses (column start, column end): 8 registers less in the slab loop
  // (MODE_LIST: no windows; LIST_WAVES pairs of slab buffers, one pair per wave, then the records)
  TapRec* stash = reinterpret_cast<TapRec*>(MODE == MODE_LIST ? smem + LIST_WAVES * 2 * L::SLAB : win_base + 3 * win_bytes) + wave * 32;

  // the workgroup's window origin: the lowest table row / leftmost coordinate of its tiles (rows: for every column)
  int a0w = 0x7fffffff;
  float bminw = 3.0e38f;
  for (int t = 0; t < NKW; ++t) {
    const int tile = wg * NKW + t;
    if (tile < n_tiles) {
      const StepBox b = box[tile];
      if (b.amax >= b.amin) {
        a0w = min(a0w, b.amin);
        bminw = fminf(bminw, b.bmin);
      }
    }
  }
  if (a0w == 0x7fffffff) { a0w = 0; bminw = 0.f; }
  if constexpr (MODE == MODE_SLOW) {
    bool unfit = false;     // the same for every wave of the workgroup: all of them leave, or none
    for (int t = 0; t < NKW; ++t) {
      const int tile = wg * NKW + t;
      if (tile >= n_tiles) break;
      const StepBox b = box[tile];
      if (b.amax < b.amin) continue;
      for (int j = lane; j < d.S; j += 64) unfit = unfit || !tile_fits(b, (float)j * rx, a0w, bminw);
    }
    if (!__any(unfit)) return;
  }

  if (MODE != MODE_LIST && wave == NKW) {
    // ---- producer: the G and H rows of slab (j, i0) -> LDS one step ahead of the key waves, and the table window of the
    // NEXT column in slices, one per slab of the current one.  THREE windows: while the slices of column j + 1 are written
    // the key waves may still be one step behind, in the last slab of column j - 1 ---------------------------------------
    __builtin_amdgcn_s_setprio(3);
    const int n_quad = (NRWD + 1) / 2, n_item = NCW * n_quad;
    // item = (column c, rows 4 m .. 4 m + 4) of the window of BEV column jn: five table values in, hi / lo parts of the row
    // pairs (4 m, + 1), (+ 2, + 3) [parity 0] and (+ 1, + 2), (+ 3, + 4) [parity 1] out.  Load and store are separate
    // steps: the loads of one slice are in flight across a barrier (they sat on the workgroup's critical path when the
    // producer waited for them before every barrier)
    auto item_load = [&](int jn, int it, float (&t)[5]) {
      if (it >= n_item || jn >= d.S) return;
      const int c = it / n_quad, m = it - c * n_quad;
      const int x0w = (int)floorf((float)jn * rx + bminw);
      const int xc = max(0, min(x0w + c + d.x_off, d.Wp - 1));
      // rows past the padded table are never weighted: clamp the run's start (the table's last rows are zero padding)
      const int y = max(0, min(a0w + d.y_off + 4 * m, HpT - 5));
      const float* src = tbl + (size_t)xc * HpT + y;
#pragma unroll
      for (int k = 0; k < 5; ++k) t[k] = src[k];
    };
    auto item_store = [&](int jn, int it, const float (&t)[5]) {
      if (it >= n_item || jn >= d.S) return;
      const int c = it / n_quad, m = it - c * n_quad;
      const uint32_t h01 = TapHalf<PREC>::pack2(t[0], t[1]), h23 = TapHalf<PREC>::pack2(t[2], t[3]);
      const uint32_t h12 = TapHalf<PREC>::pack2(t[1], t[2]), h34 = TapHalf<PREC>::pack2(t[3], t[4]);
      const uint32_t l01 = TapHalf<PREC>::pack2(t[0] - TapHalf<PREC>::lo(h01), t[1] - TapHalf<PREC>::hi(h01));
      const uint32_t l23 = TapHalf<PREC>::pack2(t[2] - TapHalf<PREC>::lo(h23), t[3] - TapHalf<PREC>::hi(h23));
      const uint32_t l12 = TapHalf<PREC>::pack2(t[1] - TapHalf<PREC>::lo(h12), t[2] - TapHalf<PREC>::hi(h12));
      const uint32_t l34 = TapHalf<PREC>::pack2(t[3] - TapHalf<PREC>::lo(h34), t[4] - TapHalf<PREC>::hi(h34));
      uint32_t* w = reinterpret_cast<uint32_t*>(win_base + (jn % 3) * win_bytes) + c * NRWD + 2 * m;
      const bool second = 2 * m + 1 < NRWD;
      w[0] = h01;
      w[NCW * NRWD] = h12;
      w[2 * NCW * NRWD] = l01;
      w[3 * NCW * NRWD] = l12;
      if (second) {
        w[1] = h23;
        w[NCW * NRWD + 1] = h34;
        w[2 * NCW * NRWD + 1] = l23;
        w[3 * NCW * NRWD + 1] = l34;
      }
    };
    // the slice of the next column's window that step (j, s) writes: items [s per_step, (s + 1) per_step), two per lane
    const int per_step = (n_item + nstep - 1) / nstep;
    auto slice_item = [&](int s2, int r) {
      const int k = r * 64 + lane;
      return k < per_step ? s2 * per_step + k : n_item;
    };
    float f0[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, f1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (!SLOW) {
      for (int it = lane; it < n_item; it += 64) {   // column 0's window, whole, before the first step
        float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        item_load(0, it, t);
        item_store(0, it, t);
      }
      item_load(1, slice_item(0, 0), f0);
      item_load(1, slice_item(0, 1), f1);
    }
    const char* Gp = G + ((size_t)ph * Mp) * (TAP_ROW * 2) + lane * 16;
    const char* Hq = H + ((size_t)ph * Mp) * (TAP_ROW * 2) + lane * 16;
    // slab `sl` (0 .. S nslab - 1, column-major) of the packed rows starts sl * 1024 bytes in; a step stages SPB slabs
    auto slab_index = [&](int j2, int st2, int u) { return min(j2 * nslab + min(SPB * st2 + u, nslab - 1), d.S * nslab - 1); };
    int e = 0;
#if BEVR_TAP_G2
    // a slab's rows are 64 bytes: 128 chunks of 16, chunk lane + 64 k = (row (lane >> 2) + 16 k, quarter lane & 3);
    // quarters 0, 1 are the row of the first image (slots 0..15), quarters 2, 3 of the second
    u32x4 gv[2][SPB], hv[2][SPB];
    auto rows_load = [&](int j2, int st2) {
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int u = 0; u < SPB; ++u) {
          gv[k][u] = gload16(Gp + k * 1024 + (size_t)slab_index(j2, st2, u) * 2048);
          hv[k][u] = gload16(Hq + k * 1024 + (size_t)slab_index(j2, st2, u) * 2048);
        }
    };
    const int row_dst = ((lane & 3) >> 1) * L::OFF_G1 + (lane >> 2) * 32 + (lane & 1) * 16;
#else
    u32x4 gv[NP][SPB], hv[NP][SPB];       // the rows in flight, per image
    const size_t g_lo = (size_t)n_ph * Mp * 32;     // the lo planes of G and H
    auto rows_load = [&](int j2, int st2) {
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int u = 0; u < SPB; ++u) {
          gv[pl][u] = gload16(Gp + pl * g_lo + (size_t)slab_index(j2, st2, u) * 1024);
          hv[pl][u] = gload16(Hq + pl * g_lo + (size_t)slab_index(j2, st2, u) * 1024);
        }
    };
#endif
    rows_load(0, 0);
    for (int j = 0; j < d.S; ++j) {
      for (int st = 0; st < nstep; ++st, ++e) {
        char* bb = smem + (e & 1) * L::BUF;
#if BEVR_TAP_G2
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int u = 0; u < SPB; ++u) {
            *reinterpret_cast<u32x4*>(bb + u * L::SLAB + L::OFF_G + row_dst + k * 512) = gv[k][u];
            *reinterpret_cast<u32x4*>(bb + u * L::SLAB + L::OFF_H + row_dst + k * 512) = hv[k][u];
          }
#else
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
          for (int u = 0; u < SPB; ++u) {
            *reinterpret_cast<u32x4*>(bb + u * L::SLAB + pl * L::OFF_LO + L::OFF_G + lane * 16) = gv[pl][u];
            *reinterpret_cast<u32x4*>(bb + u * L::SLAB + pl * L::OFF_LO + L::OFF_H + lane * 16) = hv[pl][u];
          }
#endif
        if constexpr (!SLOW) {
          item_store(j + 1, slice_item(st, 0), f0);
          item_store(j + 1, slice_item(st, 1), f1);
          // a slice beyond the two pipelined items per lane (short columns: few steps share the window): on the spot
          for (int k = 128 + lane; k < per_step; k += 64) {
            float t[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            item_load(j + 1, st * per_step + k, t);
            item_store(j + 1, st * per_step + k, t);
          }
        }
        // the next step's rows and the next window slice: in flight across the barrier
        const int jn = st + 1 < nstep ? j : min(j + 1, d.S - 1), stn = st + 1 < nstep ? st + 1 : 0;
        rows_load(jn, stn);
        if constexpr (!SLOW) {
          const int jf = st + 1 < nstep ? j + 1 : j + 2;
          item_load(jf, slice_item(stn, 0), f0);
          item_load(jf, slice_item(stn, 1), f1);
        }
        __syncthreads();
      }
    }
    __syncthreads();
    return;
  }

  // ---- key waves ---------------------------------------------------------------------------------------------------
  const int tile = wg * NKW + tslot;
  const bool have_tile = tile < n_tiles;            // uniform; a wave without a tile only keeps the barriers
  const TapRec* recs = reinterpret_cast<const TapRec*>(tap_ws) + (size_t)krow * d.Np;
#if BEVR_TAP_G2
  const TapPos1* pos1 = reinterpret_cast<const TapPos1*>(tap_ws + tap_ws_pos1_offset(d)) + (size_t)krow * d.Np;
  TapOp<NP> bk1[2];          // group 1's tap slots (lanes 0..31; lanes 32..63 zero)
  f32x4 zt1[2], zv1[2];      // Z of group 1's slots
#endif
  const int tl = have_tile ? tile : 0;
  const StepBox sb = box[tl];
  const int da = sb.amin - a0w;                       // rows between the window's origin and this tile's chunk origin

  // B operand of S / dP for key sub-tile kb: lanes 0..31 the tap slots, lanes 32..63 the cells (per column)
  TapOp<NP> bk[2];
  // Z[slot 4 g + e][key] of the logit path (G^T dS) and of the value path (H^T P: H carries ln2, undone at the end),
  // Z[cell (c = g, r = e)][key]
  f32x4 zt[2], zv[2], zc[2];
  float acc_a[2] = {0.f, 0.f}, acc_b[2] = {0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const TapRec r0 = recs[(size_t)tl * 32 + 16 * kb + li];
    if (g == 0) stash[16 * kb + li] = r0;
    TapOp<NP> t[2];
    tap_weights<PREC>(r0.ys, r0.xs, t);
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) bk[kb].p[pl] = g == 0 ? t[0].p[pl] : t[1].p[pl];
    zt[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    zv[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    zc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#if BEVR_TAP_G2
    const TapPos1 q1 = pos1[(size_t)tl * 32 + 16 * kb + li];
    tap_weights1<PREC>(r0.ys < -50.0f ? TAP_YS_DEAD : q1.ys, q1.xs, t);
    bk1[kb] = TapOp<NP>{};
    if (g < 2) bk1[kb] = g == 0 ? t[0] : t[1];
    zt1[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    zv1[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#endif
  }
  const int a_row = L::OFF_G + li * 32 + (g & 1) * 16;                          // row read of a staged image (lanes 0..31)
  const int t_off = (4 * g + (li >> 2)) * 32 + (lane & 3) * 8;                  // transposed read, second block + 512
  const int cell_c = li >> 2, cell_r = li & 3;                                   // this lane's cell in the transposed table operands
#if BEVR_DROP
  // dropout: dS = P (keep ? D dP : 0 - delta) and the value path from keep P (D rides in H).  The key is on the lane: its
  // part of the hash is computed once; the query part changes with the row
  // (with the seed and the problem-head folded in: the hash's three parts are combined by xor)
  uint32_t khk[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
    khk[kb] = ((key0 + (uint32_t)(tl * 32 + 16 * kb + li)) * 0xC2B2AE3Du) ^ drop_seed ^ ((uint32_t)ph * 0x9E3779B1u);
  uint32_t hcol = 0u;      // the query part mq * 0x85EBCA77 for row 4 g of the column -- set per column
#endif

  int e = 0;
  float jrx = 0.f;
  // this column's window and this lane's byte offsets into it at slab 0 (a row is 2 bytes, so slab i0 is 2 i0 further; the
  // row parity of a lane's reads does not change from slab to slab): the plain cell reads of the S operand (columns
  // 2 (g - 2) and + 1) and the transposed reads of the Z operands (hi and lo parts)
  const char* win_b = nullptr;
  int wq0 = 0, wq1 = 0, wth = 0, wtl = 0;
  const int win_lo = 2 * NCW * NRWD * 4;      // the window's lo parts behind its hi parts
  // one 32-row slab of column j against this wave's 32 keys.  FIT: the tile's taps fit one chunk inside the window (bias
  // and its position gradient through the matrix cores); else the per-pair gather from the table in global memory
  auto slab = [&](auto fit_tag, const char* base, int i0) {
    constexpr bool FIT = decltype(fit_tag)::value;
    // (rows past the grid carry the offset -big in G: their weights are 0 without a test here)
    TapOp<NP> qa[2], ha[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      qa[rb] = ha[rb] = TapOp<NP>{};
      if (g < 2) {
        qa[rb] = tap_ld<NP>(base + a_row + rb * 512, L::OFF_LO);
        ha[rb] = tap_ld<NP>(base + L::OFF_H - L::OFF_G + a_row + rb * 512, L::OFF_LO);
      } else if (FIT) {
        // the chunk's cells for BEV row i0 + 16 rb + li: columns 2 (g - 2), + 1; rows i .. i + 3 of the window (addresses
        // prepared per column: wq0 / wq1; a slab is 16 dwords further, the second row block 8 more); the lo image is the
        // window's lo parts
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
          const uint32_t* w0 = reinterpret_cast<const uint32_t*>(win_b + pl * win_lo + wq0 + 2 * i0) + 8 * rb;
          const uint32_t* w1 = reinterpret_cast<const uint32_t*>(win_b + pl * win_lo + wq1 + 2 * i0) + 8 * rb;
          qa[rb].p[pl] = __builtin_bit_cast(bf16x8, u32x4{w0[0], w0[1], w1[0], w1[1]});
        }
      }
    }
    const TapOp<NP> gt = tap_ld_tr<NP>(base + L::OFF_G + t_off, 512, L::OFF_LO);
    const TapOp<NP> ht = tap_ld_tr<NP>(base + L::OFF_H + t_off, 512, L::OFF_LO);
#if BEVR_TAP_G2
    TapOp<NP> qa1[2], ha1[2];   // the rows' slots 16..31 (lanes 0..31)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      qa1[rb] = ha1[rb] = TapOp<NP>{};
      if (g < 2) {
        qa1[rb] = tap_ld<NP>(base + L::OFF_G1 + a_row + rb * 512, L::OFF_LO);
        ha1[rb] = tap_ld<NP>(base + L::OFF_G1 + L::OFF_H - L::OFF_G + a_row + rb * 512, L::OFF_LO);
      }
    }
    const TapOp<NP> gt1 = tap_ld_tr<NP>(base + L::OFF_G1 + L::OFF_G + t_off, 512, L::OFF_LO);
    const TapOp<NP> ht1 = tap_ld_tr<NP>(base + L::OFF_G1 + L::OFF_H + t_off, 512, L::OFF_LO);
#endif
    bf16x8 thi = gt.p[0], tlo = gt.p[0];
    if constexpr (FIT) {
      const uint32_t* w0 = reinterpret_cast<const uint32_t*>(win_b + wth + 2 * i0);
      const uint32_t* w1 = reinterpret_cast<const uint32_t*>(win_b + wtl + 2 * i0);
      thi = __builtin_bit_cast(bf16x8, u32x4{w0[0], w0[1], w0[8], w0[9]});
      tlo = __builtin_bit_cast(bf16x8, u32x4{w1[0], w1[1], w1[8], w1[9]});
    }
#if BEVR_DROP
    // the 8 queries of this lane's accumulator rows: i0 + 4 g + r (row block 0) and + 16 (row block 1): the row hash and
    // -delta out of slots TAP_CHI / TAP_CLO of the staged H row
    // (the query part of the other seven rows differs from hq0's by constants: the product is linear modulo 2^32)
    const uint32_t hq0 = hcol + (uint32_t)i0 * 0x85EBCA77u;
    auto hq = [&](int r) { return hq0 + (uint32_t)(16 * (r >> 2) + (r & 3)) * 0x85EBCA77u; };
    float ndel[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t c2 = *reinterpret_cast<const uint32_t*>(base + L::OFF_H + (16 * (r >> 2) + 4 * g + (r & 3)) * 32 + TAP_CHI * 2);
      ndel[r] = TapHalf<PREC>::lo(c2) + TapHalf<PREC>::hi(c2);
      if constexpr (X3)
        ndel[r] = tap_drop_ndel4(c2, *reinterpret_cast<const uint32_t*>(base + L::OFF_LO + L::OFF_H + (16 * (r >> 2) + 4 * g + (r & 3)) * 32 + TAP_CHI * 2));
    }
#endif
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#if BEVR_TAP_G2
      const f32x4 s0 = tap_mm<PREC, true>(qa[0], bk[kb], tap_mm<PREC, true>(qa1[0], bk1[kb], z4));
      const f32x4 s1 = tap_mm<PREC, true>(qa[1], bk[kb], tap_mm<PREC, true>(qa1[1], bk1[kb], z4));
      const f32x4 q0 = tap_mm<PREC>(ha[0], bk[kb], tap_mm<PREC>(ha1[0], bk1[kb], z4));
      const f32x4 q1 = tap_mm<PREC>(ha[1], bk[kb], tap_mm<PREC>(ha1[1], bk1[kb], z4));
#else
      const f32x4 s0 = tap_mm<PREC, true>(qa[0], bk[kb], z4);       // S[query 4 g + e of row block 0][key]
      const f32x4 s1 = tap_mm<PREC, true>(qa[1], bk[kb], z4);
      const f32x4 q0 = tap_mm<PREC>(ha[0], bk[kb], z4);             // dP
      const f32x4 q1 = tap_mm<PREC>(ha[1], bk[kb], z4);
#endif
      float p[8], ds[8];
      if constexpr (!FIT) {
        const TapRec rk = stash[16 * kb + li];
        const float a = rk.a, tx = jrx + rk.b;
        const float af = floorf(a), xf = floorf(tx);
        const float fy = a - af, fx = tx - xf;
        const bool dead = rk.ys < -50.0f;
        const int xc = max(0, min((int)xf + d.x_off, d.Wp - 2));
        const int yb = (int)af + d.y_off + i0 + 4 * g;
        float pa = 0.f, pb = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int y = max(0, min(yb + (r & 3) + 16 * (r >> 2), HpT - 2));
          const float* c0p = tbl + (size_t)xc * HpT + y;
          const float t00 = c0p[0], t01 = c0p[1], t10 = c0p[HpT], t11 = c0p[HpT + 1];
          const float u0 = t00 + fy * (t01 - t00), u1 = t10 + fy * (t11 - t10);
          const float sv = (r < 4 ? s0[r & 3] : s1[r & 3]) + (dead ? 0.f : u0 + fx * (u1 - u0));
          p[r] = fast_exp2(sv);
#if BEVR_DROP
          {
            const bool keep = tap_drop_keep(hq(r), khk[kb], drop_thr);
            ds[r] = p[r] * (keep ? (r < 4 ? q0[r & 3] : q1[r & 3]) : ndel[r]);
            p[r] = keep ? p[r] : 0.f;
          }
#else
          ds[r] = p[r] * (r < 4 ? q0[r & 3] : q1[r & 3]);
#endif
          pa += ds[r] * ((1.0f - fx) * (t01 - t00) + fx * (t11 - t10));
          pb += ds[r] * (u1 - u0);
        }
        acc_a[kb] += dead ? 0.f : pa;
        acc_b[kb] += dead ? 0.f : pb;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#if BEVR_DROP
          p[r] = fast_exp2(s0[r]);
          p[4 + r] = fast_exp2(s1[r]);
          const bool keep0 = tap_drop_keep(hq(r), khk[kb], drop_thr), keep1 = tap_drop_keep(hq(4 + r), khk[kb], drop_thr);
          ds[r] = p[r] * (keep0 ? q0[r] : ndel[r]);
          ds[4 + r] = p[4 + r] * (keep1 ? q1[r] : ndel[4 + r]);
          p[r] = keep0 ? p[r] : 0.f;
          p[4 + r] = keep1 ? p[4 + r] : 0.f;
#else
          p[r] = fast_exp2(s0[r]);
          ds[r] = p[r] * q0[r];
          p[4 + r] = fast_exp2(s1[r]);
          ds[4 + r] = p[4 + r] * q1[r];
#endif
        }
      }
      u32x4 dsw[NP], pw[NP];      // (pair by pair: packed one after the other the two cost the gather launch scratch)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        tap_pack2<PREC>(ds[2 * k], ds[2 * k + 1], k, dsw);
        tap_pack2<PREC>(p[2 * k], p[2 * k + 1], k, pw);
      }
      const TapOp<NP> ds8 = tap_op(dsw), p8 = tap_op(pw);
      zt[kb] = tap_mm<PREC>(gt, ds8, zt[kb]);
      zv[kb] = tap_mm<PREC>(ht, p8, zv[kb]);
#if BEVR_TAP_G2
      zt1[kb] = tap_mm<PREC>(gt1, ds8, zt1[kb]);
      zv1[kb] = tap_mm<PREC>(ht1, p8, zv1[kb]);
#endif
      if constexpr (FIT) {
        // the window's hi + lo parts against dS, small terms first (split mode: the lo image of dS against the hi part too)
        zc[kb] = mfma16<PREC>(tlo, ds8.p[0], zc[kb]);
        if constexpr (X3) zc[kb] = mfma16<PREC>(thi, ds8.p[1], zc[kb]);
        zc[kb] = mfma16<PREC>(thi, ds8.p[0], zc[kb]);
      }
    }
  };

  bool any_unfit = false;     // the tile has an unfit column in the range: left to the slow pass / computed here (uniform)
  for (int j = j_first; j < j_end; ++j) {
    jrx = (float)j * rx;
#if BEVR_DROP
    hcol = (uint32_t)(j * d.Sp + 4 * g) * 0x85EBCA77u;
#endif
    const int x0 = (int)floorf(jrx + sb.bmin), a0 = sb.amin;
    const int dx = x0 - (int)floorf(jrx + bminw);
    const bool fit = tile_fits(sb, jrx, a0w, bminw);    // uniform over the wave
    const bool mine = have_tile && sb.amax >= sb.amin && fit != SLOW;   // this launch's share of the (tile, column) pairs
    if constexpr (MODE == MODE_FIT) any_unfit = any_unfit || (have_tile && sb.amax >= sb.amin && !fit);
    if constexpr (MODE == MODE_LIST) {
      // a column that fits costs this one test; an unfit one: its slabs' G | H rows through the wave's own pair of
      // buffers, the next slab's rows in flight under this one's gathers.  LDS accesses of one wave complete in order:
      // the fences only keep the compiler from moving the reads of a buffer over the stores that fill it
      if (!mine) continue;
      any_unfit = true;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        if (g >= 2) bk[kb] = TapOp<NP>{};
      char* wbuf = smem + wave * 2 * L::SLAB;
      const char* Gs = G + ((size_t)ph * Mp + (size_t)j * d.Sp) * 32 + lane * 16;
      const char* Hs = H + ((size_t)ph * Mp + (size_t)j * d.Sp) * 32 + lane * 16;
      u32x4 gv = gload16(Gs), hv = gload16(Hs);
      for (int s = 0; s < nslab; ++s) {
        char* bb = wbuf + (s & 1) * L::SLAB;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        *reinterpret_cast<u32x4*>(bb + L::OFF_G + lane * 16) = gv;
        *reinterpret_cast<u32x4*>(bb + L::OFF_H + lane * 16) = hv;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (s + 1 < nslab) {
          gv = gload16(Gs + (size_t)(s + 1) * 1024);
          hv = gload16(Hs + (size_t)(s + 1) * 1024);
        }
        slab(std::false_type{}, bb, 32 * s);
      }
      continue;
    }
    // this key's coordinates inside the chunk for this column
    auto chunk_coords = [&](int kb, float& tcol, float& trow) {
      const TapRec rk = stash[16 * kb + li];
      const float tx = jrx + rk.b;
      const float xf = floorf(tx);
      tcol = rk.ys < -50.0f ? -8.0f : (xf - (float)x0) + (tx - xf);
      trow = rk.a - (float)a0;
    };
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      if (g >= 2) {
        bk[kb] = TapOp<NP>{};
        if (!SLOW && mine) {
          float tcol, trow;
          chunk_coords(kb, tcol, trow);
          bk[kb] = tap_cell_half<PREC>(tcol, trow, g - 2);
        }
      }
      zc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    win_b = win_base + (j % 3) * win_bytes;
    {
      const int iq = li + da, pq = iq & 1;                       // plain reads: window row of BEV row li (row block 0)
      wq0 = ((pq * NCW + dx + 2 * max(g - 2, 0)) * NRWD + ((iq - pq) >> 1)) * 4;
      wq1 = wq0 + NRWD * 4;
      const int it = 4 * g + cell_r + da, pt = it & 1;           // transposed reads: rows 4 g + cell_r .. + 3 and + 16 ..
      wth = ((pt * NCW + dx + cell_c) * NRWD + ((it - pt) >> 1)) * 4;
      wtl = wth + win_lo;
    }
    for (int st = 0; st < nstep; ++st, ++e) {
      __syncthreads();
      if (!mine) continue;
#pragma unroll
      for (int u = 0; u < SPB; ++u)
        if (SPB * st + u < nslab) slab(std::integral_constant<bool, !SLOW>{}, smem + (e & 1) * L::BUF + u * L::SLAB, 32 * (SPB * st + u));
    }
    // ---- the column's bias-position gradients out of Z: this lane holds chunk column c = g, rows 0..3 of its key ----
    if (!SLOW && mine) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        float tc, tr;
        chunk_coords(kb, tc, tr);
        const float c0 = floorf(tc), r0 = floorf(tr);
        const float wxg = hat((float)g - tc);
        const float z0 = zc[kb][0], z1 = zc[kb][1], z2 = zc[kb][2], z3 = zc[kb][3];
        // rows r0, r0 + 1 (r0 in 0..2 for a key inside the chunk)
        const float zl = r0 < 0.5f ? z0 : (r0 < 1.5f ? z1 : z2);
        const float zh = r0 < 0.5f ? z1 : (r0 < 1.5f ? z2 : z3);
        const float zrow = hat(0.f - tr) * z0 + hat(1.f - tr) * z1 + hat(2.f - tr) * z2 + hat(3.f - tr) * z3;
        const float sg = ((float)g == c0 + 1.0f ? 1.0f : 0.f) - ((float)g == c0 ? 1.0f : 0.f);
        acc_a[kb] += wxg * (zh - zl);      // summed over the four lane groups at the end (the sum is linear)
        acc_b[kb] += sg * zrow;
      }
    }
  }
  if constexpr (MODE != MODE_LIST) __syncthreads();   // the producer's closing barrier

  if (!have_tile) return;
  if (MODE == MODE_LIST && !any_unfit) return;   // every column of the range fits: nothing to add
  if constexpr (MODE == MODE_FIT) {
    // the work list of the list launch (null: the full-grid slow launch finds its tiles itself)
    if (slow_list && any_unfit && lane == 0) slow_list[LIST_HEAD + atomicAdd(slow_list, 1)] = ph * n_tiles + tile;
  }
  // ---- per key: tap-weight gradients -> sampling-position gradient; everything summed over the four lane groups ----
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    const TapRec rk = stash[16 * kb + li];
    const float ys = rk.ys, xs = rk.xs;
    const float y0 = floorf(ys), x0f = floorf(xs);
    float gy = 0.f, gx = 0.f;
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const int t = 4 * g + e2;                       // slot; taps are t < 12: (r, c) = (t / 3, t % 3)
      const float r = (float)(t / 3), c = (float)(t % 3);
      const float dwy = (r == y0 + 1.0f ? 1.0f : 0.f) - (r == y0 ? 1.0f : 0.f);
      const float dwx = (c == x0f + 1.0f ? 1.0f : 0.f) - (c == x0f ? 1.0f : 0.f);
      const float z = g < 3 ? zt[kb][e2] + BEVR_LOG2E * zv[kb][e2] : 0.f;
      gy += z * dwy * hat(c - xs);
      gx += z * hat(r - ys) * dwx;
    }
    float va = acc_a[kb], vb = acc_b[kb];
    gy += __shfl_xor(gy, 16); gx += __shfl_xor(gx, 16); va += __shfl_xor(va, 16); vb += __shfl_xor(vb, 16);
    gy += __shfl_xor(gy, 32); gx += __shfl_xor(gx, 32); va += __shfl_xor(va, 32); vb += __shfl_xor(vb, 32);
    const int n = tile * 32 + 16 * kb + li;
#if BEVR_TAP_G2
    // group 1's sampling position through its own slots; dkey_y, dkey_x [row][2][Np]
    const TapPos1 q1 = pos1[(size_t)tl * 32 + 16 * kb + li];
    const float y1 = floorf(q1.ys), x1f = floorf(q1.xs);
    float gy1 = 0.f, gx1 = 0.f;
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const int t = 4 * g + e2;
      const float r = (float)(t / 3), c = (float)(t % 3);
      const float dwy = (r == y1 + 1.0f ? 1.0f : 0.f) - (r == y1 ? 1.0f : 0.f);
      const float dwx = (c == x1f + 1.0f ? 1.0f : 0.f) - (c == x1f ? 1.0f : 0.f);
      const float z = g < 3 ? zt1[kb][e2] + BEVR_LOG2E * zv1[kb][e2] : 0.f;
      gy1 += z * dwy * hat(c - q1.xs);
      gx1 += z * hat(r - q1.ys) * dwx;
    }
    gy1 += __shfl_xor(gy1, 16); gx1 += __shfl_xor(gx1, 16);
    gy1 += __shfl_xor(gy1, 32); gx1 += __shfl_xor(gx1, 32);
    if (g == 0 && n < d.N) {
      const size_t idx = (size_t)krow * d.Np + n;
      atomicAdd(dkey_a + idx, va);
      atomicAdd(dkey_b + idx, vb);
      atomicAdd(dkey_y + idx + (size_t)krow * d.Np, gy);
      atomicAdd(dkey_x + idx + (size_t)krow * d.Np, gx);
      atomicAdd(dkey_y + idx + (size_t)(krow + 1) * d.Np, gy1);
      atomicAdd(dkey_x + idx + (size_t)(krow + 1) * d.Np, gx1);
    }
#else
    if (g == 0 && n < d.N) {
      const size_t idx = (size_t)prob * d.Np + n;
      atomicAdd(dkey_a + idx, va);
      atomicAdd(dkey_b + idx, vb);
      atomicAdd(dkey_y + idx, gy);
      atomicAdd(dkey_x + idx, gx);
    }
#endif
  }
}

// the main grid: one workgroup per NKW tiles of a problem-head
template <int PREC, bool SLOW>
__global__ __launch_bounds__(64 * (NKW + 1), tap_bwd_k_waves(PREC)) void attn_tap_bwd_k_kernel(
    bevr_attn_desc d, const char* __restrict__ G, const char* __restrict__ H, const char* __restrict__ tap_ws,
    const float* __restrict__ table_t, float* __restrict__ dkey_a, float* __restrict__ dkey_b,
    float* __restrict__ dkey_y, float* __restrict__ dkey_x, int n_wg_ph, int* __restrict__ slow_list TAP_DROP_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int ph = (slot / n_wg_ph) * 8 + xcd;
  if (ph >= d.n_prob * d.heads) return;
  tap_bwd_k_body<PREC, SLOW ? MODE_SLOW : MODE_FIT>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, smem, ph,
                                                    slot % n_wg_ph, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), 0,
                                                    d.S, slow_list TAP_DROP_ARGS);
}

#if !BEVR_DROP && !BEVR_TAP_X3 && !BEVR_TAP_G2
// The list launch: every wave claims (listed tile, range of BEV columns) items from the counter list[1] until they run
// out -- the items' cost varies with the number of unfit columns, so they are claimed, not dealt.  The list is complete
// (the main launch precedes this one on the stream); a claim never waits, and every wave reaches the exit.  An empty
// list costs a wave the one read of the count.
// Three waves per SIMD: 163 registers without scratch; at the main grid's four the staging registers spill (152 bytes a lane).
template <int PREC>
__global__ __launch_bounds__(64 * LIST_WAVES, 3) void attn_tap_bwd_k_list_kernel(
    bevr_attn_desc d, const char* __restrict__ G, const char* __restrict__ H, const char* __restrict__ tap_ws,
    const float* __restrict__ table_t, float* __restrict__ dkey_a, float* __restrict__ dkey_b,
    float* __restrict__ dkey_y, float* __restrict__ dkey_x, int* __restrict__ list) {
  static_assert(tap_np<PREC> == 1, "the waves stage one image per operand");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n_list = __builtin_amdgcn_readfirstlane(list[0]);
  if (n_list <= 0) return;
  const int n_tiles = d.Np / 32;
  // ranges per tile from the list length: LIST_ITEMS_PER_WAVE items per wave of the grid, none shorter than LIST_MIN_COLS
  const int want = (LIST_ITEMS_PER_WAVE * LIST_WAVES * (int)gridDim.x + n_list - 1) / n_list;
  const int n_rng0 = max(1, min(want, d.S / LIST_MIN_COLS));
  const int cols = (d.S + n_rng0 - 1) / n_rng0;
  const int n_rng = (d.S + cols - 1) / cols;          // no empty range
  const int n_item = n_list * n_rng;
  for (;;) {
    int item = 0;
    if ((threadIdx.x & 63) == 0) item = atomicAdd(list + 1, 1);
    item = __builtin_amdgcn_readfirstlane(item);
    if (item >= n_item) return;
    const int unit = list[LIST_HEAD + item % n_list], rng = item / n_list;
    const int tile = unit % n_tiles;
    tap_bwd_k_body<PREC, MODE_LIST>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, smem, unit / n_tiles,
                                    tile / NKW, tile % NKW, rng * cols, min(d.S, (rng + 1) * cols), nullptr);
  }
}
#endif

// slow_list: null -- the slow pairs by the main grid launched again; else the work list (cleared here, filled by the
// main launch) and the list launch of at most max_wg workgroups (0: what the device holds)
template <int PREC>
int launch(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws, const float* table_t, float* dkey_a,
           float* dkey_b, float* dkey_y, float* dkey_x, int* slow_list, int max_wg, hipStream_t st TAP_DROP_PARAMS) {
  typedef LdsKp<PREC> L;
  const int n_ph = d.n_prob * d.heads;
  const int n_tiles = d.Np / 32;
  const int n_wg_ph = (n_tiles + NKW - 1) / NKW;
  const size_t lds = 2 * L::BUF + (size_t)3 * 4 * NCW * win_dwords(d.Sp) * 4 + NKW * 32 * sizeof(TapRec);
  if (lds > 160 * 1024) return BEVR_E_SHAPE;
  const long long grid = (long long)((n_ph + 7) / 8) * 8 * n_wg_ph;
  if (grid > 0x7fffffffLL) return BEVR_E_SHAPE;
  int rc;
  if (slow_list) {
    // the list kernel counts items (listed tile, range) in an int
    if ((long long)n_ph * n_tiles * (d.S / LIST_MIN_COLS + 1) > 0x7fffffffLL) return BEVR_E_SHAPE;
    rc = bevr_list_clear(slow_list, st);
    if (rc) return rc;
  }
  // the operands the kernels share; each adds its own tail
#define BEVR_TAP_BWD_K_ARGS \
  d, (const char*)G, (const char*)H, (const char*)tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x
#define BEVR_TAP_LAUNCH(SLOW_, LIST_)                                                                                  \
  hipLaunchKernelGGL((attn_tap_bwd_k_kernel<PREC, SLOW_>), dim3((unsigned)grid), dim3(64 * (NKW + 1)), lds, st,       \
                     BEVR_TAP_BWD_K_ARGS, n_wg_ph, LIST_ TAP_DROP_ARGS)
  BEVR_TAP_LAUNCH(false, slow_list);
  rc = (int)hipGetLastError();
  if (rc) return rc;
#if !BEVR_DROP && !BEVR_TAP_X3 && !BEVR_TAP_G2
  if (slow_list) {
    const size_t lds_list = LIST_WAVES * (2 * L::SLAB + 32 * sizeof(TapRec));
    const int n_wg = bevr_list_workgroups<&attn_tap_bwd_k_list_kernel<PREC>>(max_wg, 64 * LIST_WAVES, lds_list);
    if (n_wg <= 0) return (int)hipErrorInvalidDevice;
    hipLaunchKernelGGL((attn_tap_bwd_k_list_kernel<PREC>), dim3(n_wg), dim3(64 * LIST_WAVES), lds_list, st,
                       BEVR_TAP_BWD_K_ARGS, slow_list);
    return (int)hipGetLastError();
  }
#endif
  BEVR_TAP_LAUNCH(true, (int*)nullptr);
#undef BEVR_TAP_LAUNCH
#undef BEVR_TAP_BWD_K_ARGS
  return (int)hipGetLastError();
}

// The contract of every tap bwd_k entry point.  PRECS: the modes this translation unit holds the kernels of.
// slow_list: null for the full-grid slow launch (and always in the split mode, which has no list kernel)
template <int... PRECS>
int run(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws, const float* table_t, float* dkey_a,
        float* dkey_b, float* dkey_y, float* dkey_x, int* slow_list, int max_wg, void* stream TAP_DROP_PARAMS) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!G || !H || !tap_ws || !table_t || !dkey_a || !dkey_b || !dkey_y || !dkey_x) return BEVR_E_NULL;
  if (d->groups != TAP_NG || (BEVR_TAP_G2 && (d->heads & 1))) return BEVR_E_SHAPE;
  if (!bevr_aligned16(G) || !bevr_aligned16(H) || !bevr_aligned16(tap_ws)) return BEVR_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
#if !BEVR_DROP && !BEVR_TAP_X3 && !BEVR_TAP_G2
  // the split mode's kernels are attn_tap_bwd_k_x3.hip's
  if (d->precision == BEVR_PREC_BF16X3 && !slow_list)
    return bevr_tap_bwd_k_x3(*d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, st);
#endif
  return bevr_for_precision<PRECS...>(d->precision, [&](auto P) {
    return launch<P()>(*d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, slow_list, max_wg, st TAP_DROP_ARGS);
  });
}

}  // namespace

#if BEVR_TAP_G2
// two channel groups: this translation unit is attn_tap_bwd_k_g2.hip, an entry point of its own (16-bit modes, no keep
// mask; the slow pairs by the main grid launched again: no work list)
extern "C" int bevr_attn_tap_g2_bwd_k(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                      const float* table_t, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                                      void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, nullptr, 0, stream);
}
#elif BEVR_TAP_X3 && !BEVR_DROP
// the split-mode instantiations: this translation unit is attn_tap_bwd_k_x3.hip, entered from bevr_attn_tap_bwd_k
int bevr_tap_bwd_k_x3(const bevr_attn_desc& d, const void* G, const void* H, const void* tap_ws, const float* table_t,
                      float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x, hipStream_t st) {
  return launch<BEVR_PREC_BF16X3>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, nullptr, 0, st);
}
#elif BEVR_TAP_X3
// the split-mode instantiations with the keep mask: this translation unit is attn_tap_bwd_k_x3_drop.hip, an entry point
// of its own (the slow pairs by the main grid launched again: no work list)
extern "C" int bevr_attn_tap_bwd_k_x3_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                              const float* table_t, float* dkey_a, float* dkey_b, float* dkey_y,
                                              float* dkey_x, unsigned key0, unsigned drop_thr, unsigned drop_seed,
                                              void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16X3>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, nullptr, 0, stream TAP_DROP_ARGS);
}
#elif BEVR_DROP
extern "C" int bevr_attn_tap_bwd_k_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                           const float* table_t, float* dkey_a, float* dkey_b, float* dkey_y,
                                           float* dkey_x, unsigned key0, unsigned drop_thr, unsigned drop_seed,
                                           void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, nullptr, 0, stream
                                            TAP_DROP_ARGS);
}
#else
extern "C" int bevr_attn_tap_bwd_k(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                   const float* table_t, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                                   void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, nullptr, 0, stream);
}

extern "C" size_t bevr_attn_tap_bwd_k_ws_bytes(const bevr_attn_desc* d) {
  if (bevr_check_desc(d)) return 0;
  return bevr_list_bytes((size_t)d->n_prob * d->heads * (d->Np / 32));
}

extern "C" int bevr_attn_tap_bwd_k_ws(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                      const float* table_t, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                                      void* ws, int max_workgroups, void* stream) {
  if (!ws) return BEVR_E_NULL;
  if (!bevr_aligned16(ws)) return BEVR_E_ALIGN;
  if (max_workgroups < 0) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, G, H, tap_ws, table_t, dkey_a, dkey_b, dkey_y, dkey_x, (int*)ws,
                                            max_workgroups, stream);
}
#endif
