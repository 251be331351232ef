// Slab query-side backward in BEVR_PREC_BF16X3 (split-bf16 products at f32 tolerance), S <= 211: bevr_attn_slab_bwd_q_x3.
//
// attn_slab.h compiled with BEVR_SLAB_X3 = 1 gives the constants, the workspace, the preparation kernels, the scaffold of
// the kernel, the launch and the entry points; the kernel body below is this file's own -- a separate translation unit so
// that the 16-bit kernels stay what they are.  The scheme is the 16-bit kernel's (persistent workgroups, work items from an
// atomic counter, a producer wave one emission ahead, one worker wave per 31-row block, keys sorted by table column); what
// differs:
//
//   * operands.  Q, dO and the sorted K / V rows are the mode's 128-byte split rows (bevr_common.h: per 16-element half
//     hi(e0..7) | hi(e8..15) | lo(e0..7) | lo(e8..15)); S^T = K Q, dP^T = V dO and dQ += dS K are three-term split products,
//     small terms first (mma_frag / mma_split); dS is split in registers (split8, as mma_acc_b does);
//   * bias and table gradient stay per pair in f32, the region kernel's f32 layout (attn_bwd_q.hip, the !is16 branches):
//     a slab cell is the f32 pair (T[y], T[y+1]) -- 8 bytes -- and the 64-bit fixed-point gradient cell; the producer
//     writes four f32 tap weights per (column, key) and the workers take them by DPP broadcast; the kill column holds
//     BEVR_NEG_BIG; gscale (a power of two) is folded into both planes of dO and into delta;
//   * slab width.  16 bytes per cell and 2 x 18 464 bytes of staging: slab_width yields sw = 15 owned columns at the
//     448-row pitch (17 columns x 448 x 16 + 36 928 + 64 = 158 848 bytes of LDS), against 24 in the 16-bit modes.
//
// Staged K / V rows: 128 bytes, NO padding, the row's eight 16-byte chunks XOR-swizzled by the row number:
//     chunk c of staged row r sits at chunk position c ^ f(r),   f(r) = rotl3((r >> 1) & 7)   (3-bit rotate left).
// Bank check (MI355X_MICROARCH.md, LDS: ds_read_b128 is served in four groups of 16 lanes {0-3,12-15,20-27} ... with bank
// (a / 4) mod 64, ds_read_b64_tr_b16 in two groups of 32 lanes with bank (a / 4) mod 64, ds_write_b128 in eight groups of 8
// contiguous lanes with bank (a / 4) mod 32):
//   - fragment reads (lane = key row r, one chunk c per instruction): the dword address mod 64 is 32 (r & 1) + 4 (c ^ f(r)).
//     The 16 rows of a lane group are 8 even and 8 odd rows, and among the rows of one parity (r >> 1) & 7 takes 8
//     different values ({0,2,12,14,20,22,24,26} -> 0,1,6,7,2,3,4,5, likewise the others), f is a bijection of it: 16 lanes x
//     4 dwords cover the 64 banks once;
//   - transposed reads of the dQ product (a 16-lane block reads 4 consecutive key rows r0 .. r0 + 3, r0 a multiple of 4,
//     x 32 bytes = chunks {2 P, 2 P + 1} of a 16-channel half, plane P; the two blocks of a lane group are the two halves:
//     chunks C = {2 P, 2 P + 1, 4 + 2 P, 5 + 2 P} of every row): f(r0) = f(r0 + 1) = F and f(r0 + 2) = f(r0 + 3) = F ^ 2
//     (bit 0 of (r >> 1) is bit 1 of f), so the rows read positions C ^ F, C ^ F, C ^ F ^ 2, C ^ F ^ 2 at bank offsets 0, 32, 0,
//     32: C ^ 2 is the other plane's chunk set, disjoint from C -- 32 lanes x 2 dwords cover the 64 banks once;
//   - the producer's stores: 8 contiguous lanes write the 8 chunks of ONE row, a permutation of its 128 bytes: 32 banks once.
// BEVR_DROP = 1 and BEVR_SLAB_ROWS = 1 (the stub units attn_slab_bwd_q_x3_drop.hip, attn_slab_bwd_q_x3_rows.hip): attn_slab.h.
//
// No padding of a uniform row stride can do the same: a stride of 4 m dwords needs m odd for the fragment reads and the
// eight 8-dword blocks of a transposed read tile the banks only if every row starts on a multiple of 8 dwords.
#define BEVR_SLAB_X3 1
#include "attn_slab.h"

// phase clocks: the slots of attn_slab_bwd_q.hip, under a tag of this body's own
BEVR_PROF_DEFINE(slab_x3, 48)

namespace {

// chunk swizzle of staged row r (see above); rows 32 apart share it
__device__ __forceinline__ int slab_x3_swz(int r) {
  const int g = (r >> 1) & 7;
  return ((g << 1) | (g >> 2)) & 7;
}

SLAB_KERNEL_SIGNATURE {
  static_assert(PREC == BEVR_PREC_BF16X3, "the split-bf16 body");
  typedef SlabLds L;
  extern __shared__ __attribute__((aligned(256))) char lds[];
#if !BEVR_SLAB_ROWS
  constexpr int RP = SLAB_RP;
#endif
  constexpr int ROWB = 128;                          // bytes of an operand row, in memory and staged
  static_assert(SKROW == ROWB && sizeof(SlabCK) == 32, "staging layout");
  const SlabMem<f32x2> m = slab_carve<f32x2, RP>(lds, sw);

  const int tid = threadIdx.x;
  // uniform for the compiler too: the producer / worker branch is a scalar branch, not two masked passes of every wave
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave == SNWORK;
  const int rb = wave;                               // worker: row block (BEVR_SLAB_ROWS: of the launch's band)
#if BEVR_SLAB_ROWS
  const int n_rb = n_rb_band;
#else
  const int n_rb = slab_n_rb(d.S);
#endif
  const int Mp = d.S * d.Sp;
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const int n_items = cnt[0];
  const int hpg = d.heads / d.groups;

  // dS = ln2 P (dP - delta); the fixed-point scale of the cells (a power of two: exact) rides in dO and delta
  const float gscale = grad_scale[0], ginv = grad_scale[1] * BEVR_LN2;
#if BEVR_DROP
  // D: a kept pair's dP is D dP (uniform: kept in a scalar register)
  const float ksc = __builtin_bit_cast(
      float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, 65536.0f / (65536.0f - (float)drop_thr))));
#endif
  PROF_ACC(16);

  for (;;) {
    // ---- next work item -------------------------------------------------------------------------------------------
    const int i = slab_claim(tid, m, cnt);
    if (i >= n_items) break;                          // uniform: every wave leaves here
    const SlabItem it = slab_item(items, i, d, hpg, sw, table_pair, dtable);
    PROF_T_DRAIN(ti0);

    // ---- the slab: values in as they are, cells cleared; the kill column: a finite -big ----------------------------
    slab_fill<RP>(tid, m, d, it, sw, R, [](f32x2 v) { return v; }, f32x2{BEVR_NEG_BIG, BEVR_NEG_BIG});
    SLAB_BARRIER();
    PROF_T_DRAIN(ti1);
    PROF_ADD(12, ti1 - ti0);     // slab in
    PROF_ADD(15, 1);             // items

    if (producer) {
      // =========================================== PRODUCER ========================================================
      __builtin_amdgcn_s_setprio(3);
      // the lane number, opaque per item: what the producer derives from it (chunk ids, swizzled store offsets) is made
      // here and not hoisted to the kernel's entry, where it would occupy the workers' registers too -- and vice versa
      int lane = tid & 63;
      asm volatile("" : "+v"(lane));
      const SlabKey* kp = skeys + (size_t)it.pg * d.N;
      const char* Kh = Ks + (size_t)it.ph * d.N * ROWB;
      const char* Vh = Vs + (size_t)it.ph * d.N * ROWB;
      SlabRuns runs;
      runs.start(lane, kbeg, kend, d, it, n_slab);
      u32x4 kv[16];             // 64 keys x 8 chunks of K, then of V: chunk id lane + 64 q <-> key id / 8, chunk id % 8
      SlabKey sk = {0, 0.f, 0.f, 0};
      // (initialised: an array first written under a condition is, for the compiler, the previous ITEM's, and 64 registers
      // stayed live through the workers' path)
#pragma unroll
      for (int q = 0; q < 16; ++q) kv[q] = u32x4{0u, 0u, 0u, 0u};
      bool have = false;
      auto issue = [&]() {      // loads of the emission at the iterator; then step the iterator
        have = runs.more();
        if (!have) return;
        runs.take();
        const int kmax = d.N - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cid = lane + 64 * q;
          const int key = min(runs.k0 + (cid >> 3), kmax);
          kv[q] = *reinterpret_cast<const u32x4*>(Kh + (size_t)key * ROWB + (cid & 7) * 16);
          kv[8 + q] = *reinterpret_cast<const u32x4*>(Vh + (size_t)key * ROWB + (cid & 7) * 16);
        }
        sk = kp[min(runs.k0 + lane, kmax)];
        runs.step();
      };
      issue();
      int e = 0;
      while (have) {
        char* bb = m.stage + (e & 1) * L::BUF;
        const SlabRuns::Emission em = runs.emission();
        const int j = it.j0 + em.c;
        const float jrx = (float)j * rx;
        PROF_T_DRAIN(tp0);
        const SlabKey sk_e = sk;
        // ---- K and V rows, chunks swizzled: straight out of the load registers (a copy of 16 x 4 registers, as the 16-bit
        // kernel's 8 x 4, would be a quarter of the register file) ----
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cid = lane + 64 * q, row = cid >> 3;
          const int o = row * ROWB + (((cid & 7) ^ slab_x3_swz(row)) * 16);
          *reinterpret_cast<u32x4*>(bb + o) = kv[q];
          *reinterpret_cast<u32x4*>(bb + L::OFF_V + o) = kv[8 + q];
        }
        PROF_T_DRAIN(tp1);
        PROF_ADD(0, tp1 - tp0);      // producer: wait for this emission's loads, rows stored
        issue();              // the next emission's loads fly while this one's constants are written and it is processed
        // ---- constants of (column j, key) ----
        {
          const float tx = jrx + sk_e.b;
          const float xf = floorf(tx);
          const int X = (int)xf;
          const bool live = (em.k0 + lane < em.kend) && X >= it.x0 && X < it.x0 + sw;
          // The column fraction without the rounding of jrx + b (|tx| reaches ~1000 table columns: half an ulp is 3e-5 of a
          // column, as much again as the error jrx itself carries): the integer comes off the LARGER term first -- exact,
          // both are on that term's grid and the difference is no larger -- and the sum of two terms of nearly equal size
          // and opposite sign is exact too.  X stays the floor of the rounded sum, the same in every slab (each pair has
          // ONE slab), so fx may leave [0, 1) by that 3e-5: the same bilinear form, extended by a hair.
          const bool b_big = fabsf(sk_e.b) >= fabsf(jrx);
          const float fx = ((b_big ? sk_e.b : jrx) - xf) + (b_big ? jrx : sk_e.b), fy = sk_e.fy;
          SlabCK ck;
          if (live) {
            ck.w00 = (1.0f - fx) * (1.0f - fy);
            ck.w01 = (1.0f - fx) * fy;
            ck.w10 = fx * (1.0f - fy);
            ck.w11 = fx * fy;
            ck.row = sk_e.A + SLAB_ROW0;
            ck.cell = ((X - it.x0 + 1) * RP + ck.row) * 8;    // BYTE offset of the first tap's value entry
          } else {          // masked: first tap in the kill column => P = 0, dS = 0
            ck.w00 = 1.f;
            ck.w01 = ck.w10 = ck.w11 = 0.f;
            ck.row = 0;
            ck.cell = 0;
          }
          ck.pad0 = ck.pad1 = 0;
          *reinterpret_cast<SlabCK*>(bb + L::OFF_CK + lane * (int)sizeof(SlabCK)) = ck;
#if BEVR_DROP
          // the keys arrive sorted by b: the mask is of the ORIGINAL index (SlabKey::pad, this unit's prep)
          *reinterpret_cast<unsigned*>(bb + L::OFF_KN + lane * 4) = (unsigned)sk_e.pad * 0xC2B2AE3Du;
#endif
          slab_post(bb, lane, live, live && slab_far(d, sk_e.A), em, j);
        }
        ++e;
        PROF_T_DRAIN(tp2);
        PROF_ADD(1, tp2 - tp1);      // producer: next loads issued, constants
        SLAB_BARRIER();
        PROF_T_DRAIN(tp3);
        PROF_ADD(2, tp3 - tp2);      // producer: waiting for the workers
        PROF_ADD(3, 1);
      }
      slab_post_done(m.stage + (e & 1) * L::BUF, lane);
      SLAB_BARRIER();
      __builtin_amdgcn_s_setprio(0);
    } else {
      // =========================================== WORKERS =========================================================
      const bool active = rb < n_rb;
      int lane = tid & 63;                            // opaque per item, as in the producer
      asm volatile("" : "+v"(lane));
      const int lq = lane & 31, hi = lane >> 5;
      if (wave >= 4) __builtin_amdgcn_s_setprio(1);   // the younger wave of a SIMD (attn_slab_bwd_q.hip)
#if BEVR_SLAB_ROWS
      const int i0 = row0 + __builtin_amdgcn_readfirstlane(rb) * SQROWS;     // uniform: a scalar register
#else
      const int i0 = rb * SQROWS;
#endif
      const int qrow = i0 + lq;
      const bool live = lq < SQROWS && qrow < d.S;
      const int rowoff8 = (i0 + lq) * 8;
      const char* Qh = Q + ((size_t)(it.qb * d.heads + it.hd) * Mp) * ROWB;
      const char* dOh = dO + ((size_t)it.ph * Mp) * ROWB;
      const unsigned cells_off = m.cells_off;
      // this lane's four chunks of a staged row (lane = key row lq of a half, its 16-element half `hi`): hi plane of k-step
      // 0 and 1, lo plane of k-step 0 and 1
      const int fsw = slab_x3_swz(lq);
      // transposed reads of the dQ product: the 16-lane block (chalf, hi) reads key rows 4 hi + (i16 >> 2) of an 8-key
      // block, channels 16 chalf + 4 (i16 & 3) .. + 3 of plane P: chunk 4 chalf + 2 P + ((i16 & 3) >> 1), byte 8 (i16 & 1).
      // The swizzle of row 8 blk + rr (rr < 8) is 2 (rr >> 1) | blk
      const int i16 = lane & 15, chalf = (lane >> 4) & 1, rr = 4 * hi + (i16 >> 2);
      const int tr_base = rr * ROWB + 8 * (i16 & 1);
      const int tr_c = (4 * chalf + ((i16 & 3) >> 1)) ^ (2 * (rr >> 1));
      Frag<PREC> qf, dof;
#pragma unroll
      for (int k = 0; k < 16; ++k) qf.v[k] = dof.v[k] = 0.f;      // (initialised: as the producer's load registers)
      float nl = 0.f, nd = 0.f, lse_r = 0.f, dlt_r = 0.f;
      int jcur = -1;
#if BEVR_DROP
      uint32_t hrow = 0u;      // the row part of the keep hash: per column, out of the key-row loops
#endif
      f32x16 dq;
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = 0.f;

      // the rows of column j for this wave's row block: issued (raw) ...
      auto issue_column = [&](int j) {
        const size_t mq = (size_t)j * d.Sp + min(qrow, d.S - 1);
        qf.load(Qh + mq * ROWB, hi);
        dof.load(dOh + mq * ROWB, hi);
        lse_r = LSE[(size_t)it.ph * Mp + mq];
        dlt_r = delta[(size_t)it.ph * Mp + mq];
#if BEVR_DROP
        hrow = bevr_drop_row(drop_seed, (uint32_t)it.ph, (uint32_t)(j * d.Sp + qrow));
#endif
        jcur = j;
      };
      // ... and made ready: lanes without a query compute on a copy of a real one with dO = delta = 0 (their dS is exactly
      // 0); the fixed-point scale of the table-gradient cells is folded into both planes of dO and into delta
      // (attn_bwd_q.hip: gscale is a power of two, the scaling of a bf16 plane is exact)
      auto finish_column = [&]() {
        float dlt = dlt_r;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const unsigned w = live ? __builtin_bit_cast(unsigned, dof.v[k]) : 0u;
          dof.v[k] = __builtin_bit_cast(float, pack_bf16x2(__builtin_bit_cast(float, w << 16) * gscale,
                                                            __builtin_bit_cast(float, w & 0xffff0000u) * gscale));
        }
        if (!live) dlt = 0.f;
        nl = -lse_r;
        nd = -dlt * gscale;
      };
      // one flush per (slab, column): this wave saw every key of the column's run
      auto flush_dq = [&]() {
        // dq[r]: query i0 + crow(r, hi), channel lq (dq_product): a wave instruction adds two 128-byte rows
        // (one lane-dependent pointer and one row bound, made here: as 16 hoisted 64-bit offsets and 16 hoisted lane masks
        // they stayed in registers for the whole kernel)
        float* base = dQ + ((size_t)it.ph * Mp + (size_t)jcur * d.Sp + i0 + 4 * hi) * 32 + lq;
        int nrow = min(SQROWS, d.S - i0) - 4 * hi;      // rows crow(r, 0) < nrow of this lane half are queries
        asm volatile("" : "+v"(nrow));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (crow(r, 0) < nrow) atomicAdd(base + crow(r, 0) * 32, ginv * dq[r]);
          dq[r] = 0.f;
        }
      };
      // a staged row's fragment for this lane
      auto load_row = [&](Frag<PREC>& f, const char* rowp) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(rowp + (((4 * hi + k) ^ fsw) * 16));
          f.v[4 * k + 0] = t[0]; f.v[4 * k + 1] = t[1]; f.v[4 * k + 2] = t[2]; f.v[4 * k + 3] = t[3];
        }
      };

      // One emission against this wave's 31 queries, ONE 32-key half at a time (the 16-bit kernel keeps s and dp of both
      // halves live and issues the second half's products under the first half's loop: with split fragments that spilled):
      // the half's S and dP products, its key-row loop as two interleaved dependency chains (key rows r and r + 8), its dQ
      // product; then the other half.  CLAMP: the row index is clamped into the window.
      auto process = [&](const char* bb, auto clamp_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        // the constants of both halves' keys: lane l holds the record of key bcast_key(l) of each half (attn_tile.h: the
        // key-row loops take theirs from these by DPP)
        f32x4 ckw[2];
        int ckcell[2], ckrow[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const char* p = bb + L::OFF_CK + (h * 32 + bcast_key(lane)) * (int)sizeof(SlabCK);
          ckw[h] = *reinterpret_cast<const f32x4*>(p);
          const u32x2 cr = *reinterpret_cast<const u32x2*>(p + 16);
          ckcell[h] = (int)cr[0];
          ckrow[h] = (int)cr[1];
        }
        float a0 = nl, b0 = nd;
        asm volatile("" : "+v"(a0), "+v"(b0));
        f32x16 s[2], dp[2];
        auto products = [&](int h) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[h][r] = a0; dp[h][r] = b0; }
          Frag<PREC> kf, vkf;
          load_row(kf, bb + (h * 32 + lq) * ROWB);
          s[h] = mma_frag(kf, qf, s[h]);          // S^T - LSE
          load_row(vkf, bb + L::OFF_V + (h * 32 + lq) * ROWB);
          dp[h] = mma_frag(vkf, dof, dp[h]);      // dP^T - delta
        };
        products(0);
        __builtin_amdgcn_sched_barrier(0);
        PROF_T_DRAIN(tq0);
        // byte offset of key row t's first tap VALUE for this lane's row; the gradient cell sits cells_off behind it
        // (8-byte values, 8-byte cells)
        auto offset = [&](int h, int t) -> int {
          const int cell = row_bcast(ckcell[h], t);
          if constexpr (CLAMP) {
            const int row = row_bcast(ckrow[h], t);
            return (cell - 8 * row) + 8 * max(0, min(row + (rowoff8 >> 3), R - 1));
          } else {
            return cell + rowoff8;
          }
        };
        auto read_tap = [&](int off, f32x2& a, f32x2& b) {
          a = *reinterpret_cast<const f32x2*>(lds + off);
          b = *reinterpret_cast<const f32x2*>(lds + off + RP * 8);
        };
        auto dq_product = [&](int h) {
          // B operand K^T[channel lq][key]: element j of k-step ks <-> key 16 ks + 8 (j >> 2) + 4 hi + (j & 3), both planes,
          // out of the swizzled row tile by transposed reads; the A operand is the accumulator tile of dS^T, split here
          typedef s16x4 __attribute__((address_space(3)))* lp;
          const char* kb = bb + h * 32 * ROWB + tr_base;
          // dS is split HERE: without the fence the conversions drift up into the key-row loop, a key row's hi and lo parts
          // live from its step to this product, and the kernel spills
#pragma unroll
          for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(s[h][r]));
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8 kt[2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
              const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(kb + (16 * ks) * ROWB + ((tr_c ^ (2 * pl)) * 16)));
              const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(kb + (16 * ks + 8) * ROWB + ((tr_c ^ (2 * pl) ^ 1) * 16)));
              kt[pl] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
            }
            float xs[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) xs[k] = s[h][8 * ks + k];
            dq = mma_split(split8(xs), Split8{kt[0], kt[1]}, dq);
          }
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (h == 1) {
            products(1);
            __builtin_amdgcn_sched_barrier(0);
          }
#if BEVR_DROP
          // dS = P (keep ? D dP - delta : -delta); dp holds dP - delta, nd = -delta, both in cell units (attn_bwd_q.hip).
          // The hash words of the keys bcast_key(lane), taken by DPP like the constants.  Ahead of the half's key-row
          // loop, four hashes in flight between scheduling fences: no scratch in any of the three placements tried, and
          // this one the fastest per launch (66.8 ms against 67.8 with all sixteen at once and 67.6 with the hashes inside
          // the two-chain loop: DESIGN.md section 5)
          const unsigned kn = *reinterpret_cast<const unsigned*>(bb + L::OFF_KN + (h * 32 + bcast_key(lane)) * 4);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool keep = (bevr_drop_mix(hrow ^ row_bcast(kn, r)) >> 16) >= drop_thr;
            dp[h][r] = keep ? fmaf(ksc, dp[h][r] - nd, nd) : nd;
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
#endif
          // chain c walks the key rows c * 8 + 0 .. 7 of the accumulator tile
          int o0[2];
          f32x2 ta[2], tb[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            o0[c] = offset(h, 8 * c);
            read_tap(o0[c], ta[c], tb[c]);
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            f32x2 na[2], nb[2];
            f32x4 w[2];
            int o1[2];
            // the LDS atomics are ordered memory operations for the compiler (it moves no load across them): the taps of
            // the next key row, of BOTH chains, are requested before the adds of this step are issued
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              na[c] = ta[c]; nb[c] = tb[c]; o1[c] = o0[c];
              if (r + 1 < 8) { o1[c] = offset(h, 8 * c + r + 1); read_tap(o1[c], na[c], nb[c]); }
#pragma unroll
              for (int k = 0; k < 4; ++k) w[c][k] = row_bcast(ckw[h][k], 8 * c + r);
            }
            int iA[2], iB[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int row = 8 * c + r;
              const float sv = fmaf(tb[c][1], w[c][3], fmaf(tb[c][0], w[c][2], fmaf(ta[c][1], w[c][1], fmaf(ta[c][0], w[c][0], s[h][row]))));
              const float ds = fast_exp2(sv) * dp[h][row];   // masked keys: -big from the kill column => 0
              s[h][row] = ds;
              // table row (A + l) of column X receives w00 dS[query l] + w01 dS[query l - 1] (attn_bwd_q.hip); already in
              // cell units
              const float gb_ = lane_below(ds);
              iA[c] = cvt_rpi(fmaf(gb_, w[c][1], ds * w[c][0]));
              iB[c] = cvt_rpi(fmaf(gb_, w[c][3], ds * w[c][2]));
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              unsigned long long* gp = reinterpret_cast<unsigned long long*>(lds + cells_off + o0[c]);
              atomicAdd(gp, AccCell::from_int(iA[c]));
              atomicAdd(gp + RP, AccCell::from_int(iB[c]));
              ta[c] = na[c]; tb[c] = nb[c]; o0[c] = o1[c];
            }
          }
          // the half's dQ product: issued here, it runs under the other half's loop (h = 0) or the barrier wait (h = 1)
          dq_product(h);
          __builtin_amdgcn_sched_barrier(0);
        }
        PROF_T_DRAIN(tq1);
        PROF_ADD(4, tq1 - tq0);      // worker: the key-row loops and dQ products
      };

      int e = 0;
      for (;;) {
        PROF_T_DRAIN(tw0);
        SLAB_BARRIER();
        PROF_T_DRAIN(tw1);
        PROF_ADD(0, tw1 - tw0);      // worker: barrier wait
        const char* bb = m.stage + (e & 1) * L::BUF;
        const SlabCtl ct = slab_read_ctl(bb);
        if (ct.done()) break;
        if (active) {
          // (no prefetch of the next column's rows into the registers of Q and dO, as the 16-bit kernel has it: the
          // conditional reload of 32 registers kept the old and the new rows live across the products and the kernel
          // spilled; a column's ~9 emissions at the benchmark shape wait for these loads once)
          if (ct.first()) {
            issue_column(ct.j());
            finish_column();
          }
          const unsigned hb = ct.halves();
          if (hb & 3u) {
            if (hb & 12u) process(bb, std::true_type{});
            else process(bb, std::false_type{});
          }
          if (ct.last()) flush_dq();
        }
        PROF_T_DRAIN(tw2);
        PROF_ADD(1, tw2 - tw1);      // worker: the emission
        PROF_ADD(2, ct.halves() & 1u);
        PROF_ADD(3, 1);
        ++e;
      }
    }

    // ---- flush the slab: every cell once ----------------------------------------------------------------------------
    SLAB_BARRIER();
    PROF_T_DRAIN(tf0);
    slab_flush<RP>(tid, m, d, it, sw, R, ginv);
    PROF_T_DRAIN(tf1);
    PROF_ADD(13, tf1 - tf0);     // slab out
  }
  PROF_FLUSH(slab_x3, producer ? 32 : (wave ? 16 : 0), (tid & 63) == 0 && (wave == 0 || wave == SNWORK - 1 || producer));
}

}  // namespace
