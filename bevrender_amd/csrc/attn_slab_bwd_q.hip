// Slab query-side backward, the 16-bit body (BEVR_PREC_BF16, BEVR_PREC_F16): bevr_attn_slab_bwd_q, and through the stub
// units attn_slab_bwd_q_rows.hip (BEVR_SLAB_ROWS = 1) and attn_slab_bwd_q_drop.hip (BEVR_DROP = 1) bevr_attn_slab_bwd_q_rows
// and bevr_attn_slab_bwd_q_dropout.  attn_slab.h describes the formulation and holds everything but the arithmetic; what
// is this body's own: 80-byte staged K / V rows, table values, taps and weights as packed 16-bit pairs (a value cell is
// one dword), the key-row loop on dot2 with the table-gradient sums in inline assembly, BOTH halves' S and dP products
// ahead of the first half's loop, and the next column's Q / dO rows prefetched into the registers of this one's.
#include "attn_slab.h"

// clocks summed over the emissions of wave 0 (a worker, at 0), wave 6 (the last worker, at 16) and the producer (at 32) of
// every workgroup, 16 slots each
BEVR_PROF_DEFINE(slab, 48)

namespace {

SLAB_KERNEL_SIGNATURE {
  typedef SlabLds L;
  extern __shared__ __attribute__((aligned(256))) char lds[];
#if !BEVR_SLAB_ROWS
  constexpr int RP = SLAB_RP;
#endif
  const SlabMem<unsigned> m = slab_carve<unsigned, RP>(lds, sw);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lq = lane & 31, hi = lane >> 5;
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

  const float gscale = grad_scale[0], ginv = grad_scale[1] * BEVR_LN2;
  const float kp16 = PREC == BEVR_PREC_F16 ? grad_scale[2] : 0.f, c2_16 = PREC == BEVR_PREC_F16 ? grad_scale[3] : 1.f;
  const float cfix = PREC == BEVR_PREC_F16 ? grad_scale[0] * grad_scale[4] : 1.f;
  const float dq_scale = PREC == BEVR_PREC_F16 ? grad_scale[4] * BEVR_LN2 : ginv;
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

    // ---- the slab: values in, cells cleared -----------------------------------------------------------------------
    slab_fill<RP>(tid, m, d, it, sw, R, [](f32x2 v) { return Half<PREC>::pack2(v[0], v[1]); },
                  Half<PREC>::pack2(Half<PREC>::NEG_BIG, Half<PREC>::NEG_BIG));
    SLAB_BARRIER();
    PROF_T_DRAIN(ti1);
    PROF_ADD(12, ti1 - ti0);     // slab in
    PROF_ADD(15, 1);             // items

    if (producer) {
      // =========================================== PRODUCER ========================================================
      __builtin_amdgcn_s_setprio(3);
      const SlabKey* kp = skeys + (size_t)it.pg * d.N;
      const char* Kh = Ks + (size_t)it.ph * d.N * 64;
      const char* Vh = Vs + (size_t)it.ph * d.N * 64;
      SlabRuns runs;
      runs.start(lane, kbeg, kend, d, it, n_slab);
      u32x4 kv[8];
      SlabKey sk;
      bool have = false;
      auto issue = [&]() {      // loads of the emission at the iterator; then step the iterator
        have = runs.more();
        if (!have) return;
        runs.take();
        const int kmax = d.N - 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cid = lane + 64 * q;                       // chunk of the K tile: key cid / 4, part cid % 4
          const int key = min(runs.k0 + (cid >> 2), kmax);
          kv[q] = *reinterpret_cast<const u32x4*>(Kh + (size_t)key * 64 + (cid & 3) * 16);
          kv[4 + q] = *reinterpret_cast<const u32x4*>(Vh + (size_t)key * 64 + (cid & 3) * 16);
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
        u32x4 kv_e[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) kv_e[q] = kv[q];
        PROF_T_DRAIN(tp1);
        PROF_ADD(0, tp1 - tp0);      // producer: wait for this emission's loads
        issue();              // the next emission's loads fly while this one is written and processed
        // ---- constants of (column j, key) ----
        {
          const float tx = jrx + sk_e.b;
          const float xf = floorf(tx);
          const int X = (int)xf;
          const bool live = (em.k0 + lane < em.kend) && X >= it.x0 && X < it.x0 + sw;
          const float fx = tx - xf, fy = sk_e.fy;
          SlabCK ck;
          if (live) {
            ck.wA = Half<PREC>::pack2((1.0f - fx) * (1.0f - fy), (1.0f - fx) * fy);
            ck.wB = Half<PREC>::pack2(fx * (1.0f - fy), fx * fy);
            ck.row = sk_e.A + SLAB_ROW0;
            ck.cell = ((X - it.x0 + 1) * RP + ck.row) * 4;    // BYTE offset of the first tap's value entry
          } else {          // masked: first tap in the kill column => P = 0, dS = 0
            ck.wA = Half<PREC>::pack2(1.f, 0.f);
            ck.wB = 0u;
            ck.row = 0;
            ck.cell = 0;
          }
          *reinterpret_cast<SlabCK*>(bb + L::OFF_CK + lane * 16) = ck;
#if BEVR_DROP
          // the keys arrive sorted by b: the mask is of the ORIGINAL index (SlabKey::pad, this unit's prep)
          *reinterpret_cast<unsigned*>(bb + L::OFF_KN + lane * 4) = (unsigned)sk_e.pad * 0xC2B2AE3Du;
#endif
          // the column after this one (the iterator is one emission ahead): the workers prefetch its Q / dO rows
          const int jn = (em.last && have) ? it.j0 + runs.c + 1 : 0;
          slab_post(bb, lane, live, live && slab_far(d, sk_e.A), em, j, (unsigned)jn);
        }
        // ---- K and V rows ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cid = lane + 64 * q;
          *reinterpret_cast<u32x4*>(bb + (cid >> 2) * SKROW + (cid & 3) * 16) = kv_e[q];
          *reinterpret_cast<u32x4*>(bb + L::OFF_V + (cid >> 2) * SKROW + (cid & 3) * 16) = kv_e[4 + q];
        }
        ++e;
        PROF_T_DRAIN(tp2);
        PROF_ADD(1, tp2 - tp1);      // producer: constants, stores, next loads issued
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
      // waves 4 .. 6 share a SIMD with waves 0 .. 2, and the issue arbitration favours the older wave: the phase stamps had
      // wave 6's key-row loop 26 % longer than wave 0's, and the barrier waits for the slowest
      if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#if BEVR_SLAB_ROWS
      const int i0 = row0 + __builtin_amdgcn_readfirstlane(rb) * SQROWS;     // uniform: a scalar register
#else
      const int i0 = rb * SQROWS;
#endif
      const int qrow = i0 + lq;
      const bool live = lq < SQROWS && qrow < d.S;
      const int rowoff4 = (i0 + lq) * 4;
      const char* Qh = Q + ((size_t)(it.qb * d.heads + it.hd) * Mp) * 64;
      const char* dOh = dO + ((size_t)it.ph * Mp) * 64;
      const unsigned cells_off = m.cells_off;
      Frag<PREC> qf, dof;
      float nl = 0.f, nd = 0.f, lse_r = 0.f, dlt_r = 0.f;
      int jcur = -1, jpend = -1;
#if BEVR_DROP
      uint32_t hrow = 0u;      // the row part of the keep hash: per column, out of the key-row loops
#endif
      f32x16 dq;
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = 0.f;

      // the rows of column j for this wave's row block: issued (raw) ...
      auto issue_column = [&](int j) {
        const size_t mq = (size_t)j * d.Sp + min(qrow, d.S - 1);
        qf.load(Qh + mq * 64, hi);
        dof.load(dOh + mq * 64, hi);
        lse_r = LSE[(size_t)it.ph * Mp + mq];
        dlt_r = delta[(size_t)it.ph * Mp + mq];
        jpend = j;
      };
      // ... and made ready: lanes without a query compute on a copy of a real one with dO = delta = 0 (their dS is exactly
      // 0); the fixed-point scale of the table-gradient cells is folded into dO and delta (attn_bwd_q.hip)
      auto finish_column = [&]() {
        float dlt = dlt_r;
        if (!live) {
          dof.v[0] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          dof.v[1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          dlt = 0.f;
        }
        if constexpr (PREC != BEVR_PREC_F16) dlt *= gscale;
        if constexpr (PREC == BEVR_PREC_BF16) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            u32x4 w = __builtin_bit_cast(u32x4, dof.v[h]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              w[k] = pack_bf16x2(__builtin_bit_cast(float, w[k] << 16) * gscale,
                                 __builtin_bit_cast(float, w[k] & 0xffff0000u) * gscale);
            dof.v[h] = __builtin_bit_cast(bf16x8, w);
          }
        }
        nl = kp16 - lse_r;
        nd = -dlt;
#if BEVR_DROP
        hrow = bevr_drop_row(drop_seed, (uint32_t)it.ph, (uint32_t)(jpend * d.Sp + qrow));
#endif
        jcur = jpend;
      };
      // one flush per (slab, column): this wave saw every key of the column's run
      auto flush_dq = [&]() {
        // dq[r]: query i0 + crow(r, hi), channel lq (dq_product): a wave instruction adds two 128-byte rows
        float* base = dQ + ((size_t)it.ph * Mp + (size_t)jcur * d.Sp + i0) * 32 + lq;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qr = crow(r, hi);
          if (qr < SQROWS && i0 + qr < d.S) atomicAdd(base + (size_t)qr * 32, dq_scale * dq[r]);
          dq[r] = 0.f;
        }
      };

      // One emission -- both 32-key halves, one after the other -- against this wave's 31 queries.  The key-row loop of a
      // half runs TWO key rows per step (rows r and r + 8: two independent dependency chains written side by side): with
      // two waves per SIMD the latency of a chain (LDS round trips: constants -> taps -> ... -> atomics) is covered by
      // the other chain and the other wave, where the 14-wave version (one half per wave, one row per step) needed
      // 128-register waves that spilled.  The matrix products are placed so that they run UNDER a loop: S and dP of the
      // second half are issued before the first half's loop, the first half's dQ product before the second half's loop.
      // CLAMP: the row index is clamped into the window.  jn >= 0: the column's last emission -- once the products that
      // read Q and dO are issued, the rows of column jn are requested INTO the same registers.
      auto process = [&](const char* bb, int jn, auto clamp_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        // the constants of both halves' keys: lane l holds the record of key bcast_key(l) of each half (attn_tile.h: the
        // key-row loops take theirs from these by DPP)
        u32x4 ck[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
          ck[h] = *reinterpret_cast<const u32x4*>(bb + L::OFF_CK + (h * 32 + bcast_key(lane)) * (int)sizeof(SlabCK));
        f32x16 s[2], dp[2];
        {
          float a = nl, b = nd;
          asm volatile("" : "+v"(a), "+v"(b));
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[h][r] = a; dp[h][r] = b; }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Frag<PREC> kf, vkf;
          kf.load(bb + (h * 32 + lq) * SKROW, hi);
          s[h] = mma_frag(kf, qf, s[h]);          // S^T - LSE
          vkf.load(bb + L::OFF_V + (h * 32 + lq) * SKROW, hi);
          dp[h] = mma_frag(vkf, dof, dp[h]);      // dP^T - delta
        }
        if (jn >= 0) issue_column(jn);
        __builtin_amdgcn_sched_barrier(0);
        PROF_T_DRAIN(tq0);
        // byte offset of key row t's first tap VALUE for this lane's row; the gradient cell sits at twice that (8-byte
        // cells behind the 4-byte values)
        auto offset = [&](const u32x4& k, int t) -> int {
          const int cell = row_bcast((int)k[2], t);
          if constexpr (CLAMP) {
            const int row = row_bcast((int)k[3], t);
            return (cell - 4 * row) + 4 * max(0, min(row + (rowoff4 >> 2), R - 1));
          } else {
            return cell + rowoff4;
          }
        };
        auto read_tap = [&](int off, unsigned& a, unsigned& b) {
          a = *reinterpret_cast<const unsigned*>(lds + off);
          b = *reinterpret_cast<const unsigned*>(lds + off + RP * 4);
        };
        auto dq_product = [&](int h) {
          // A operand K^T[channel lq][key] for the accumulator contraction: element j of k-step s <-> key
          // 16 s + 8 (j >> 2) + 4 hi + (j & 3) (bevr_common.h: mma_acc_b), out of the row tile by transposed reads
          Frag<PREC> ktf;
          const int i16 = lane & 15, chalf = (lane >> 4) & 1;
          const char* p = bb + (h * 32 + 4 * hi + (i16 >> 2)) * SKROW + chalf * 32 + 8 * (i16 & 3);
          ktf.v[0] = lds_tr8(p, 8 * SKROW);
          ktf.v[1] = lds_tr8(p + 16 * SKROW, 8 * SKROW);
          // dQ[query][channel] += dS[query][key] K[key][channel]: the accumulator tile of dS^T (key rows in registers, query
          // on the lane) is the A operand as it stands -- lane (query, hi) holds the keys crow(8 s + j, hi) of k-step s,
          // the same key order as ktf's -- and the product comes out with the CHANNEL on the lane: the flush below adds
          // 128 contiguous bytes per query row (with the query on the lane, as the first version had it, every lane of an
          // atomic instruction hit its own cache line: 85 GB of atomic write traffic per launch against ~23 GB of payload)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            u32x4 w;
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = Half<PREC>::pack2(s[h][8 * ks + 2 * k], s[h][8 * ks + 2 * k + 1]);
            dq = Half<PREC>::mfma(__builtin_bit_cast(bf16x8, w), ktf.v[ks], dq);
          }
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#if BEVR_DROP
          // dS = P (keep ? D dP - delta : -delta); dp holds dP - delta, nd = -delta (attn_bwd_q.hip).  Ahead of the half's
          // key-row loop, which needs dp at once anyway: inside it the hashes of two chains cost more registers than a
          // wave has (40 bytes of scratch per lane)
          // (the hash words of the keys bcast_key(lane), taken by DPP like the constants)
          const unsigned kn = *reinterpret_cast<const unsigned*>(bb + L::OFF_KN + (h * 32 + bcast_key(lane)) * 4);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool keep = (bevr_drop_mix(hrow ^ row_bcast(kn, r)) >> 16) >= drop_thr;
            dp[h][r] = keep ? fmaf(ksc, dp[h][r] - nd, nd) : nd;
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four hashes in flight, not sixteen: registers
          }
#endif
          // chain c walks the key rows c * 8 + 0 .. 7 of the accumulator tile
          const u32x4 k = ck[h];
          int o0[2];
          unsigned ta[2], tb[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            o0[c] = offset(k, 8 * c);
            read_tap(o0[c], ta[c], tb[c]);
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            unsigned na[2], nb[2], wA[2], wB[2];
            int o1[2];
            // the LDS atomics are ordered memory operations for the compiler (it moves no load across them): the taps of
            // the next key row, of BOTH chains, are requested before the adds of this step are issued
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              na[c] = ta[c]; nb[c] = tb[c]; o1[c] = o0[c];
              if (r + 1 < 8) { o1[c] = offset(k, 8 * c + r + 1); read_tap(o1[c], na[c], nb[c]); }
              wA[c] = row_bcast(k[0], 8 * c + r);
              wB[c] = row_bcast(k[1], 8 * c + r);
            }
            int iA[2], iB[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int row = 8 * c + r;
              float sv = Half<PREC>::dot2(ta[c], wA[c], s[h][row]);
              sv = Half<PREC>::dot2(tb[c], wB[c], sv);
              float ds = fast_exp2(sv) * dp[h][row];
              if constexpr (PREC == BEVR_PREC_F16) ds *= c2_16;
              s[h][row] = ds;
              const float gb_ = lane_below(ds);
              if constexpr (PREC == BEVR_PREC_BF16) {
                const unsigned pr = pack_bf16x2(ds, gb_);
                asm("v_dot2_f32_bf16 %0, %2, %3, 0\n\t"
                    "v_dot2_f32_bf16 %1, %2, %4, 0\n\t"
                    "s_nop 2\n\t"
                    "v_cvt_rpi_i32_f32 %0, %0\n\t"
                    "v_cvt_rpi_i32_f32 %1, %1"
                    : "=&v"(iA[c]), "=&v"(iB[c])
                    : "v"(pr), "v"(wA[c]), "v"(wB[c]));
              } else {
                const unsigned pr = Half<PREC>::pack2(ds, gb_);
                asm("v_dot2_f32_f16 %0, %2, %3, 0\n\t"
                    "v_dot2_f32_f16 %1, %2, %4, 0\n\t"
                    "s_nop 2\n\t"
                    "v_mul_f32 %0, %0, %5\n\t"
                    "v_mul_f32 %1, %1, %5\n\t"
                    "v_cvt_rpi_i32_f32 %0, %0\n\t"
                    "v_cvt_rpi_i32_f32 %1, %1"
                    : "=&v"(iA[c]), "=&v"(iB[c])
                    : "v"(pr), "v"(wA[c]), "v"(wB[c]), "v"(cfix));
              }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              unsigned long long* gp = reinterpret_cast<unsigned long long*>(lds + cells_off + 2 * o0[c]);
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
          const int j = ct.j();
          if (ct.first()) {
            if (jpend != j) issue_column(j);      // not prefetched: an item's first column
            finish_column();
          }
          const unsigned hb = ct.halves();
          if (hb & 3u) {
            const int jn = ct.last() ? ct.jn() - 1 : -1;
            if (hb & 12u) process(bb, jn, std::true_type{});
            else process(bb, jn, std::false_type{});
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
  PROF_FLUSH(slab, producer ? 32 : (wave ? 16 : 0), lane == 0 && (wave == 0 || wave == SNWORK - 1 || producer));
}

}  // namespace
