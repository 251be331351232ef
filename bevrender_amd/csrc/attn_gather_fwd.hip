// Forward of the GATHER kernels: attention over SCATTERED keys (the camera-visible keys of SCA in their static k-d
// order, TSA's keys) with every product on the matrix cores, 16-bit operand modes.
//     S[n][q] = scale Q_q . K_n + bias[n][q],   bias = bilinear sample of the rpe table at (i + a_n, j rx + b_n)
//     O_q     = softmax_n(S) V                  (model/SCA_deform_attn.py:331-413, model/TSA_deform_attn.py:245-333)
// Same operands, key workspace and outputs (O normalised, two LSE planes) as bevr_attn_fwd (attn_fwd.hip), which it
// replaces for the 16-bit modes; the table arrives as 16-bit PAIRS, table_pk[h][Wp][Hp] = (T2[y][x], T2[y + 1][x]).
//
// The bias as a matrix product with a SPARSE contraction: a 16-key tile has 64 slots, slot (key n', tap) -- the four
// bilinear taps of key n' in the order (y, x), (y + 1, x), (y, x + 1), (y + 1, x + 1):
//     bias^T[n][q] = sum_slots W[n][slot] Tg[slot][q],    W[n][(n', tap)] = w_tap(n) [n' == n],
//                                                          Tg[(n', tap)][q] = T2[A_n' + i_q + dy][X_n' + dx]
// Tg is the B operand exactly as the lanes GATHER it: lane (q, k-group) holds one dword (a (y, y + 1) pair) of each of four
// keys at ONE of their two table columns -- ds_read_b32 from an LDS WINDOW of the pair table; the 16 lanes of a k-group
// read 16 consecutive rows of one column, the two k-groups of a half wave the columns x and x + 1 of the same key, a
// column stride = 16 (mod 32 banks) apart: no bank conflicts wherever the key lies (round 4's slot order -- two keys x two
// columns per lane, the k-groups on DIFFERENT keys -- lost 34 % of the LDS cycles to them).  W is block diagonal: zero
// except for the 8 bytes (four packed weights) each key owns.  Per 16 keys x 16 BEV rows: 3 MFMAs for S (QK^T + 2 x bias), 1 for
// PV, 4 LDS gathers; no per-pair arithmetic but the exponential.
//
// Work split (as the tap kernels, attn_tap_fwd.hip): workgroup = ONE BEV column j of one (problem, head); wave w owns
// the 16-row blocks [w NB, (w + 1) NB) of the column; the LAST wave is the PRODUCER.  Per emission (one 32-key tile) it
// stages the K rows, the V rows (two 16-channel images for the transposed reads of the PV product), the W image, every
// key's window address, and the WINDOW itself: the columns [x0, x1] x rows [a0, a0 + ROWS) of the pair table that the
// tile's taps reach for ALL BEV rows of the column (a k-d leaf of 32 keys: ~13 columns x 256 rows, 13 KB, one 16-byte
// load per lane and column).  Two buffers: the producer fills emission e + 1 while the row-block waves work on e; one
// barrier per emission.
//
// ANY key set is handled: a tile whose box does not fit the window (more than WIN_COLS columns or ROWS rows) is emitted
// in groups of 14 keys with one two-column STRIP of the table per key, the other keys masked.
//
// Softmax reference: STATIC.  The first pass works against the caller's mref[q] (an upper bound of the row's logits minus
// a headroom, bevrender_amd/ops.py): no running maximum, rescale or mass test in the loop.  A row whose weights all
// underflowed against it flags its column and the EXACT instantiation -- the only one with an online maximum (the
// maximum of the row's first tile, raised with a rescale when a later logit exceeds it) -- recomputes that column.
// The row's largest weight is tracked beside the sums for LSE plane 1.
//
// BEVR_GATHER_ROWS = 1 (attn_gather_fwd_rows.hip, a translation unit of its own so that the whole-column kernels stay
// the code they were): the ROW-RANGE kernels.  A workgroup computes the BEV rows [row0, row0 + n_rows) of its column
// (row0 a multiple of 16, at most 14 row blocks) instead of the whole column: query rows are independent, so only the
// row ORIGIN moves -- the table row of a tap for the band's first BEV row, the Q / mref / O / LSE rows and the rows a
// window must hold.  Rows outside the band are not written; the band that ends at S writes the rows past the grid as the
// whole-column kernel does.  BEV sides up to 448 run as bands of at most 224 rows (bevrender_amd/ops.py).
//
// BEVR_GATHER_X3 = 1 (attn_gather_fwd_x3.hip, a translation unit of its own again, with BEVR_GATHER_ROWS = 1: the split
// mode takes a row range from the start): BEVR_PREC_BF16X3.  Every matrix operand is two bf16 IMAGES, hi = bf16(x) and
// lo = bf16(x - hi), of the 16-bit mode's shape and addressing, the lo image a fixed distance behind the hi image
// (LdsGn<2>), and a product is three MFMAs, lo hi + hi lo + hi hi (mfma16s, attn_tap.h):
//   Q, K, V   arrive in the split ROW format (bevr_common.h: 128-byte rows, per 16-element half hi(e0..7) | hi(e8..15) |
//             lo(e0..7) | lo(e8..15)); the producer's direct-to-LDS loads put each 16-byte chunk into the image that
//             needs it -- K hi / lo with the swizzle of the 16-bit image, V as a hi and a lo image of each channel half
//   table     table_pk2[2][heads][Wp][Hp]: plane 0 the pairs of hi parts, plane 1 the pairs of lo parts; a window holds
//             both, the lo plane LdsGn::WIN_PLANE behind the hi plane: ONE address per key, two direct-to-LDS loads per column
//   W         computed in f32 by the producer, a hi and a lo image in the layout of w_image_pos
//   P         split in registers after exp2; the row sum is the ones-operand product of BOTH parts -- of the values PV
//             contracts
// One workgroup per CU (152 KB of LDS), two waves per SIMD: see DESIGN.md "Split-bf16 mode on the gather forward".
//
// BEVR_DROP = 1 (attn_gather_fwd_drop.hip, a translation unit of its own, with BEVR_GATHER_ROWS = 1): attention dropout,
// the semantics of bevr_attn_fwd_dropout (attn_fwd.hip).  The keep decision of pair (ph, mq = j Sp + ABSOLUTE BEV row,
// n = the key's index in the caller's order) is bevr_drop_keep's (bevr_common.h); the row part of the hash is formed once
// per row block, the key part once per emission (the emission's first key index travels in the control word's third
// dword, free with NT = 1) -- a strip emission and the EXACT pass hash the same index and so decide alike.  Softmax
// first: the row sum (a ones-operand product, as without a mask), the largest weight and both LSE planes are of ALL the
// rounded weights; PV contracts the same packed weights with the dropped ones' 16 bits cleared; D = 65536 / (65536 -
// drop_thr) multiplies O in the epilogue (the fp16 operands stay the unscaled weights).
#include "attn_tap.h"
#include "attn_host.h"

#ifndef BEVR_GATHER_ROWS
#define BEVR_GATHER_ROWS 0
#endif
#ifndef BEVR_GATHER_X3
#define BEVR_GATHER_X3 0
#endif

#include "bevr_prof.h"

BEVR_PROF_DEFINE(gather, 32)   // 8 slots each: the producer wave (at 0), row-block waves 0 (at 8) and 3 (at 16)

namespace {

constexpr int GT = 32;                 // keys per emission (one 32-key tile; 64: two tiles that share one window -- too
                                       // wide for WIN_COLS at the benchmark: 1.7x the emissions)
constexpr int NT = GT / 32;
constexpr int ROWS = 256;              // window rows (dwords) per column: one 16-byte load per lane
constexpr int PITCH = 272;             // column stride in dwords, = 16 (mod 32): the two 16-lane k-groups of a half wave read
                                       // rows i .. i + 15 of columns x and x + 1 of ONE key -- opposite halves of the 32 banks
                                       // of ds_read_b32, conflict-free for every key position
constexpr int WIN_COLS = 28;
constexpr int STRIP_KEYS = WIN_COLS / 2;
// NP: images per operand (1; split mode 2: the lo image of K, of each V half, of W and of the window K_IMG, V_IMG, W_IMG
// and WIN_PLANE bytes behind the hi image)
template <int NP> struct LdsGn {
  static constexpr int K_IMG = GT * 64, V_IMG = GT * 32, W_IMG = (GT / 16) * 2 * 64 * 16;
  static constexpr int OFF_K = 0;                       // [64 keys][4 chunks of 16 B], chunk c of key n at position c ^ ((n >> 2) & 3)
  static constexpr int OFF_VLO = NP * K_IMG;            // [64 keys][16 channels] 16-bit: channels 0..15
  static constexpr int OFF_VHI = OFF_VLO + NP * V_IMG;  // channels 16..31
  static constexpr int OFF_W = OFF_VHI + NP * V_IMG;    // the W operand AS THE LANES HOLD IT: [16-key sub-tile][bias product][lane]
                                                        // 16 bytes; zero but for one dword per (key, column): w_image_pos
  static constexpr int W_BYTES = NP * W_IMG;
  static constexpr int OFF_OFF = OFF_W + W_BYTES;       // [64 keys] LDS byte address of tap (y, x) for BEV row 0
  static constexpr int OFF_CT = OFF_OFF + GT * 4;       // u32x4: flags (bit 2: done), live keys 0..31, 32..63, entries of the fill list
  static constexpr int OFF_FD = OFF_CT + 16;            // fill list of the NEXT emission's window: [WIN_COLS] (column, first row)
  static constexpr int BUF = OFF_FD + WIN_COLS * 8;
  static constexpr int WIN_PLANE = WIN_COLS * PITCH * 4;
  static constexpr int WIN = NP * WIN_PLANE;
  static constexpr int OFF_WIN = 2 * BUF;
  static constexpr int TOTAL = OFF_WIN + 2 * WIN;
};
typedef LdsGn<BEVR_GATHER_X3 ? 2 : 1> LdsG;
static_assert(LdsG::BUF % 16 == 0 && LdsG::WIN % 16 == 0, "16-byte aligned LDS blocks");
// 16-bit modes: two workgroups per CU; split mode: one (both planes of two full windows: DESIGN.md)
static_assert((BEVR_GATHER_X3 ? 1 : 2) * LdsG::TOTAL <= 160 * 1024, "workgroups per CU");
static_assert(LdsG::WIN_PLANE + 2 * QB * 4 < 65536, "the lo plane of a tap is an immediate offset of its hi plane's read");
// Slot order of a bias product (8 keys x 4 taps = 32 slots of the contraction): k-group kg holds the dwords ((y, y + 1)
// pairs) of keys 4 (kg >> 1) + {0 .. 3} at table column x + (kg & 1).  The A operand of product m of a 16-key sub-tile is
// then, for lane (key li, k-group kg), dword dd = the key's packed weights of that column if li == 8 m + 4 (kg >> 1) + dd,
// else 0: byte offset in the W image of the dword that key n (0 .. 15) owns for column c (0, 1); the other column's is
// 256 bytes further.
__device__ __forceinline__ int w_image_pos(int n) {
  const int m = n >> 3, half = (n >> 2) & 1, dd = n & 3;
  return (m * 64 + n + 32 * half) * 16 + dd * 4;
}
// Workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global load in flight
// (s_waitcnt vmcnt(0)): the prefetches that are meant to cross the barrier.
__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
constexpr float RAISE = 40.0f;   // EXACT: binades a logit may exceed the reference before the reference moves
// fp16 operands: the weights are rounded to 5 exponent bits (largest value 2^15.99, normal down to 2^-14, zero under 2^-25).
// The EXACT reference is put F16_LIFT binades UNDER the maximum it has seen, so that weights down to 2^-(25 + F16_LIFT) of
// the row's largest survive, and moves when a logit exceeds it by F16_RAISE binades (2^15 is an fp16 number; the rescale
// of already packed weights multiplies by 2^-delta <= 1).
constexpr float F16_RAISE = 15.0f;
constexpr float F16_LIFT = 8.0f;
// fp16, static pass: a weight under 2^-14 is stored with an absolute error of up to 2^-25 (subnormal step 2^-24; zero
// under 2^-25), so N keys move the row sum and the numerator of O by up to N 2^-25 (x max |V|) -- relative to the row
// sum, which is at least the largest ROUNDED weight pmax: N 2^-25 / pmax.  Held to 2^-11, one rounding of an fp16 operand
// (a fifth of the mode's output tolerance 2.5e-3): a row with pmax < N 2^-14 sends its column to the exact pass.
constexpr float F16_PMAX_PER_KEY = 6.103515625e-05f;      // 2^-14

template <int V> struct IntC { static constexpr int value = V; };
typedef const char __attribute__((address_space(1)))* gptr_t;
typedef char __attribute__((address_space(3)))* lptr_t;
// 64 lanes x 16 bytes, global (per-lane address) -> LDS (base + 16 lane), no registers
__device__ __forceinline__ void glds16(const char* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_base, 16, 0, 0);
}

#if BEVR_DROP
static_assert(BEVR_GATHER_ROWS && !BEVR_GATHER_X3, "the keep mask: the 16-bit row-range kernels");
#define BEVR_GATHER_KERNEL attn_gather_fwd_drop_kernel
#define BEVR_GATHER_ROW_PARAMS , const int row0, const int n_rows, const unsigned drop_thr, const unsigned drop_seed
#define BEVR_GATHER_WAVES_PER_SIMD 4
#elif BEVR_GATHER_X3
#define BEVR_GATHER_KERNEL attn_gather_fwd_x3_kernel
#define BEVR_GATHER_ROW_PARAMS , const int row0, const int n_rows
#define BEVR_GATHER_WAVES_PER_SIMD 2      // one workgroup of 8 waves per CU: 256 registers
#elif BEVR_GATHER_ROWS
#define BEVR_GATHER_KERNEL attn_gather_fwd_rows_kernel
#define BEVR_GATHER_ROW_PARAMS , const int row0, const int n_rows
#define BEVR_GATHER_WAVES_PER_SIMD 4
#else
#define BEVR_GATHER_KERNEL attn_gather_fwd_kernel
#define BEVR_GATHER_ROW_PARAMS
#define BEVR_GATHER_WAVES_PER_SIMD 4
#endif
// table_pk: the 16-bit pair table [heads][Wp][Hp]; split mode: table_pk2 [2][heads][Wp][Hp], plane 1 the lo parts
template <int PREC, int NB, bool EXACT, bool DMA>
__global__ __launch_bounds__(512, BEVR_GATHER_WAVES_PER_SIMD) void BEVR_GATHER_KERNEL(
    bevr_attn_desc d, const char* __restrict__ Q, const char* __restrict__ K, const char* __restrict__ V,
    const char* __restrict__ key_ws, const uint32_t* __restrict__ table_pk, const float* __restrict__ mref,
    float* __restrict__ O, float* __restrict__ LSE, int* __restrict__ flags BEVR_GATHER_ROW_PARAMS) {
  constexpr bool BAND = BEVR_GATHER_ROWS != 0;
  constexpr bool X3 = tap_split(PREC);
  static_assert(X3 == (BEVR_GATHER_X3 != 0), "the split mode lives in its own translation unit");
  static_assert(!X3 || BAND, "the split mode takes a row range");
  constexpr int NP = tap_np<PREC>;            // images per operand
  constexpr int ROWB = X3 ? 128 : 64;         // bytes of a Q / K / V row
  typedef TapHalf<PREC> H16;                  // the 16-bit arithmetic the images are made with
#if !BEVR_GATHER_ROWS
  constexpr int row0 = 0, n_rows = 0;      // the whole column
#endif
  typedef LdsG L;
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
  const int nblk = ((BAND ? n_rows : d.S) + QB - 1) / QB;      // row blocks of the column (BAND: of the band)
  const int rows_q = nblk * QB;
  const int row_end = BAND ? row0 + n_rows : d.S;
  const bool to_end = !BAND || row_end == d.S;                 // this launch owns the rows past the grid
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const float jrx = (float)j * rx;
  const unsigned smem_base = (unsigned)(size_t)(lptr_t)smem;     // window addresses are handed over as LDS addresses

  // ---- the window fill, shared by ALL waves: entry c of a fill list = (padded table column, first table row) of window
  // column c; wave w copies the entries w, w + n_wave, ...  One column = ROWS dwords = 64 lanes x 16 bytes, global -> LDS
  // directly (no registers): issued when an emission starts, waited for before its closing barrier -- the L2 latency hides
  // behind the emission's matrix work.  A table shorter than a window column (small problems) goes through registers.
  const char* tbl = reinterpret_cast<const char*>(table_pk + (size_t)hd * d.Wp * d.Hp);
  const unsigned lane16 = (unsigned)lane * 16u;
  const size_t tbl_plane = (size_t)d.heads * d.Wp * d.Hp * 4;      // split mode: bytes from the hi plane to the lo plane
  auto fill_one = [&](char* win, int c, int xc, int r0) {      // xc, r0: uniform
    static_assert(ROWS == 256, "one 16-byte load per lane and column");
    BEVR_ASSERT(c >= 0 && c < WIN_COLS && xc >= 0 && xc < d.Wp && r0 >= 0 && (DMA ? r0 + ROWS <= d.Hp : r0 < d.Hp));
    if constexpr (DMA) {       // the launcher's choice: the table is at least a window column tall
      // scalar base + this lane's 16 bytes: no vector address arithmetic next to the accumulators
      const char* sbase = tbl + ((size_t)__builtin_amdgcn_readfirstlane(xc) * d.Hp + __builtin_amdgcn_readfirstlane(r0)) * 4;
      glds16(sbase + lane16, win + (c * PITCH) * 4);
      if constexpr (X3) glds16(sbase + tbl_plane + lane16, win + L::WIN_PLANE + (c * PITCH) * 4);
    } else {
      const int rr = r0 + 4 * lane;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) {
        const char* src = tbl + pl * tbl_plane + ((size_t)xc * d.Hp + rr) * 4;
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (rr + k < d.Hp) v[k] = *reinterpret_cast<const uint32_t*>(src + 4 * k);
        *reinterpret_cast<u32x4*>(win + pl * L::WIN_PLANE + (c * PITCH) * 4 + lane * 16) = v;
      }
    }
  };
  auto fill_share = [&](const int* fd, char* win, int nfill) {
    for (int c = wave; c < nfill; c += n_wave) fill_one(win, c, fd[2 * c], fd[2 * c + 1]);
  };

  // the W images of both buffers: zero once; the producer rewrites the dwords the keys own every emission
  for (int i = tid; i < 2 * L::W_BYTES / 16; i += (int)blockDim.x)
    *reinterpret_cast<u32x4*>(smem + (i / (L::W_BYTES / 16)) * L::BUF + L::OFF_W + (i % (L::W_BYTES / 16)) * 16) =
        u32x4{0u, 0u, 0u, 0u};       // ordered before the first use by the prologue's barrier
  if (wave == n_wave - 1) {
    // ---- producer ------------------------------------------------------------------------------------------
    __builtin_amdgcn_s_setprio(3);
    const int pg = prob * d.groups + hd / (d.heads / d.groups);
    const KeyW* kws = reinterpret_cast<const KeyW*>(key_ws) + (size_t)pg * d.Np;
    const StepBox* box = reinterpret_cast<const StepBox*>(key_ws + key_ws_box_offset(d)) + (size_t)pg * (d.Np / 32);
    const char* Kp = K + (size_t)ph * d.Np * ROWB;
    const char* Vp = V + (size_t)ph * d.Np * ROWB;
    const int n_steps = d.Np / GT;

    // One emission: the keys `sel` of a 64-key step, their weights and window addresses, and the fill list of its window
    // (this lane's entry).  The producer DESCRIBES one emission ahead of the one it stages (the fill list of window e + 1
    // travels with emission e) and stages one emission ahead of the row-block waves.
    struct Em {
      unsigned long long sel;
      int step, nfill, fd_xc, fd_r0, koff;
      u32x2 w[NP];      // the packed weights of the key's two columns, per image
    };
    int step = -1;
    unsigned long long rem = 0ull;
    const int kl = lane & (GT - 1);      // this lane's key of a step (GT = 32: the upper half wave duplicates the lower)
    const bool klane = lane < GT;
    KeyW kw_n = kws[kl];
    StepBox sb0_n = box[0], sb1_n = box[NT - 1];
    int ar = 0, xc = 0, x0 = 0, a0w = 0, cols = 0;
    bool fits = false;
    u32x2 w_t[NP];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) w_t[pl] = u32x2{0u, 0u};
    auto advance = [&](Em& em) -> bool {
      while (rem == 0ull) {      // on to the next step with live keys
        if (++step >= n_steps) return false;
        const KeyW kw = kw_n;
        const StepBox sb = box_union(sb0_n, sb1_n);
        if (step + 1 < n_steps) {
          kw_n = kws[(size_t)(step + 1) * GT + kl];
          sb0_n = box[NT * (step + 1)];
          sb1_n = box[NT * (step + 1) + NT - 1];
        }
        if (sb.amax < sb.amin) continue;               // a step of padding only
        const bool live = klane && step * GT + kl < d.N;
        ar = (kw.aoff >> 3) - d.x_off * d.Hp;          // padded table row of tap (y, .) for BEV row 0
        if constexpr (BAND) ar += row0;                // ... for the band's first BEV row
        const float tx = jrx + kw.b;
        const float xf = floorf(tx);
        xc = (int)xf + d.x_off;                        // padded table column of tap (., x)
        const float fx = tx - xf, fy = kw.fy;
        if constexpr (X3) {
          TAP_SPLIT2((1.0f - fx) * (1.0f - fy), (1.0f - fx) * fy, w_t[0][0], w_t[NP - 1][0]);
          TAP_SPLIT2(fx * (1.0f - fy), fx * fy, w_t[0][1], w_t[NP - 1][1]);
        } else {
          w_t[0][0] = H16::pack2((1.0f - fx) * (1.0f - fy), (1.0f - fx) * fy);
          w_t[0][1] = H16::pack2(fx * (1.0f - fy), fx * fy);
        }
        // the step's box: columns [x0, x1], rows [a0, a0 + rspan)
        x0 = (int)floorf(jrx + sb.bmin) + d.x_off;
        const int x1 = (int)floorf(jrx + sb.bmax) + 1 + d.x_off;
        cols = x1 - x0 + 1;
        fits = cols <= WIN_COLS && sb.amax - sb.amin + rows_q + 1 <= ROWS;
        a0w = max(0, min(sb.amin + d.y_off + (BAND ? row0 : 0), d.Hp - ROWS));
        rem = __ballot(live);
      }
      em.w[0] = w_t[0];
      if constexpr (X3) em.w[NP - 1] = w_t[NP - 1];
      em.step = step;
      if (fits) {
        em.sel = rem;
        em.koff = ((xc - x0) * PITCH + (ar - a0w)) * 4;
        em.nfill = cols;
        em.fd_xc = x0 + lane;
        em.fd_r0 = a0w;
      } else {
        // the first STRIP_KEYS remaining keys, one two-column strip each: entries 2 rank + {0, 1}
        const int rank = __builtin_popcountll(rem & ((1ull << kl) - 1ull));
        const bool mine = klane && (rem >> kl & 1ull) && rank < STRIP_KEYS;
        em.sel = __ballot(mine);
        const int akw = max(0, min(ar, d.Hp - ROWS));
        em.koff = (2 * rank * PITCH + (ar - akw)) * 4;
        em.nfill = 2 * __builtin_popcountll(em.sel);
        // lane 2 r + c holds the entry of the key with rank r: fetch that key's (xc, akw)
        int src = 0;
        {
          unsigned long long t = em.sel;
          for (int k = 0; k < (lane >> 1) && t; ++k) t &= t - 1;
          src = t ? __builtin_ctzll(t) : 0;
        }
        em.fd_xc = __shfl(xc, src) + (lane & 1);
        em.fd_r0 = __shfl(akw, src);
      }
      rem &= ~em.sel;
      return true;
    };
    // Staging of emission e (one emission ahead of its use).  K / V rows go global -> LDS directly (8 x 1 KB, no
    // registers): K with its 16-byte chunks XOR-swizzled (conflict-free fragment reads of unpadded 64-byte rows), V as two
    // [key][16 channel] images.
    auto stage = [&](const Em& em, int e, const Em* nxt) {
      char* bb = smem + (e & 1) * L::BUF;
      const size_t n0 = (size_t)em.step * GT;
#pragma unroll
      for (int i = 0; i < GT / 16; ++i) {      // keys 16 i .. 16 i + 15: lane = (key, position)
        const int n = 16 * i + (lane >> 2), c = (lane & 3) ^ ((n >> 2) & 3);
        if constexpr (X3) {      // elements 8 c .. 8 c + 7 of the split row: half c >> 1, chunk c & 1; the lo parts 32 bytes on
          const char* src = Kp + (n0 + n) * ROWB + 64 * (c >> 1) + 16 * (c & 1);
          glds16(src, bb + L::OFF_K + i * 1024);
          glds16(src + 32, bb + L::OFF_K + L::K_IMG + i * 1024);
        } else {
          glds16(Kp + (n0 + n) * 64 + 16 * c, bb + L::OFF_K + i * 1024);
        }
      }
#pragma unroll
      for (int i = 0; i < NT; ++i) {           // keys 32 i .. 32 i + 31: lane = (key, 16-byte half of the 16 channels)
        const int n = 32 * i + (lane >> 1);
        if constexpr (X3) {      // a split row: hi(ch 0..15) | lo(ch 0..15) | hi(ch 16..31) | lo(ch 16..31), 32 bytes each
          const char* src = Vp + (n0 + n) * ROWB + 16 * (lane & 1);
          glds16(src, bb + L::OFF_VLO + i * 1024);
          glds16(src + 32, bb + L::OFF_VLO + L::V_IMG + i * 1024);
          glds16(src + 64, bb + L::OFF_VHI + i * 1024);
          glds16(src + 96, bb + L::OFF_VHI + L::V_IMG + i * 1024);
        } else {
          glds16(Vp + (n0 + n) * 64 + 16 * (lane & 1), bb + L::OFF_VLO + i * 1024);
          glds16(Vp + (n0 + n) * 64 + 32 + 16 * (lane & 1), bb + L::OFF_VHI + i * 1024);
        }
      }
      if (klane) {
        char* wk = bb + L::OFF_W + (kl >> 4) * 2048 + w_image_pos(kl & 15);
        *reinterpret_cast<uint32_t*>(wk) = em.w[0][0];
        *reinterpret_cast<uint32_t*>(wk + 256) = em.w[0][1];
        if constexpr (X3) {
          *reinterpret_cast<uint32_t*>(wk + L::W_IMG) = em.w[NP - 1][0];
          *reinterpret_cast<uint32_t*>(wk + L::W_IMG + 256) = em.w[NP - 1][1];
        }
        // a key outside the emission: any address inside the window (its logit is masked)
        const bool in = em.sel >> kl & 1ull;
        *reinterpret_cast<unsigned*>(bb + L::OFF_OFF + kl * 4) = smem_base + L::OFF_WIN + (e & 1) * L::WIN + (in ? em.koff : 0);
      }
      if (nxt && lane < nxt->nfill) {
        int* fd = reinterpret_cast<int*>(bb + L::OFF_FD);
        fd[2 * lane] = nxt->fd_xc;
        fd[2 * lane + 1] = nxt->fd_r0;
      }
#if BEVR_DROP
      static_assert(NT == 1, "the third dword (live keys 32..63) carries the emission's first key index");
      if (lane == 0)
        *reinterpret_cast<u32x4*>(bb + L::OFF_CT) =
            u32x4{0u, (unsigned)em.sel, (unsigned)(em.step * GT), nxt ? (unsigned)nxt->nfill : 0u};
#else
      if (lane == 0)
        *reinterpret_cast<u32x4*>(bb + L::OFF_CT) =
            u32x4{0u, (unsigned)em.sel, (unsigned)(em.sel >> 32), nxt ? (unsigned)nxt->nfill : 0u};
#endif
    };

    Em cur, nxt;
    advance(cur);       // N >= 1: there is a first emission
    bool more = advance(nxt);
    {                   // prologue: the fill list of window 0 travels in buffer 1; emission 0 is staged
      int* fd = reinterpret_cast<int*>(smem + L::BUF + L::OFF_FD);
      if (lane < cur.nfill) {
        fd[2 * lane] = cur.fd_xc;
        fd[2 * lane + 1] = cur.fd_r0;
      }
      if (lane == 0) *reinterpret_cast<u32x4*>(smem + L::BUF + L::OFF_CT) = u32x4{0u, 0u, 0u, (unsigned)cur.nfill};
      barrier_lds();
      fill_share(fd, smem + L::OFF_WIN, cur.nfill);
      stage(cur, 0, more ? &nxt : nullptr);
      wait_vm0();
    }
    PROF_ACC(8);
    // iteration e: the row-block waves work on emission e; the producer stages emission e + 1 (`nxt`), fills its share of
    // window e + 1 and describes emission e + 2
    for (int e = 0;; ++e) {
      PROF_T_FREE(p0);
      barrier_lds();      // emission e and window e are complete; buffer / window (e + 1) & 1 are free
      PROF_T_FREE(p1);
      if (!more) {
        if (lane == 0) *reinterpret_cast<u32x4*>(smem + ((e + 1) & 1) * L::BUF + L::OFF_CT) = u32x4{4u, 0u, 0u, 0u};
        barrier_lds();
        break;
      }
      cur = nxt;          // emission e + 1
      {                   // the producer's columns of window e + 1; the fill list comes out of the lanes' registers
        char* wn = smem + L::OFF_WIN + ((e + 1) & 1) * L::WIN;
        for (int c = wave; c < cur.nfill; c += n_wave)
          fill_one(wn, c, __builtin_amdgcn_readlane(cur.fd_xc, c), __builtin_amdgcn_readlane(cur.fd_r0, c));
      }
      PROF_T_FREE(p2);
      more = advance(nxt);
      stage(cur, e + 1, more ? &nxt : nullptr);
      PROF_T_FREE(p3);
      wait_vm0();         // the K / V rows and the window columns have landed
      PROF_T_FREE(p4);
      PROF_ADD(4, p1 - p0);
      PROF_ADD(6, p2 - p1);
      PROF_ADD(1, p3 - p2);
      PROF_ADD(3, p4 - p3);
      PROF_ADD(5, 1);
    }
    PROF_FLUSH(gather, 0, lane == 0);
    return;
  }

  // ---- row-block waves --------------------------------------------------------------------------------------
  const int blk0 = wave * NB;
  const int qb = prob / d.q_div;
  TapOp<NP> qf[NB];       // B operand of QK^T: Q[q][8 kg ..]
  f32x4 o_lo[NB], o_hi[NB];
  f32x4 negm[NB];         // minus the softmax reference: the accumulator start of every logit product
  f32x4 lacc[NB];         // row sum: a product of the ROUNDED weights with a ones operand (every register the same sum):
                          // O / l is then exact where one key dominates -- the backward's delta = dO . O relies on it
  float pmx[NB];          // the largest weight
#if BEVR_DROP
  uint32_t hrow[NB];      // the row part of the keep hash, out of the emission loop
#endif
  // byte offset of the lane's BEV row (first block) in ITS window column: k-groups 0, 2 read a key's column x, k-groups
  // 1, 3 column x + 1.  The second block's rows are QB dwords further: one ds_read2_b32 serves both blocks.
  const unsigned qoff0 = (unsigned)(blk0 * QB + li) * 4u + (unsigned)(kg & 1) * (PITCH * 4u);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int row = (BAND ? row0 : 0) + min(blk0 + nb, nblk - 1) * QB + li;
    const size_t mcol = (size_t)j * d.Sp + row;
    if constexpr (X3)      // elements 8 kg .. 8 kg + 7 of the split row, the lo parts 32 bytes behind the hi parts
      qf[nb] = tap_ld<NP>(Q + (((size_t)qb * d.heads + hd) * Mp + mcol) * ROWB + 64 * (kg >> 1) + 16 * (kg & 1), 32);
    else
      qf[nb].p[0] = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const u32x4*>(Q + ((((size_t)qb * d.heads + hd) * Mp + mcol) * 32 + 8 * kg) * 2));
    o_lo[nb] = o_hi[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float mr = EXACT ? 0.f : mref[(size_t)ph * Mp + mcol];
    negm[nb] = f32x4{-mr, -mr, -mr, -mr};
    lacc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    pmx[nb] = 0.f;
#if BEVR_DROP
    hrow[nb] = bevr_drop_row(drop_seed, (uint32_t)ph, (uint32_t)mcol);      // mq = j Sp + the absolute BEV row
#endif
  }
  const uint32_t one2 = H16::pack2(1.0f, 1.0f);
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{one2, one2, one2, one2});
  const int t_off = (4 * kg + (li >> 2)) * 32 + (lane & 3) * 8;      // transposed reads of a [key][16] image
  const int k_off = li * 64 + 16 * (kg ^ (li >> 2));                 // this lane's K fragment in a 16-key block
  typedef const uint32_t __attribute__((address_space(3)))* lds_u32p;
  typedef const volatile uint32_t __attribute__((address_space(3)))* vlds_u32p;

  {   // prologue: window 0
    barrier_lds();
    const int nf0 = __builtin_amdgcn_readfirstlane((int)reinterpret_cast<const u32x4*>(smem + L::BUF + L::OFF_CT)[0][3]);
    fill_share(reinterpret_cast<const int*>(smem + L::BUF + L::OFF_FD), smem + L::OFF_WIN, nf0);
    wait_vm0();
  }
  bool first = true;      // EXACT only
  PROF_ACC(8);
  PROF_T_FREE(cprev);
  // the sweep over the emissions, instantiated for the distance (dwords) from the first block's window rows to the
  // second's: QB, or 0 for the wave whose second block lies past the column (it leaves that block out)
  auto sweep = [&](auto off1_c) {
  constexpr int OFF1 = decltype(off1_c)::value;
  constexpr int NBX = (NB == 2 && OFF1 == 0) ? 1 : NB;      // that wave works on its one block only
  for (int e = 0;; ++e) {
    PROF_T_FREE(c0);
    barrier_lds();
    PROF_T_FREE(c1);
    PROF_ADD(0, c1 - c0);
    PROF_ADD(4, c0 - cprev);
    PROF_ADD(5, 1);
    PROF_SET(cprev, c1);
    const char* bb = smem + (e & 1) * L::BUF;
    const u32x4 ct = *reinterpret_cast<const u32x4*>(bb + L::OFF_CT);
    if (__builtin_amdgcn_readfirstlane((int)ct[0]) & 4) break;
    // this wave's share of the next window: in flight during the emission's work
    fill_share(reinterpret_cast<const int*>(bb + L::OFF_FD), smem + L::OFF_WIN + ((e + 1) & 1) * L::WIN,
               __builtin_amdgcn_readfirstlane((int)ct[3]));
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      const unsigned livem = (unsigned)__builtin_amdgcn_readfirstlane((int)(t ? ct[2] : ct[1]));
      // (no shortcut for a tile or sub-tile without live keys -- strip emissions only: its keys are masked like any
      // other; every accumulator update stays unconditional, which keeps the accumulators in place)
      const TapOp<NP> vlo = tap_ld_tr<NP>(bb + L::OFF_VLO + t * 1024 + t_off, 512, L::V_IMG);
      const TapOp<NP> vhi = tap_ld_tr<NP>(bb + L::OFF_VHI + t * 1024 + t_off, 512, L::V_IMG);
      u32x4 pw[NB][NP];      // the tile's weights, packed: the B operand of PV
#if BEVR_DROP
      u32x4 km[NB];          // 0xffff over every kept weight of pw: PV contracts pw & km, the row sum all of pw
      // the key part of the hash: key n = the emission's first key + 16 s2 + 4 kg + r
      const uint32_t kh0 = ((uint32_t)__builtin_amdgcn_readfirstlane((int)ct[2]) + 4u * (uint32_t)kg) * 0xC2B2AE3Du;
#endif
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int kb = 32 * t + 16 * s2;                 // first key of the sub-tile
        const TapOp<NP> kf = tap_ld<NP>(bb + L::OFF_K + kb * 64 + k_off, L::K_IMG);
        // W as the lanes hold it (w_image_pos): two 16-byte reads, no per-lane selection
        const TapOp<NP> wa0 = tap_ld<NP>(bb + L::OFF_W + kb * 128 + lane * 16, L::W_IMG);
        const TapOp<NP> wa1 = tap_ld<NP>(bb + L::OFF_W + kb * 128 + 1024 + lane * 16, L::W_IMG);
        const int kq = 4 * (kg >> 1);
        // window addresses of keys kq .. kq + 3 (first bias product) and 8 + kq .. 8 + kq + 3 (second)
        const u32x4 oc0 = *reinterpret_cast<const u32x4*>(bb + L::OFF_OFF + (kb + kq) * 4);
        const u32x4 oc1 = *reinterpret_cast<const u32x4*>(bb + L::OFF_OFF + (kb + 8 + kq) * 4);
        // both row blocks' logit chains first (independent: their matrix products interleave), then the weights.  A wave
        // whose second block lies past the column computes it on the clamped rows and drops it in the epilogue.
        f32x4 sv[NB];
        u32x4 g0[NB][NP], g1[NB][NP];
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
          const lds_u32p p0 = (lds_u32p)(uintptr_t)(oc0[dd] + qoff0), p1 = (lds_u32p)(uintptr_t)(oc1[dd] + qoff0);
#ifdef BEVR_DEBUG
          {      // every tap read lies inside the emission's window (the hi plane; the lo plane is the same offset in its own)
            const unsigned w0 = smem_base + L::OFF_WIN + (e & 1) * L::WIN, last = (unsigned)((NBX - 1) * OFF1) * 4u;
            BEVR_ASSERT(oc0[dd] + qoff0 >= w0 && oc0[dd] + qoff0 + last + 4u <= w0 + L::WIN_PLANE);
            BEVR_ASSERT(oc1[dd] + qoff0 >= w0 && oc1[dd] + qoff0 + last + 4u <= w0 + L::WIN_PLANE);
          }
#endif
          if constexpr (X3) {      // the lo plane: the same address, WIN_PLANE further (an immediate offset; volatile as
                                   // below: hi and lo would merge into a ds_read2st64_b32 whose pair feeds two operands)
#pragma unroll
            for (int nb = 0; nb < NBX; ++nb) {
              g0[nb][0][dd] = ((vlds_u32p)p0)[nb * OFF1];
              g1[nb][0][dd] = ((vlds_u32p)p1)[nb * OFF1];
              g0[nb][NP - 1][dd] = ((vlds_u32p)p0)[nb * OFF1 + L::WIN_PLANE / 4];
              g1[nb][NP - 1][dd] = ((vlds_u32p)p1)[nb * OFF1 + L::WIN_PLANE / 4];
            }
          } else
#pragma unroll
          for (int nb = 0; nb < NBX; ++nb) {
            // (volatile: kept from merging with the first block's read into a ds_read2_b32, whose register PAIR would have to
            // be moved apart into the two blocks' operands -- vector instructions are what this loop is short of)
            if (nb == 0) {
              g0[nb][0][dd] = p0[0];
              g1[nb][0][dd] = p1[0];
            } else {
              g0[nb][0][dd] = ((vlds_u32p)p0)[nb * OFF1];
              g1[nb][0][dd] = ((vlds_u32p)p1)[nb * OFF1];
            }
          }
        }
#pragma unroll
        for (int nb = 0; nb < NBX; ++nb) {
          sv[nb] = tap_mm<PREC>(kf, qf[nb], negm[nb]);
          sv[nb] = tap_mm<PREC>(wa0, tap_op(g0[nb]), sv[nb]);
          sv[nb] = tap_mm<PREC>(wa1, tap_op(g1[nb]), sv[nb]);
        }
        if ((livem >> (16 * s2) & 0xffffu) != 0xffffu) {      // uniform: padding keys, or a strip emission
#pragma unroll
          for (int nb = 0; nb < NBX; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (!(livem >> (16 * s2 + 4 * kg + r) & 1u)) sv[nb][r] = -1.0e30f;
        }
#pragma unroll
        for (int nb = 0; nb < NBX; ++nb) {
          if constexpr (EXACT) {
            // online reference: the maximum of the row's first keys, raised (with a rescale) when a later logit exceeds it
            const float tm = fmaxf(fmaxf(sv[nb][0], sv[nb][1]), fmaxf(sv[nb][2], sv[nb][3]));
            constexpr float RAISE_P = PREC == BEVR_PREC_F16 ? F16_RAISE : RAISE;
            if (first || __any(tm > RAISE_P)) {
              float tx = fmaxf(tm, __shfl_xor(tm, 16));
              tx = fmaxf(tx, __shfl_xor(tx, 32));
              if constexpr (PREC == BEVR_PREC_F16) tx -= F16_LIFT;
              const float delta = first ? tx : fmaxf(tx, 0.f);
              const float al = first ? 1.0f : fast_exp2(-delta);
              negm[nb] -= delta;
              o_lo[nb] *= al;
              o_hi[nb] *= al;
              lacc[nb] *= al;
              pmx[nb] *= al;
              sv[nb] -= delta;
              if (s2 == 1) {       // the first sub-tile's weights of this tile are in pw already
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                  if constexpr (X3)      // hi + lo is the weight PV contracts: rescaled and split again
                    tap_pack2<PREC>((H16::lo(pw[nb][0][k]) + H16::lo(pw[nb][NP - 1][k])) * al,
                                    (H16::hi(pw[nb][0][k]) + H16::hi(pw[nb][NP - 1][k])) * al, k, pw[nb]);
                  else
                    pw[nb][0][k] = H16::pack2(H16::lo(pw[nb][0][k]) * al, H16::hi(pw[nb][0][k]) * al);
                }
              }
            }
          }
          const f32x2 pa = {fast_exp2(sv[nb][0]), fast_exp2(sv[nb][1])}, pb2 = {fast_exp2(sv[nb][2]), fast_exp2(sv[nb][3])};
          if constexpr (X3) {
            tap_pack2<PREC>(pa[0], pa[1], 2 * s2, pw[nb]);
            tap_pack2<PREC>(pb2[0], pb2[1], 2 * s2 + 1, pw[nb]);
          } else {
            pw[nb][0][2 * s2] = H16::pack2(pa[0], pa[1]);
            pw[nb][0][2 * s2 + 1] = H16::pack2(pb2[0], pb2[1]);
          }
          pmx[nb] = fmaxf(fmaxf(fmaxf(pmx[nb], pa[0]), pa[1]), fmaxf(pb2[0], pb2[1]));
#if BEVR_DROP
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            // (n 0xC2B2AE3D is additive in n: the two keys of dword k are 16 s2 + 4 kg + 2 k + {0, 1})
            const uint32_t kn = kh0 + (uint32_t)(16 * s2 + 2 * k) * 0xC2B2AE3Du;
            const bool k0 = (bevr_drop_mix(hrow[nb] ^ kn) >> 16) >= drop_thr;
            const bool k1 = (bevr_drop_mix(hrow[nb] ^ (kn + 0xC2B2AE3Du)) >> 16) >= drop_thr;
            km[nb][2 * s2 + k] = (k0 ? 0xffffu : 0u) | (k1 ? 0xffff0000u : 0u);
          }
#endif
        }
        if constexpr (EXACT) first = false;
      }
#pragma unroll
      for (int nb = 0; nb < NBX; ++nb) {
        const TapOp<NP> pb = tap_op(pw[nb]);
#if BEVR_DROP
        const u32x4 pk[NP] = {pw[nb][0] & km[nb]};      // the kept weights (the EXACT pass rescales pw: masked after it)
        const TapOp<NP> pkb = tap_op(pk);
        o_lo[nb] = tap_mm<PREC>(vlo, pkb, o_lo[nb]);
        o_hi[nb] = tap_mm<PREC>(vhi, pkb, o_hi[nb]);
#else
        o_lo[nb] = tap_mm<PREC>(vlo, pb, o_lo[nb]);
        o_hi[nb] = tap_mm<PREC>(vhi, pb, o_hi[nb]);
#endif
        // (split mode: ones . lo + ones . hi, the f32 sum of exactly the values PV contracts)
#pragma unroll
        for (int pl = NP - 1; pl >= 0; --pl) lacc[nb] = mfma16<PREC>(ones, pb.p[pl], lacc[nb]);
      }
    }
    PROF_T_FREE(c2);
    PROF_ADD(1, c2 - c1);
    wait_vm0();
    PROF_T_FREE(c3);
    PROF_ADD(2, c3 - c2);
  }
  };
  if constexpr (NB == 2) {
    if (blk0 + 1 < nblk) sweep(IntC<QB>{});
    else sweep(IntC<0>{});
  } else {
    sweep(IntC<0>{});
  }
  PROF_FLUSH(gather, wave ? 16 : 8, lane == 0 && (wave == 0 || wave == 3));

  // ---- epilogue: O[q][16 half + 4 kg ..], the two LSE planes; flag the column if a row's mass is not a healthy number ----
  bool bad = false;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (blk0 + nb >= nblk) continue;
    const float l = lacc[nb][0];
    float pm = fmaxf(pmx[nb], __shfl_xor(pmx[nb], 16));
    pm = fmaxf(pm, __shfl_xor(pm, 32));
    const int row = (BAND ? row0 : 0) + (blk0 + nb) * QB + li;
    if (!EXACT && row < row_end && !(l >= 7.9e-31f && l < 3.0e38f)) bad = true;
    if constexpr (!EXACT && PREC == BEVR_PREC_F16) {      // the largest weight too deep in fp16's subnormals: F16_PMAX_PER_KEY
      if (row < row_end && !(pm >= (float)d.N * F16_PMAX_PER_KEY)) bad = true;
    }
    if (BAND && !to_end && row >= row_end) continue;      // rows of the next band (no shuffles below)
    // rows past the grid (zero Q rows of the last block) get their O and LSE like any other: the key-side backward
    // walks all Sp rows of a column and needs a finite LSE there; the rows no block covers take the last block's
#if BEVR_DROP
    const float inv = (65536.0f / (65536.0f - (float)drop_thr)) / l;      // the kept weights' 1 / (1 - p)
#else
    const float inv = 1.0f / l;
#endif
    const size_t mq = (size_t)ph * Mp + (size_t)j * d.Sp + row;
    float* orow = O + mq * 32;
    *reinterpret_cast<f32x4*>(orow + 4 * kg) = o_lo[nb] * inv;
    *reinterpret_cast<f32x4*>(orow + 16 + 4 * kg) = o_hi[nb] * inv;
    if (kg == 0) {
      const float lg = __log2f(l);
      const int n_copy = (to_end && blk0 + nb == nblk - 1) ? (d.Sp - row + QB - 1) / QB : 1;
      for (int k = 0; k < n_copy; ++k) {
        float lse0 = lg - negm[nb][0];
        if constexpr (BAND || PREC == BEVR_PREC_F16) {
          // A row past the grid that no block covers has Q = 0 -- its logits are the bias alone -- but carries the LSE of a
          // REAL row: the key-side backward forms P = 2^(bias - LSE) there (times 0).  A real row whose logits all lie far
          // under the bias (activations that explode along a recurrence) would make that P overflow: the copy is kept
          // PAD_FLOOR binades over the padding row's own reference (an upper bound of its logits minus the headroom), which
          // no row of ordinary size comes near in bf16; in fp16 P becomes an fp16 operand scaled for the launch's largest
          // weight (>= 2^-60, grad_scale), so there the copy is put where P vanishes against any such scale.
          constexpr float PAD_FLOOR = PREC == BEVR_PREC_F16 ? 70.0f : -36.0f;
          if (k > 0) lse0 = fmaxf(lse0, mref[mq + k * QB] + PAD_FLOOR);
        }
        LSE[mq + k * QB] = lse0;
        // plane 1: log2 of the row's largest softmax weight
        LSE[(size_t)n_ph * Mp + mq + k * QB] = __log2f(pm) - lg;
      }
    }
  }
  if constexpr (!EXACT) {
    if (__any(bad) && lane == 0) flags[ph * d.S + j] = 1;
  }
}

// BEVR_GATHER_ROWS: the rows [row0, row0 + n_rows) of every column; else the whole column (row0, n_rows unused).
template <int PREC>
int launch(const bevr_attn_desc& d, const void* Q, const void* K, const void* V, const void* key_ws,
           const void* table_pk, const float* mref, float* O, float* LSE, int* flags, int row0, int n_rows,
           hipStream_t st BEVR_DROP_PARAMS) {
  typedef LdsG L;
  const int n_ph = d.n_prob * d.heads;
  const int grid = ((n_ph + 7) / 8) * 8 * d.S;
  const int nblk = ((BEVR_GATHER_ROWS ? n_rows : d.S) + QB - 1) / QB;
  // a key's taps for all BEV rows of a column (of a band) must fit one window column
  if (nblk * QB + 1 > ROWS || nblk > 14) return BEVR_E_SHAPE;
  const int nb = nblk <= 7 ? 1 : 2;      // row blocks per wave: at most 7 row-block waves + the producer
  const int n_cw = (nblk + nb - 1) / nb;
  const dim3 block(64 * (n_cw + 1));
#if BEVR_DROP
#define BEVR_GATHER_ROW_ARGS , row0, n_rows, drop_thr, drop_seed
#elif BEVR_GATHER_ROWS
#define BEVR_GATHER_ROW_ARGS , row0, n_rows
#else
#define BEVR_GATHER_ROW_ARGS
#endif
#define BEVR_GATHER_LAUNCH_(NB_, EX_, DMA_)                                                                          \
  hipLaunchKernelGGL((BEVR_GATHER_KERNEL<PREC, NB_, EX_, DMA_>), dim3(grid), block, L::TOTAL, st, d,                \
                     (const char*)Q, (const char*)K, (const char*)V, (const char*)key_ws, (const uint32_t*)table_pk, \
                     mref, O, LSE, flags BEVR_GATHER_ROW_ARGS)
#if BEVR_GATHER_X3
  // more than 64 KB of dynamic LDS: the limit is raised per kernel and per device
#define BEVR_GATHER_LAUNCH(NB_, EX_, DMA_)                                                                           \
  do {                                                                                                               \
    const int ea = bevr_raise_dynamic_lds<&BEVR_GATHER_KERNEL<PREC, NB_, EX_, DMA_>>(L::TOTAL);                      \
    if (ea) return ea;                                                                                               \
    BEVR_GATHER_LAUNCH_(NB_, EX_, DMA_);                                                                             \
  } while (0)
#else
#define BEVR_GATHER_LAUNCH(NB_, EX_, DMA_) BEVR_GATHER_LAUNCH_(NB_, EX_, DMA_)
#endif
  const bool dma = d.Hp >= ROWS;        // else (small problems): the window columns are copied through registers
  for (int ex = 0; ex < 2; ++ex) {       // static reference, then the exact pass over the flagged columns
    if (nb == 1) {
      if (dma) { if (ex) BEVR_GATHER_LAUNCH(1, true, true); else BEVR_GATHER_LAUNCH(1, false, true); }
      else { if (ex) BEVR_GATHER_LAUNCH(1, true, false); else BEVR_GATHER_LAUNCH(1, false, false); }
    } else {
      if (dma) { if (ex) BEVR_GATHER_LAUNCH(2, true, true); else BEVR_GATHER_LAUNCH(2, false, true); }
      else { if (ex) BEVR_GATHER_LAUNCH(2, true, false); else BEVR_GATHER_LAUNCH(2, false, false); }
    }
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
#undef BEVR_GATHER_LAUNCH
#undef BEVR_GATHER_LAUNCH_
  return BEVR_OK;
}

// The contract of the three gather entry points.  PRECS: the modes this translation unit holds the kernels of.
template <int... PRECS>
int run(const bevr_attn_desc* d, const void* Q, const void* K, const void* V, const void* key_ws, const void* table_pk,
        const float* mref, float* O, float* LSE, int* flags, int row0, int n_rows, void* stream BEVR_DROP_PARAMS) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!Q || !K || !V || !key_ws || !table_pk || !mref || !O || !LSE || !flags) return BEVR_E_NULL;
  if (!bevr_aligned16(Q) || !bevr_aligned16(K) || !bevr_aligned16(V) || !bevr_aligned16(O) || !bevr_aligned16(key_ws))
    return BEVR_E_ALIGN;
  return bevr_for_precision<PRECS...>(d->precision, [&](auto P) {
    // a row range is checked after the precision: it starts on a row block and fits the column and one launch
    if (BEVR_GATHER_ROWS && (row0 < 0 || row0 % QB != 0 || n_rows < 1 || n_rows > 14 * QB || n_rows > d->S - row0))
      return (int)BEVR_E_SHAPE;
    return launch<P()>(*d, Q, K, V, key_ws, table_pk, mref, O, LSE, flags, row0, n_rows, (hipStream_t)stream BEVR_DROP_ARGS);
  });
}

}  // namespace

#if BEVR_DROP
extern "C" int bevr_attn_gather_fwd_dropout(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                                            const void* key_ws, const void* table_pk, const float* mref, float* O,
                                            float* LSE, int* flags, int row0, int n_rows, unsigned drop_thr,
                                            unsigned drop_seed, void* stream) {
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, Q, K, V, key_ws, table_pk, mref, O, LSE, flags, row0, n_rows, stream,
                                            drop_thr, drop_seed);
}
#elif BEVR_GATHER_X3
extern "C" int bevr_attn_gather_fwd_x3(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                                       const void* key_ws, const void* table_pk2, const float* mref, float* O,
                                       float* LSE, int* flags, int row0, int n_rows, void* stream) {
  return run<BEVR_PREC_BF16X3>(d, Q, K, V, key_ws, table_pk2, mref, O, LSE, flags, row0, n_rows, stream);
}
#elif BEVR_GATHER_ROWS
extern "C" int bevr_attn_gather_fwd_rows(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                                         const void* key_ws, const void* table_pk, const float* mref, float* O,
                                         float* LSE, int* flags, int row0, int n_rows, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, Q, K, V, key_ws, table_pk, mref, O, LSE, flags, row0, n_rows, stream);
}
#else
extern "C" int bevr_attn_gather_fwd(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                                    const void* key_ws, const void* table_pk, const float* mref, float* O, float* LSE,
                                    int* flags, void* stream) {
  return run<BEVR_PREC_BF16, BEVR_PREC_F16>(d, Q, K, V, key_ws, table_pk, mref, O, LSE, flags, 0, 0, stream);
}
#endif
