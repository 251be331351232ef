// Attention backward, query side (dQ and the rpe-table gradient), SLAB-STATIONARY: bevr_attn_slab_bwd_q.
//
// Same arithmetic per (query, key) pair as attn_bwd_q.hip (reference model/SCA_deform_attn.py:331-413,
// model/TSA_deform_attn.py:245-333 differentiated):  S^T[key][query] tiles with the query on the lane, P = exp2(S - LSE),
// dS = P (dP - delta), dQ += dS K, and the table gradient of the pair's four bilinear taps as two pre-summed 64-bit
// fixed-point LDS adds per key row -- but the work is cut along the TABLE instead of along the queries:
//
//   a work item owns a SLAB of `sw` consecutive table columns [x0, x0 + sw) of one (problem, head) -- ALL rows of them: the
//   table values (16-bit pairs) and the gradient cells of columns x0 .. x0 + sw (the right tap of the last owned column)
//   sit in LDS for the whole item -- and processes exactly the pairs whose LEFT tap column X = floor(j rx + b_n) lies in
//   the slab.  With the keys of a problem sorted by b, the keys that meet that for BEV column j are one contiguous run
//   [kbeg, kend) of the sorted list, sliding by rx keys' worth per column (bevr_attn_slab_prep finds the runs).
//
// What that buys over the query-tile kernel (attn_bwd_q.hip: a (31 x 8)-query tile with a table window that MOVES with
// the keys, 0.33-0.48 moves per 64-key step, 93 GB of flush atomics per launch at the benchmark):
//   * no window logic at all: no region moves, refills, dirty boxes, grouped passes or global-memory path; any key set
//     runs at the same speed;
//   * every table cell leaves the workgroup ONCE per (item): the flush is ~(sw + 1) x rows floats per item, < 1 GB per
//     launch; what goes to memory instead is the slab's share of dQ, one float atomic per (query, channel) and
//     (slab, column) -- 2 S S 128 B x n_slab per (problem, head);
//   * 7 worker waves, one per row block of 31 queries, each running BOTH 32-key halves of a 64-key emission as two
//     interleaved dependency chains (8 waves per CU = 256 registers per wave: no spills; the first version, 14 workers of
//     one half each at 128 registers, reloaded spilled fragments from scratch on every emission and needed an exchange
//     to sum the two halves' dQ), and the staging, the per-(column, key) constants and the key bookkeeping on a PRODUCER
//     wave, one emission ahead: one barrier per emission, no staging registers in the workers.
// The price: K and V are re-streamed per slab (every pair belongs to one slab, every key to ~S sw / (Wt / rx) of them),
// and a workgroup is the whole CU (~150 KB of LDS).
//
// Work distribution: bevr_attn_slab_prep lists the non-empty (problem-head, slab, column chunk) items; the kernel is
// PERSISTENT, one workgroup per CU, items handed out by an atomic counter (every wave reaches the exit: the counter only
// grows and the list is finite).
//
// Rows.  Window row w of a slab column holds the pair (T2[w - ROW0], T2[w - ROW0 + 1]) of that table column;
// R = ROW0 + S + PADR + 31 n_rb + 2 rows cover every key with floor(a) in [-ROW0, S - 1 + PADR] for every row block
// (ROW0 = 10, PADR = 8: the learned offsets move a key ~3 rows past the table's ends).  A 32-key half with a key outside
// that range takes the CLAMPED body: the row index is clamped into the window, whose first and last rows lie outside the
// real table (zero values, gradient discarded), exactly as the zero padding of the global table.
//
// This header is the formulation's shared part, included by the two files that hold a kernel body and by nothing else:
// the constants, the workspace, the preparation kernels, the kernel's signature, the scaffold of a body (LDS carve-up,
// work items, slab fill and flush, the producer's run iterator, the control word between producer and workers), the
// launch and the entry points.  attn_slab_bwd_q.hip holds the 16-bit body, attn_slab_bwd_q_x3.hip (BEVR_SLAB_X3 = 1) the
// split-bf16 body (BEVR_PREC_BF16X3); each is compiled three times, as it stands and through two stub units that set one
// of the switches below -- translation units of their own, so that one kernel's registers do not depend on another's:
//
// BEVR_SLAB_ROWS = 1 (attn_slab_bwd_q_rows.hip, attn_slab_bwd_q_x3_rows.hip): S <= 448, where the one-band kernels stop at
// 211.  The window keeps its FULL height -- every table row the whole column can reach, R from the same formula -- at one
// of two taller row pitches (a template parameter: the pitch stays a compile-time multiple of 64; split-bf16: 7 and 6
// owned columns of 16-byte cells), and a launch covers a BAND of at most SNRB row blocks: worker wave w owns row block
// row0 / 31 + w.  Nothing else changes: a pair's window row is A + ROW0 + i whichever band i lies in, so the indexing and
// the clamping argument are the ones above (a window cut to the band's rows would clamp a key with A = -15 seen from row
// 217 onto the wrong, non-zero, row).  The entry points are bevr_attn_slab_rows_ws_bytes / _slab_rows_prep /
// bevr_attn_slab_bwd_q_rows and bevr_attn_slab_x3_rows_ws_bytes / _slab_x3_rows_prep / bevr_attn_slab_bwd_q_x3_rows.  No
// keep mask on either band kernel.
//
// BEVR_DROP = 1 (attn_slab_bwd_q_drop.hip, attn_slab_bwd_q_x3_drop.hip): attention dropout on the one-band kernels, the
// arithmetic of bevr_attn_bwd_q_dropout: dS = P (keep ? D dP - delta : -delta), one FMA per pair on the dP accumulator
// (which starts at -delta).  The keys arrive SORTED by b and the mask is a function of the key's index in the caller's
// order: these units' preparation (bevr_attn_slab_drop_prep, bevr_attn_slab_x3_drop_prep) writes that index into
// SlabKey::pad, the producer stages index x 0xC2B2AE3D per emission beside the constants, and the key-row loops take it by
// DPP as they take those.  The entry points are bevr_attn_slab_drop_ws_bytes / _slab_drop_prep /
// bevr_attn_slab_bwd_q_dropout and bevr_attn_slab_x3_drop_ws_bytes / _slab_x3_drop_prep / bevr_attn_slab_bwd_q_x3_dropout.
#pragma once
#ifndef BEVR_SLAB_ROWS
#define BEVR_SLAB_ROWS 0
#endif
#ifndef BEVR_SLAB_X3
#define BEVR_SLAB_X3 0
#endif
#include "attn_tile.h"
#include "attn_tap.h"
#include "attn_host.h"

#include "bevr_prof.h"

namespace {

constexpr int SLAB_W_MAX = 24;     // owned table columns per slab (fewer when the rows of a large S leave less room)
constexpr int SLAB_ROW0 = 10;      // window row of table row 0
constexpr int SLAB_PADR = 8;       // rows past the table's last key row covered without clamping
constexpr int SLAB_RP = 448;       // row PITCH of a slab column in entries: 7 x 64, so that the two taps of a pair are ONE
                                   // ds_read2st64_b32 and the two gradient adds share an address register (S <= 211)
constexpr int SLAB_CH = 25;        // BEV columns per work item
constexpr int SQROWS = 31;         // query rows per row block (lane 31 of a half: the 32nd table row, attn_bwd_q.hip)
constexpr int SNRB = 7;            // row blocks per column (S <= 217) -- BEVR_SLAB_ROWS: per launch (a band of the column)
constexpr int SNWORK = SNRB;       // worker waves: one per row block, BOTH 32-key halves of an emission each
constexpr int STHREADS = (SNWORK + 1) * 64;   // 8 waves = 2 per SIMD: 256 registers per wave (see the kernel)
constexpr int SEK = 64;            // keys per emission
#if BEVR_SLAB_X3
constexpr int SKROW = 128;         // split-mode rows, unpadded: their 16-byte chunks are swizzled (attn_slab_bwd_q_x3.hip)
constexpr int SLAB_CELL = 16;      // bytes per table cell in LDS: the f32 pair (T[y], T[y+1]) and the 64-bit gradient cell
#else
constexpr int SKROW = 80;          // bytes per staged K / V row (64 + 16: conflict-free fragment reads)
constexpr int SLAB_CELL = 12;      // bytes per table cell in LDS: the 16-bit pair and the 64-bit gradient cell
#endif
constexpr float SLAB_EPS = 0.02f;  // slack of the key runs (in table columns): the kernel's own floor() decides membership

// per key, in the problem's b-sorted order (bevr_attn_slab_prep)
struct SlabKey { int A; float fy; float b; int pad; };

// per-(column, key) constants of an emission, written by the producer (lane = key); a worker lane reads ONE record per
// half and the key-row loop takes its constants from those registers by DPP (process)
#if BEVR_SLAB_X3
struct SlabCK {
  float w00, w01, w10, w11;   // tap weights (1-fx)(1-fy), (1-fx)fy, fx(1-fy), fx fy in f32, as the region kernel's f32 layout
  int cell;                   // BYTE offset of the key's first tap's value entry (8-byte entries) for window row offset 0
  int row;                    // its row part, A + ROW0 (the clamped body separates the two)
  int pad0, pad1;
};
#else
struct SlabCK {
  unsigned wA, wB;   // tap weights of column X / X + 1 as packed 16-bit pairs (row y, row y + 1)
  int cell;          // window index of the key's first tap for window row offset 0: colbase + row
  int row;           // its row part, A + ROW0 (the clamped body separates the two)
};
#endif

struct SlabLds {
  static constexpr int K_BYTES = SEK * SKROW;
  static constexpr int OFF_V = K_BYTES;
  static constexpr int OFF_CK = 2 * K_BYTES;
  static constexpr int OFF_CT = OFF_CK + SEK * (int)sizeof(SlabCK);     // 2 x u32x4: {flags, j, amin0, amax0}, {amin1, amax1, 0, 0}
#if BEVR_DROP
  static constexpr int OFF_KN = OFF_CT + 32;      // [SEK] u32: the key part of the keep hash, (ORIGINAL key index) 0xC2B2AE3D
  static constexpr int BUF = OFF_KN + SEK * 4;
#else
  static constexpr int BUF = OFF_CT + 32;
#endif
};
enum { SF_DONE = 1, SF_FIRST = 2, SF_LAST = 4 };

__host__ __device__ inline int slab_n_rb(int S) { return (S + SQROWS - 1) / SQROWS; }
__host__ __device__ inline int slab_rows(int S) { return SLAB_ROW0 + S + SLAB_PADR + SQROWS * slab_n_rb(S) + 2; }
// columns in LDS: column 0 is the KILL column (values -big, masked keys point there; its right neighbour is a real column,
// read with weight 0), columns 1 .. sw + 1 the slab's sw owned columns and the right tap column of the last one
__host__ __device__ inline size_t slab_lds_bytes(int S, int sw, int rp = SLAB_RP) {
  return (size_t)(sw + 2) * rp * SLAB_CELL + 2 * SlabLds::BUF + 64;
}
__host__ __device__ inline int slab_width(int S, int rp = SLAB_RP) {
  int sw = SLAB_W_MAX;
  while (sw > 1 && slab_lds_bytes(S, sw, rp) > 160 * 1024) --sw;
  return sw;
}
#if BEVR_SLAB_ROWS
// the two tall pitches (13 x 64, 15 x 64): 832 holds the 826 rows of S = 403 at sw = 12 (162 432 B of LDS), 960 the 933
// rows of S = 448 at sw = 10 (160 896 B)
constexpr int SLAB_RP_A = 832, SLAB_RP_B = 960;
constexpr int SLAB_ROWS_MAX_S = 448;
constexpr int SLAB_BAND_ROWS = SNRB * SQROWS;      // 217
__host__ __device__ inline int slab_pitch(int S) { return slab_rows(S) <= SLAB_RP_A ? SLAB_RP_A : SLAB_RP_B; }
#else
__host__ __device__ inline int slab_pitch(int S) { return SLAB_RP; }
#endif
#if BEVR_DROP
static_assert(!BEVR_SLAB_ROWS, "the keep mask: the one-band kernels, 16-bit and split-bf16");
#if BEVR_SLAB_X3
// split-bf16: the hash words leave the slab its 15 owned columns (17 x 448 x 16 + 2 x 18 720 + 64 = 159 360 bytes; a 16th
// would need 166 528) -- the slab width, the workspace and the work list are bevr_attn_slab_bwd_q_x3's
static_assert((15 + 2) * SLAB_RP * SLAB_CELL + 2 * SlabLds::BUF + 64 <= 160 * 1024 &&
              (16 + 2) * SLAB_RP * SLAB_CELL + 2 * (SlabLds::BUF - SEK * 4) + 64 > 160 * 1024, "15 columns with and without the mask");
#else
// the widest slab with the staged hash words beside OFF_CK: the workgroup is still the CU's 160 KB
static_assert((SLAB_W_MAX + 2) * SLAB_RP * SLAB_CELL + 2 * SlabLds::BUF + 64 <= 160 * 1024, "160 KB of LDS");
#endif
#endif
// first table column any slab has to cover and the number of slabs: X = floor(j rx + b), b clamped as the key prep does
__host__ __device__ inline int slab_xmin(const bevr_attn_desc& d) { return -(d.Wt / 2 + 2) - 1; }
__host__ __device__ inline int slab_count(const bevr_attn_desc& d, int sw) {
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const int xmax = (int)((float)(d.S - 1) * rx) + d.Wt + 3;
  return (xmax - slab_xmin(d) + sw) / sw;
}
__host__ __device__ inline int slab_chunks(int S) { return (S + SLAB_CH - 1) / SLAB_CH; }

// workspace: SlabKey[PG][N] | kbeg[PG][n_slab][S] | kend[PG][n_slab][S] | items[n_ph * n_slab * n_chunk] (int4) | counters
struct SlabWs {
  size_t off_beg, off_end, off_items, off_cnt, total;
  int n_slab, n_chunk, sw;
};
__host__ __device__ inline SlabWs slab_ws(const bevr_attn_desc& d) {
  SlabWs w;
  w.sw = slab_width(d.S, slab_pitch(d.S));
  w.n_slab = slab_count(d, w.sw);
  w.n_chunk = slab_chunks(d.S);
  const size_t pg = (size_t)d.n_prob * d.groups;
  size_t o = pg * d.N * sizeof(SlabKey);
  o = (o + 255) & ~(size_t)255;
  w.off_beg = o;
  o += pg * w.n_slab * d.S * 4;
  w.off_end = o;
  o += pg * w.n_slab * d.S * 4;
  o = (o + 255) & ~(size_t)255;
  w.off_items = o;
  o += (size_t)d.n_prob * d.heads * w.n_slab * w.n_chunk * 16;
  w.off_cnt = o;
  o += 256;
  w.total = o;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------
// preparation
__global__ __launch_bounds__(256) void slab_keys_kernel(bevr_attn_desc d, const float* __restrict__ key_a,
                                                        const float* __restrict__ key_b, const int* __restrict__ order,
                                                        SlabKey* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)d.n_prob * d.groups * d.N;
  if (t >= total) return;
  const int pg = (int)(t / d.N);
  const int n = order[t];
  const KeyClamp c = key_clamp(key_a[(size_t)pg * d.Np + n], key_b[(size_t)pg * d.Np + n], d);
  SlabKey k;
  k.A = (int)c.af;
  k.fy = c.a - c.af;
  k.b = c.b;
#if BEVR_DROP
  k.pad = n;      // the key's index in the caller's order: what the keep mask hashes
#else
  k.pad = 0;
#endif
  out[t] = k;
}

// first index in the sorted keys of `pg` whose b is >= thr
__device__ __forceinline__ int slab_lower_bound(const SlabKey* __restrict__ keys, int N, float thr) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid].b < thr) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one thread per (pg, slab, chunk): the key runs of the chunk's columns, and the chunk's work items (one per head of the
// group) if any run is non-empty
__global__ __launch_bounds__(256) void slab_ranges_kernel(bevr_attn_desc d, const SlabKey* __restrict__ keys,
                                                          int* __restrict__ kbeg, int* __restrict__ kend,
                                                          int4* __restrict__ items, int* __restrict__ cnt, int n_slab,
                                                          int n_chunk, int sw) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n_pg = d.n_prob * d.groups;
  if (t >= n_pg * n_slab * n_chunk) return;
  // chunk fastest: the items of one slab are neighbours in the list (their K / V runs overlap: L2 reuse)
  const int chunk = t % n_chunk, slab = (t / n_chunk) % n_slab, pg = t / (n_chunk * n_slab);
  const SlabKey* kp = keys + (size_t)pg * d.N;
  const float rx = (float)(d.Wt - 1) / (2.0f * (float)(d.S - 1));
  const int x0 = slab_xmin(d) + slab * sw;
  int work = 0;
  const int j1 = min(d.S, (chunk + 1) * SLAB_CH);
  for (int j = chunk * SLAB_CH; j < j1; ++j) {
    const float jrx = (float)j * rx;
    const int b0 = slab_lower_bound(kp, d.N, (float)x0 - jrx - SLAB_EPS);
    const int b1 = slab_lower_bound(kp, d.N, (float)(x0 + sw) - jrx + SLAB_EPS);
    kbeg[((size_t)pg * n_slab + slab) * d.S + j] = b0;
    kend[((size_t)pg * n_slab + slab) * d.S + j] = b1;
    work += b1 - b0;
  }
  if (work > 0) {
    const int hpg = d.heads / d.groups;
    const int prob = pg / d.groups, grp = pg % d.groups;
    const int at = atomicAdd(cnt, hpg);
    for (int h = 0; h < hpg; ++h) items[at + h] = make_int4(prob * d.heads + grp * hpg + h, slab, chunk, work);
  }
}

// LDS-only barrier is not enough here: the producer's global loads are consumed by its own LDS stores before the barrier
#define SLAB_BARRIER() __syncthreads()

// ---------------------------------------------------------------------------------------------------------------
// The kernel's signature, written once: declared here for the launch below, defined by the body file with the same macro
// (no parameter struct: the kernarg layout is part of what the body files' registers were measured with).
// BEVR_SLAB_ROWS: RP the row pitch (else SLAB_RP), row0 (a multiple of SQROWS) the first BEV row of the launch's band,
// n_rb_band <= SNRB its row blocks: worker wave w owns row block row0 / SQROWS + w of the column.
#if BEVR_SLAB_ROWS
#define SLAB_KERNEL_TEMPLATE template <int PREC, int RP>
#define SLAB_BAND_PARAMS , int row0, int n_rb_band
#define SLAB_BAND_ARGS , row0, n_rb_band
#define SLAB_KERNEL(PREC, RP) attn_slab_bwd_q_kernel<PREC, RP>
#else
#define SLAB_KERNEL_TEMPLATE template <int PREC>
#define SLAB_BAND_PARAMS
#define SLAB_BAND_ARGS
#define SLAB_KERNEL(PREC, RP) attn_slab_bwd_q_kernel<PREC>
#endif
#define SLAB_KERNEL_SIGNATURE                                                                                            \
  SLAB_KERNEL_TEMPLATE __global__ __launch_bounds__(STHREADS, 1) void attn_slab_bwd_q_kernel(                            \
      bevr_attn_desc d, const char* __restrict__ Q, const char* __restrict__ Ks, const char* __restrict__ Vs,            \
      const SlabKey* __restrict__ skeys, const int* __restrict__ kbeg, const int* __restrict__ kend,                     \
      const int4* __restrict__ items, int* __restrict__ cnt, const char* __restrict__ table_pair,                        \
      const char* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ delta,                       \
      const float* __restrict__ grad_scale, float* __restrict__ dQ, float* __restrict__ dtable, int n_slab, int sw, int R \
      BEVR_DROP_PARAMS SLAB_BAND_PARAMS)

SLAB_KERNEL_SIGNATURE;

// ---------------------------------------------------------------------------------------------------------------
// The scaffold of a kernel body.  Everything here is inlined into the one kernel of its translation unit and takes the
// thread's `tid` / `lane` as an argument: each body decides where its lane number becomes opaque to the compiler (the
// split-bf16 body makes it so per item, for its registers).

// dynamic LDS: vals | cells (u64) | staging x 2 | item slot; V is a value cell, the pair (T[y], T[y+1]) of a table column
// -- `unsigned` (a packed 16-bit pair) in the 16-bit modes, f32x2 in split-bf16
template <typename V>
struct SlabMem {
  V* vals;
  unsigned long long* cells;
  char* stage;
  int* item_slot;
  unsigned cells_off;     // byte offset of `cells` in LDS: a value's gradient cell from its own offset, without a pointer
};
template <typename V, int RP>
__device__ __forceinline__ SlabMem<V> slab_carve(char* lds, int sw) {
  static_assert(RP % 64 == 0, "the two taps of a pair are one ds_read2st64_b32");
  static_assert(sizeof(V) + 8 == SLAB_CELL, "slab_lds_bytes");
  const int ncell = (sw + 2) * RP;
  SlabMem<V> m;
  m.vals = reinterpret_cast<V*>(lds);
  m.cells = reinterpret_cast<unsigned long long*>(lds + (size_t)ncell * sizeof(V));
  m.stage = reinterpret_cast<char*>(m.cells) + (size_t)ncell * 8;
  m.item_slot = reinterpret_cast<int*>(m.stage + 2 * SlabLds::BUF);
  m.cells_off = (unsigned)(ncell * (int)sizeof(V));
  return m;
}

// The index of the workgroup's next work item in the list (uniform), off the launch's atomic counter.
template <typename V>
__device__ __forceinline__ int slab_claim(int tid, const SlabMem<V>& m, int* cnt) {
  SLAB_BARRIER();                                   // everybody is done with the previous item's slot and slab
  if (tid == 0) m.item_slot[0] = atomicAdd(cnt + 1, 1);
  SLAB_BARRIER();
  // read through readfirstlane: an LDS load is divergent to the compiler, and everything derived from the item (the
  // problem's pointers, the slab's origin, the chunk's columns) would live in vector registers
  return __builtin_amdgcn_readfirstlane(m.item_slot[0]);
}
// a work item, decoded: (problem, head) ph = prob * heads + hd, its problem-group pg and query batch qb; the slab's first
// owned table column x0; the chunk's BEV columns [j0, j1); the head's table and table gradient
struct SlabItem {
  int ph, slab, chunk, prob, hd, pg, qb, x0, j0, j1;
  const char* tbl;
  float* dtb;
};
// (hpg = heads / groups: the kernel's, formed once -- a division is not hoisted out of a loop it may not reach)
__device__ __forceinline__ SlabItem slab_item(const int4* items, int i, const bevr_attn_desc& d, int hpg, int sw,
                                              const char* table_pair, float* dtable) {
  const int4 item = items[i];
  SlabItem it;
  it.ph = __builtin_amdgcn_readfirstlane(item.x);
  it.slab = __builtin_amdgcn_readfirstlane(item.y);
  it.chunk = __builtin_amdgcn_readfirstlane(item.z);
  it.prob = it.ph / d.heads;
  it.hd = it.ph % d.heads;
  it.pg = it.prob * d.groups + it.hd / hpg;
  it.qb = it.prob / d.q_div;
  it.x0 = slab_xmin(d) + it.slab * sw;
  it.j0 = it.chunk * SLAB_CH;
  it.j1 = min(d.S, it.j0 + SLAB_CH);
  it.tbl = table_pair + (size_t)it.hd * d.Wp * d.Hp * 8;
  it.dtb = dtable + (size_t)it.hd * d.Wp * (d.Hp + 1);
  return it;
}

// The slab in: the values of the item's columns x0 .. x0 + sw of its head's table, as conv(T[y], T[y+1]) makes a cell of
// them, the kill column at `kill`, every gradient cell cleared.
template <int RP, typename V, typename Conv>
__device__ __forceinline__ void slab_fill(int tid, const SlabMem<V>& m, const bevr_attn_desc& d, const SlabItem& it, int sw,
                                          int R, Conv conv, V kill) {
  for (int u = tid; u < (sw + 1) * RP; u += STHREADS) {
    const int c = u / RP, w = u - c * RP;
    const int xc = it.x0 + c + d.x_off;             // padded table column
    const int yr = w - SLAB_ROW0 + d.y_off;         // padded table row
    f32x2 v = {0.f, 0.f};
    if (w < R && yr >= 0 && yr < d.Hp && xc >= 0 && xc < d.Wp)   // tiny S: the window is taller than the padded table
      v = *reinterpret_cast<const f32x2*>(it.tbl + ((size_t)xc * d.Hp + yr) * 8);
    m.vals[RP + u] = conv(v);
    m.cells[RP + u] = 0ull;
  }
  for (int u = tid; u < RP; u += STHREADS) {
    m.vals[u] = kill;
    m.cells[u] = 0ull;
  }
}

// The slab out: every non-zero gradient cell once, to the head's table gradient (ginv: cell units to the caller's)
template <int RP, typename V>
__device__ __forceinline__ void slab_flush(int tid, const SlabMem<V>& m, const bevr_attn_desc& d, const SlabItem& it, int sw,
                                           int R, float ginv) {
  const int Hq = d.Hp + 1;
  for (int u = tid; u < (sw + 1) * RP; u += STHREADS) {
    const int c = u / RP, w = u - c * RP;
    const unsigned long long v = w < R ? m.cells[RP + u] : 0ull;
    if (v != 0ull) {
      const int xc = it.x0 + c + d.x_off, yr = w - SLAB_ROW0 + d.y_off;
      if (xc >= 0 && xc < d.Wp && yr >= 0 && yr < Hq) atomicAdd(it.dtb + (size_t)xc * Hq + yr, AccCell::to_float(v) * ginv);
    }
  }
}

// The producer's emission iterator over the key runs of the item's columns: an emission is up to SEK keys [k0, kend) of
// ONE column's run.  The iterator stands one emission ahead of the one being staged: the body takes emission e + 1 for
// its loads -- if (more()) { take(); ... step(); } -- before it hands emission e over.
struct SlabRuns {
  int my_beg, my_end;       // lane c: the run of column j0 + c
  int ncol;                 // j1 - j0
  int lc, lk, lend;         // the next emission to load: column index, first key, the run's end
  int c, k0, kend;          // the emission taken last
  int prev_c;

  __device__ __forceinline__ void seek() {    // from column index lc on: the first column with a non-empty run; lc == ncol: none left
    while (lc < ncol) {
      const int b = __builtin_amdgcn_readlane(my_beg, lc), e = __builtin_amdgcn_readlane(my_end, lc);
      if (b < e) { lk = b; lend = e; return; }
      ++lc;
    }
  }
  __device__ __forceinline__ void start(int lane, const int* kbeg, const int* kend_, const bevr_attn_desc& d,
                                        const SlabItem& it, int n_slab) {
    const size_t rbase = ((size_t)it.pg * n_slab + it.slab) * d.S;
    my_beg = it.j0 + lane < it.j1 ? kbeg[rbase + it.j0 + lane] : 0;
    my_end = it.j0 + lane < it.j1 ? kend_[rbase + it.j0 + lane] : 0;
    ncol = it.j1 - it.j0;
    lc = 0; lk = 0; lend = 0;
    seek();
    c = -1; k0 = 0; kend = 0;
    prev_c = -1;
  }
  __device__ __forceinline__ bool more() const { return lc < ncol; }
  __device__ __forceinline__ void take() { c = lc; k0 = lk; kend = lend; }
  __device__ __forceinline__ void step() {
    lk += SEK;
    if (lk >= lend) { ++lc; seek(); }
  }
  // the emission taken last, read BEFORE the next take(): its column index and keys, and whether it is its column's first
  // and last emission (the iterator already points at the next one)
  struct Emission { int c, k0, kend; bool first, last; };
  __device__ __forceinline__ Emission emission() {
    const Emission e = {c, k0, kend, c != prev_c, !(lc < ncol) || lc != c};
    prev_c = c;
    return e;
  }
};

// a live key whose rows leave the window for some row block: its half takes the clamped body
__device__ __forceinline__ bool slab_far(const bevr_attn_desc& d, int A) { return A + SLAB_ROW0 < 0 || A > d.S - 1 + SLAB_PADR; }
// The control word of an emission, producer to workers: which of the two 32-key halves have a live key, which a far one,
// the column j, first / last emission of the column.  `live`: this lane's key belongs to the emission and to the slab;
// `far`: live && slab_far; jn: a field of the body's own (16-bit: the column to prefetch, plus one).
__device__ __forceinline__ void slab_post(char* bb, int lane, bool live, bool far, const SlabRuns::Emission& em, int j,
                                          unsigned jn = 0u) {
  const unsigned long long lm = __ballot(live), fm = __ballot(far);
  const unsigned hb = ((unsigned)lm != 0u ? 1u : 0u) | ((unsigned)(lm >> 32) != 0u ? 2u : 0u) |
                      ((unsigned)fm != 0u ? 4u : 0u) | ((unsigned)(fm >> 32) != 0u ? 8u : 0u);
  if (lane == 0)
    *reinterpret_cast<u32x4*>(bb + SlabLds::OFF_CT) =
        u32x4{(unsigned)((em.first ? SF_FIRST : 0) | (em.last ? SF_LAST : 0)) | (hb << 8), (unsigned)j | (jn << 16), 0u, 0u};
}
// after the item's last emission: the workers leave their loop
__device__ __forceinline__ void slab_post_done(char* bb, int lane) {
  if (lane == 0) *reinterpret_cast<u32x4*>(bb + SlabLds::OFF_CT) = u32x4{(unsigned)SF_DONE, 0u, 0u, 0u};
}
// ... as a worker reads it (uniform: scalar registers)
struct SlabCtl {
  unsigned flags, jword;
  __device__ __forceinline__ bool done() const { return flags & SF_DONE; }
  __device__ __forceinline__ bool first() const { return flags & SF_FIRST; }
  __device__ __forceinline__ bool last() const { return flags & SF_LAST; }
  __device__ __forceinline__ int j() const { return (int)(jword & 0xffffu); }
  __device__ __forceinline__ int jn() const { return (int)(jword >> 16); }
  __device__ __forceinline__ unsigned halves() const { return flags >> 8; }   // bits 0, 1: the halves with a live key; bits 2, 3: with a far one
};
__device__ __forceinline__ SlabCtl slab_read_ctl(const char* bb) {
  const u32x4 ct = *reinterpret_cast<const u32x4*>(bb + SlabLds::OFF_CT);
  return SlabCtl{(unsigned)__builtin_amdgcn_readfirstlane((int)ct[0]), (unsigned)__builtin_amdgcn_readfirstlane((int)ct[1])};
}

// ---------------------------------------------------------------------------------------------------------------
// launch and entry points
template <int PREC, int RP>
int launch(const bevr_attn_desc& d, const void* Q, const void* Ks, const void* Vs, const void* ws, const float* table_pair,
           const void* dO, const float* LSE, const float* delta, const float* grad_scale, float* dQ, float* dtable,
           int row0, int n_rb_band, hipStream_t st BEVR_DROP_PARAMS) {
  const SlabWs w = slab_ws(d);
  const char* base = static_cast<const char*>(ws);
  int* cnt = reinterpret_cast<int*>(const_cast<char*>(base) + w.off_cnt);
  hipError_t e = hipMemsetAsync(cnt + 1, 0, 4, st);       // the item counter of this launch
  if (e != hipSuccess) return (int)e;
  // one workgroup per CU of the current device, with more than 64 KB of dynamic LDS
  const int n_cu = bevr_cu_count();
  if (n_cu <= 0) return BEVR_E_SHAPE;
  const int R = slab_rows(d.S);
  const size_t lds = slab_lds_bytes(d.S, w.sw, RP);
  const int ea = bevr_raise_dynamic_lds<&SLAB_KERNEL(PREC, RP)>(160 * 1024);
  if (ea) return ea;
  hipLaunchKernelGGL((SLAB_KERNEL(PREC, RP)), dim3(n_cu), dim3(STHREADS), lds, st, d, (const char*)Q,
                     (const char*)Ks, (const char*)Vs, reinterpret_cast<const SlabKey*>(base),
                     reinterpret_cast<const int*>(base + w.off_beg), reinterpret_cast<const int*>(base + w.off_end),
                     reinterpret_cast<const int4*>(base + w.off_items), cnt, (const char*)table_pair, (const char*)dO,
                     LSE, delta, grad_scale, dQ, dtable, w.n_slab, w.sw, R BEVR_DROP_ARGS SLAB_BAND_ARGS);
  return (int)hipGetLastError();
}

// the modes this translation unit holds the kernels of
#if BEVR_SLAB_X3
__host__ __device__ constexpr bool slab_prec_x3(int prec) { return prec == BEVR_PREC_BF16X3; }
#define SLAB_PREC_OK slab_prec_x3
#define SLAB_PRECS BEVR_PREC_BF16X3
#else
#define SLAB_PREC_OK is16
#define SLAB_PRECS BEVR_PREC_BF16, BEVR_PREC_F16
#endif
#if BEVR_SLAB_ROWS
// any S up to 448: a small S runs on the 832 pitch like any other (its window is shorter than the pitch, as S < 200's is
// at 448).  Split-bf16: 16-byte cells on the same two pitches -- 7 owned columns at 832 (9 x 832 x 16 + 2 x 18 464 + 64 =
// 156 800 bytes of LDS), 6 at 960 (159 872)
bool slab_shape_ok(const bevr_attn_desc& d) {
  return SLAB_PREC_OK(d.precision) && d.S <= SLAB_ROWS_MAX_S && slab_rows(d.S) <= slab_pitch(d.S) && SLAB_CH <= 64 &&
         slab_lds_bytes(d.S, slab_width(d.S, slab_pitch(d.S)), slab_pitch(d.S)) <= 160 * 1024;
}
// a band of row blocks: starts on a block, at most SNRB blocks, whole blocks unless it ends the column (no sum is formed
// before its terms are bounded: 1 << 30 does not wrap)
bool slab_band_ok(const bevr_attn_desc& d, int row0, int n_rows) {
  if (row0 < 0 || row0 % SQROWS != 0 || n_rows < 1 || n_rows > SLAB_BAND_ROWS) return false;
  if (row0 > d.S - n_rows) return false;
  return n_rows % SQROWS == 0 || row0 == d.S - n_rows;
}
#else
bool slab_shape_ok(const bevr_attn_desc& d) {
  return SLAB_PREC_OK(d.precision) && slab_n_rb(d.S) <= SNRB && slab_rows(d.S) <= SLAB_RP && SLAB_CH <= 64 &&
         slab_lds_bytes(d.S, slab_width(d.S)) <= 160 * 1024;
}
#endif
// the entry points' names; the masked units have a preparation of their own: it writes SlabKey::pad, and the code of the
// unmasked units' stays what it is
#if BEVR_SLAB_ROWS && BEVR_SLAB_X3
#define SLAB_WS_BYTES bevr_attn_slab_x3_rows_ws_bytes
#define SLAB_PREP bevr_attn_slab_x3_rows_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q_x3_rows
#elif BEVR_SLAB_ROWS
#define SLAB_WS_BYTES bevr_attn_slab_rows_ws_bytes
#define SLAB_PREP bevr_attn_slab_rows_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q_rows
#elif BEVR_SLAB_X3 && BEVR_DROP
#define SLAB_WS_BYTES bevr_attn_slab_x3_drop_ws_bytes
#define SLAB_PREP bevr_attn_slab_x3_drop_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q_x3_dropout
#elif BEVR_SLAB_X3
#define SLAB_WS_BYTES bevr_attn_slab_x3_ws_bytes
#define SLAB_PREP bevr_attn_slab_x3_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q_x3
#elif BEVR_DROP
#define SLAB_WS_BYTES bevr_attn_slab_drop_ws_bytes
#define SLAB_PREP bevr_attn_slab_drop_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q_dropout
#else
#define SLAB_WS_BYTES bevr_attn_slab_ws_bytes
#define SLAB_PREP bevr_attn_slab_prep
#define SLAB_BWD_Q bevr_attn_slab_bwd_q
#endif

}  // namespace

extern "C" size_t SLAB_WS_BYTES(const bevr_attn_desc* d) {
  if (bevr_check_desc(d) || !slab_shape_ok(*d)) return 0;
  return slab_ws(*d).total;
}

extern "C" int SLAB_PREP(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int* order,
                         void* slab_ws_, void* stream) {
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!key_a || !key_b || !order || !slab_ws_) return BEVR_E_NULL;
  if (!SLAB_PREC_OK(d->precision)) return BEVR_E_PRECISION;
  if (!slab_shape_ok(*d)) return BEVR_E_SHAPE;
  if (!bevr_aligned16(slab_ws_)) return BEVR_E_ALIGN;
  const SlabWs w = slab_ws(*d);
  char* base = static_cast<char*>(slab_ws_);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(base + w.off_cnt, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  const size_t nk = (size_t)d->n_prob * d->groups * d->N;
  hipLaunchKernelGGL(slab_keys_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, *d, key_a, key_b, order,
                     reinterpret_cast<SlabKey*>(base));
  const int nt = d->n_prob * d->groups * w.n_slab * w.n_chunk;
  hipLaunchKernelGGL(slab_ranges_kernel, dim3((nt + 255) / 256), dim3(256), 0, st, *d,
                     reinterpret_cast<const SlabKey*>(base), reinterpret_cast<int*>(base + w.off_beg),
                     reinterpret_cast<int*>(base + w.off_end), reinterpret_cast<int4*>(base + w.off_items),
                     reinterpret_cast<int*>(base + w.off_cnt), w.n_slab, w.n_chunk, w.sw);
  return (int)hipGetLastError();
}

// The contract of the six slab bwd_q entry points, written once.  After the operands: the band (row0, n_rows) of
// BEVR_SLAB_ROWS, the keep mask (drop_thr, drop_seed) of BEVR_DROP, the stream.
extern "C" int SLAB_BWD_Q(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs, const void* slab_ws_,
                          const float* table_pair, const void* dO, const float* LSE, const float* delta,
                          const float* grad_scale, float* dQ, float* dtable
#if BEVR_SLAB_ROWS
                          , int row0, int n_rows
#endif
                          BEVR_DROP_PARAMS, void* stream) {
#if BEVR_DROP
  if (drop_thr >= 65536u) return BEVR_E_SHAPE;
#endif
#if !BEVR_SLAB_ROWS
  const int row0 = 0, n_rows = 0;
#endif
  int rc = bevr_check_desc(d);
  if (rc) return rc;
  if (!Q || !Ks || !Vs || !slab_ws_ || !table_pair || !dO || !LSE || !delta || !grad_scale || !dQ || !dtable)
    return BEVR_E_NULL;
  // the precision before the shape before the alignment
  return bevr_for_precision<SLAB_PRECS>(d->precision, [&](auto P) {
    if (!slab_shape_ok(*d)) return (int)BEVR_E_SHAPE;
#if BEVR_SLAB_ROWS
    if (!slab_band_ok(*d, row0, n_rows)) return (int)BEVR_E_SHAPE;
#endif
    if (!bevr_aligned16(Q) || !bevr_aligned16(Ks) || !bevr_aligned16(Vs) || !bevr_aligned16(dO) || !bevr_aligned16(dQ) ||
        !bevr_aligned16(table_pair) || !bevr_aligned16(slab_ws_))
      return (int)BEVR_E_ALIGN;
    const int nb = (n_rows + SQROWS - 1) / SQROWS;
    auto go = [&](auto RP) {
      return launch<decltype(P)::value, decltype(RP)::value>(*d, Q, Ks, Vs, slab_ws_, table_pair, dO, LSE, delta,
                                                             grad_scale, dQ, dtable, row0, nb, (hipStream_t)stream
                                                             BEVR_DROP_ARGS);
    };
#if BEVR_SLAB_ROWS
    return slab_pitch(d->S) == SLAB_RP_B ? go(std::integral_constant<int, SLAB_RP_B>())
                                         : go(std::integral_constant<int, SLAB_RP_A>());
#else
    return go(std::integral_constant<int, SLAB_RP>());
#endif
  });
}
