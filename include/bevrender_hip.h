/*
 * bevrender_hip.h -- C ABI of libbevrender_hip.so: the MI355X (gfx950) kernels behind the
 * BEV-lift + correlation hot path of rpl-cmu/bevrender.
 *
 * The reference has no FFI: its boundary is Python nn.Module.forward.  The
 * Python modules in bevrender_amd/model/ mirror that interface and bind these entry points with
 * ctypes (bevrender_amd/_lib.py); INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA storage) unless named host_*;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all calls are asynchronous
 *     on that stream, allocate nothing and never synchronise (graph-capture safe);
 *   - return value: 0 on success, a negative BEVR_E_* code when the arguments violate the stated
 *     contract (nothing is launched), a positive hipError_t if the launch itself failed;
 *   - tensors are dense row-major with the layouts written next to each argument.
 *
 * Reference functions replaced (paths relative to the reference repo):
 *   bevr_project_bev_grid[_masked]  model/bev_cmr_proj.py:61-124  (bev_grid_to_camera + get_in_bound_mask)
 *   bevr_sample_fwd/bwd     F.grid_sample at model/SCA_deform_attn.py:290-301, model/TSA_deform_attn.py:210-217
 *   bevr_attn_fwd/bwd_*     model/SCA_deform_attn.py:331-413, model/TSA_deform_attn.py:245-333
 *                           (QK^T*scale + bilinear RPE bias + softmax + PV, never materialised)
 *   bevr_attn_cell_*        the same lines, for key segments sorted by rpe-table cell (bias as a matrix product)
 *   bevr_pack_kv/unpack_dkv model/SCA_deform_attn.py:312-321 (projection outputs -> per-head operand layouts)
 *   bevr_dwconv_fwd/bwd_w   model/encoder.py:363-411, model/model_utils.py:6-35 (depthwise 3x3 of the layer glue)
 *   bevr_offset_head_fwd/bwd  model/SCA_deform_attn.py:56-77, model/TSA_deform_attn.py:54-68 (offset heads, fused)
 *   bevr_layernorm_fwd/bwd  model/model_utils.py:37-49, model/encoder.py:275 (LayerNormProxy)
 *   bevr_merge_views_fwd/bwd  model/SCA_deform_attn.py:415-420, model/TSA_deform_attn.py:325-333 (view concat before proj_out)
 *   bevr_kv_project         model/SCA_deform_attn.py:290-321, model/TSA_deform_attn.py:210-236 (sample + proj_k | proj_v + pack)
 *   bevr_key_positions_fwd/bwd  model/SCA_deform_attn.py:248-277, model/TSA_deform_attn.py:170-196 (row split, tanh range, + ref, key order)
 *   bevr_affine_warp_fwd/bwd  model/encoder.py:413-466 (project_history_bev_feat: torchvision F.affine, twice)
 *   bevr_corr_fwd/bwd       train.py:554 (2 - 2 cam map^T) and the pairwise distance inside
 *                           loss/contrastive_loss.py:10-19 / loss/lift_loss.py:13-22
 */
#ifndef BEVRENDER_HIP_H
#define BEVRENDER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: bevr_attn_fwd writes TWO LSE planes (round 2 changed that under version 2: a version-2 caller's [n_prob][heads][Mp]
 *    buffer is too small), the key workspace carries group boxes, bevr_attn_bwd_q takes grad_scale; new: bevr_attn_cell_*,
 *    problem strides of bevr_pack_kv / bevr_unpack_dkv, BEVR_PREC_F16, grad_scale[8] for every backward entry point. */
/* 4: new entry points bevr_attn_tap_* (the projector-pinned keys without K / V), bevr_attn_gather_fwd (the forward over
 *    scattered keys with the bias on the matrix cores) and bevr_attn_*_dropout; nothing else
 *    changed. */
/* 5: new entry points bevr_attn_slab_ws_bytes / _slab_prep / _slab_bwd_q (the query-side backward cut along the rpe
 *    table: a workgroup owns a slab of table columns); bevr_attn_tap_bwd_k's table operand is declared as what it always
 *    was (the plain packed table, not the pair table); bevr_kv_project takes the channel-group count (before `stream`);
 *    nothing else changed. */
/* 6: bevr_kv_project takes `float* knorm2_max` (the largest squared K row norm per problem and head) before `groups`;
 *    new entry points bevr_merge_views_fwd / _bwd, bevr_merge_tap_fwd / _bwd, bevr_attn_bwd_prep and
 *    bevr_dwconv_res_gelu; bevr_corr_bwd with aliased operands (cam == map, n == m) writes both sides' sum into dcam and
 *    leaves dmap untouched, on every path (see its declaration); nothing else changed.
 *    Added since, without a new version (nothing a version-6 caller uses changed): bevr_attn_tap_fwd_dropout,
 *    bevr_attn_tap_bwd_q_dropout, bevr_attn_tap_bwd_k_dropout (attention dropout on the tap entry points);
 *    bevr_attn_gather_fwd_rows (the gather forward over a row range of every BEV column: BEV sides above 224), and
 *    bevr_attn_gather_fwd accepts BEVR_PREC_F16 where it returned BEVR_E_PRECISION;
 *    bevr_attn_tap_fwd, bevr_attn_tap_bwd_q and bevr_attn_tap_bwd_k accept BEVR_PREC_BF16X3 where they returned
 *    BEVR_E_PRECISION (operand format: "TAP entry points in BEVR_PREC_BF16X3" below);
 *    bevr_attn_slab_rows_ws_bytes / _slab_rows_prep / bevr_attn_slab_bwd_q_rows (the slab query-side backward over a band
 *    of BEV rows of every column: BEV sides up to 448; the three bevr_attn_slab_* entry points keep their contract);
 *    bevr_attn_gather_fwd_x3 (the gather forward in BEVR_PREC_BF16X3, over a row range; bevr_attn_gather_fwd and
 *    bevr_attn_gather_fwd_rows keep returning BEVR_E_PRECISION for that mode);
 *    bevr_attn_slab_x3_ws_bytes / _slab_x3_prep / bevr_attn_slab_bwd_q_x3 (the slab query-side backward in
 *    BEVR_PREC_BF16X3, S <= 211; the 16-bit slab entry points keep returning BEVR_E_PRECISION for that mode);
 *    bevr_attn_tap_fwd_x3_dropout, bevr_attn_tap_bwd_q_x3_dropout, bevr_attn_tap_bwd_k_x3_dropout (attention dropout on
 *    the tap entry points in BEVR_PREC_BF16X3; the three _dropout entry points keep returning BEVR_E_PRECISION for that
 *    mode);
 *    bevr_attn_tap_g2_ws_bytes / _tap_g2_prep / _tap_g2_fwd / _tap_g2_bwd_q / _tap_g2_bwd_k (the tap entry points for two
 *    channel groups, 32-slot operands; the one-group tap entry points keep returning BEVR_E_SHAPE for groups != 1);
 *    bevr_attn_gather_fwd_dropout (the gather forward with the keep mask, over a row range) and
 *    bevr_attn_slab_drop_ws_bytes / _slab_drop_prep / bevr_attn_slab_bwd_q_dropout (the slab query-side backward with
 *    the keep mask, S <= 211), both in the 16-bit modes; every other gather and slab entry point keeps its contract;
 *    bevr_kv_project_w2 (bevr_kv_project with the weights as two E planes, hi + lo; bevr_kv_project keeps its
 *    contract);
 *    bevr_attn_slab_x3_drop_ws_bytes / _slab_x3_drop_prep / bevr_attn_slab_bwd_q_x3_dropout (the slab query-side backward
 *    with the keep mask in BEVR_PREC_BF16X3, S <= 211; every other slab entry point keeps its contract);
 *    bevr_attn_slab_x3_rows_ws_bytes / _slab_x3_rows_prep / bevr_attn_slab_bwd_q_x3_rows (the slab query-side backward in
 *    BEVR_PREC_BF16X3 over a band of BEV rows of every column: BEV sides up to 448; every other slab entry point keeps
 *    its contract). */
#define BEVR_ABI_VERSION 6

enum {
  BEVR_OK = 0,
  BEVR_E_NULL = -1,      /* a required pointer is NULL */
  BEVR_E_SHAPE = -2,     /* a dimension violates the contract below */
  BEVR_E_PRECISION = -3, /* unknown precision code */
  BEVR_E_ALIGN = -4      /* a pointer is not 16-byte aligned */
};

/* BEVR_PREC_F16: fp16 operands (v_mfma_f32_32x32x16_f16), f32 accumulate -- BASELINE config 5.  fp16 has 5 exponent bits:
 * the kernels keep softmax weights and logit gradients inside its normal range with power-of-two scales (forward: the
 * softmax reference sits 10 binades below the running maximum; backward: grad_scale[2..5]). */
/* BEVR_PREC_BF16X3: the fp32-tolerance mode that is not bound by the f32 matrix rate.  Every matrix operand is split
 *   x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (round to nearest), and a product runs as three bf16 MFMAs
 *   (lo*hi + hi*lo + hi*hi; the lo*lo term, <= 2^-16 of the product, is dropped); everything per pair -- bias taps, f32
 *   table window, softmax -- is BEVR_PREC_F32's arithmetic.  Results agree with BEVR_PREC_F32 to ~1e-5 relative.
 *   Packed operands (Q, K, V, dO and their transposes) keep BEVR_PREC_F32's shapes, strides and byte sizes (E = float
 *   as a container) but hold the two bf16 planes:
 *     row layout, per 16-element half [e0..e15] of a 32-element row (64 bytes):
 *         hi(e0..e7) | hi(e8..e15) | lo(e0..e7) | lo(e8..e15)
 *     transposed (bits 2 <-> 3 swapped) layout, per block of 32 (128 bytes = 8 chunks of 16 bytes), y[q] = the block in
 *     the f32 mode's order:   chunk 2 h + s = hi(y[16 s + 8 h .. + 7]),   chunk 4 + 2 h + s = lo(same),   h, s in {0, 1}
 *   bevr_pack_kv writes K, V in this format; bevrender_amd/ops.py (_split_rows, _split_perm_t) is the definition the
 *   tests compare it with and what packs Q and dO. */
enum { BEVR_PREC_F32 = 0, BEVR_PREC_BF16 = 1, BEVR_PREC_F16 = 2, BEVR_PREC_BF16X3 = 3 };

int bevr_abi_version(void);
/* Human-readable text for a BEVR_E_* code (static storage). */
const char* bevr_strerror(int code);

/* ------------------------------------------------------------------------------------------------
 * Attention core geometry shared by the three attention kernels.
 *
 * Queries are the S x S BEV grid.  The kernels index them column-major with the rows of a column
 * padded to Sp = 32*ceil(S/32): packed query index  mq = j*Sp + i  (i = BEV row, j = BEV column),
 * Mp = S*Sp.  Rows i >= S are padding (zero on input, ignored on output).
 * Keys: N real keys padded to Np (multiple of 64); keys >= N are masked inside the kernels.
 * head_dim is fixed at 32 (the reference's dims/heads always give 32; smaller heads are zero-padded
 * by the caller).  heads % groups == 0; the heads of one group share key positions.
 *
 * Relative-position bias: the reference samples rpe_table[h, Ht=2S-1, Wt] bilinearly at
 *   ty = i + a_n,         a_n = (1 - py_n) * (S-1)/2
 *   tx = j * rx + b_n,    b_n = (1 - px_n) * (Wt-1)/4,   rx = (Wt-1) / (2(S-1))
 * (algebraically identical to grid_sample(align_corners=True) of (q_grid - pos)/2).
 * The table is handed over transposed, zero-padded and pair-packed:
 *   table_pair[h][Wp][Hp][2] = ( T2[y - y_off][x - x_off], T2[y + 1 - y_off][x - x_off] ),  T2 = T * log2(e),
 * zero outside the real table, with  y_off = Sp + 2, Hp = Ht + 2*Sp + 4,
 * x_off = (Wt-1)/2 + 4, Wp = 2*Wt + 8  (bevr_attn_table_dims computes them).
 * Keys carry key_a[n] = a_n, key_b[n] = b_n (float, any value; the kernels clamp to the padded range,
 * where every tap is zero exactly as grid_sample's zero padding).
 * Q is pre-multiplied by head_dim^-0.5 * log2(e); logits and LSE are in log2 units.
 * ---------------------------------------------------------------------------------------------- */
typedef struct bevr_attn_desc {
  int32_t n_prob;    /* B' = batch * views: independent softmax problems per head            */
  int32_t q_div;     /* query batch index = prob / q_div (views of one sample share the query) */
  int32_t heads;     /* h                                                                    */
  int32_t groups;    /* g                                                                    */
  int32_t S;         /* BEV side                                                             */
  int32_t Sp;        /* padded rows per column, 32*ceil(S/32)                                */
  int32_t N;         /* real keys                                                            */
  int32_t Np;        /* padded keys, multiple of 64                                          */
  int32_t Ht, Wt;    /* rpe table height (must equal 2S-1) and width                         */
  int32_t Hp, Wp;    /* padded table dims                                                    */
  int32_t y_off, x_off;
  int32_t precision; /* BEVR_PREC_F32: exact-f32 MFMA; BEVR_PREC_BF16 / BEVR_PREC_F16: 16-bit operands, f32 accumulate */
  int32_t reserved;
} bevr_attn_desc;

/* Fill Sp, Hp, Wp, y_off, x_off from S, Wt.  Returns 0 or BEVR_E_SHAPE. */
int bevr_attn_table_dims(bevr_attn_desc* d);

/* Key preparation, once per attention call (shared by bevr_attn_fwd and bevr_attn_bwd_q of the same keys);
 * replaces the query-grid / key-position displacement of model/SCA_deform_attn.py:352-378 and
 * model/TSA_deform_attn.py:264-291 (reference), reduced to per-key table coordinates:
 * clamps key_a/key_b, splits them into table row / fraction / column parts and reduces, per 64-key step, the
 * bounding box of the table taps the step needs.  key_ws: caller-allocated device buffer of
 * bevr_attn_key_ws_bytes(d) bytes, 16-byte aligned; its content is opaque to the caller.
 *   key_a, key_b [n_prob*groups][Np] float */
size_t bevr_attn_key_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_key_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, void* key_ws, void* stream);

/* Forward.  Element type E = float (F32), bf16 (BF16) or fp16 (F16).
 *   Q   [n_prob/q_div][heads][Mp][32]  E     K  [n_prob][heads][Np][32] E
 *   Vt  [n_prob][heads][32][Np] E, keys permuted inside each aligned block of 32: the key with
 *       in-block index r is stored at position (r & 19) | ((r & 4) << 1) | ((r & 8) >> 1)
 *       (bits 2 and 3 swapped) -- the order the MFMA consumes the P accumulator in.
 *   key_ws: output of bevr_attn_key_prep for these keys      table_pair as above, float
 *   O   [n_prob][heads][Mp][32] float (normalised)
 *   LSE [2][n_prob][heads][Mp] float: plane 0 the log2-sum-exp of the row (what the backward entry points read:
 *       they take a pointer to plane 0), plane 1 an upper bound of log2 of the row's largest softmax weight (may exceed 0: clamp;
 *       rows past the grid: unspecified), from which the caller may tighten grad_scale of bevr_attn_bwd_q */
int bevr_attn_fwd(const bevr_attn_desc* d, const void* Q, const void* K, const void* Vt,
                  const void* key_ws, const float* table_pair,
                  float* O, float* LSE, void* stream);

/* Backward, query side (same tiling as the forward):  dQ [like Q, float] and the table gradient
 *   dtable [heads][Wp][Hp+1] float, transposed/padded like table_pair but one value per entry;
 *   it is ACCUMULATED into (caller zeroes it).
 *   V  [n_prob][heads][Np][32] E (row layout), Kt [like Vt] E, dO [n_prob][heads][Mp][32] E,
 *   delta [n_prob][heads][Mp] float = rowsum(dO * O).
 *   grad_scale [8] float (device): { s, 1/s, kp, c2, 1/(2^kp c2), 2^-kp, 0, 0 }.  s: a power of two such that s * max|P (dP - delta)| <= 2^30; a
 *   valid bound is Pmax * (max_q |dO_q| * max_n |V_n| + max |delta|) (Euclidean norms over the 32 channels), Pmax = 1
 *   or the largest softmax weight of the launch (2^max of LSE plane 1, with a margin for the recomputation).  The
 *   kernel multiplies dO and delta by s as it loads them (exact) and accumulates the table gradient in 64-bit fixed
 *   point with unit ln2 / s (each contribution rounded to nearest; sums are exact and order-independent within a
 *   workgroup's window, and a cell cannot wrap: 2^33 contributions of the largest size fit); ln2 / s is applied
 *   when a cell is flushed and when dQ is stored.
 *   Entries 2..5 are read in BEVR_PREC_F16 mode only, by every backward entry point (the others take the same array
 *   and ignore it in the other modes): kp, an integer-valued exponent with Pmax 2^kp <= 2^14 -- the kernels form
 *   P' = P 2^kp so that fp16 holds the softmax weights in its normal range; c2, a power of two with
 *   max|P' (dP - delta) c2| <= 2^14 -- the logit gradient as fp16 operand; then their inverses.  bevr_attn_bwd_q
 *   additionally needs s = 2^16 2^kp c2 there (its fixed-point cells then count units of 2^-16 of an fp16 operand,
 *   and s max|P (dP - delta)| <= 2^30 as in the other modes); dO and delta are NOT pre-scaled by s in this mode.
 *   All gradients are with respect to the log2-domain logits' inputs as handed in (Q pre-scaled,
 *   table pre-multiplied): the caller's autograd undoes the scaling. */
int bevr_attn_bwd_q(const bevr_attn_desc* d, const void* Q, const void* K, const void* Kt, const void* V,
                    const void* key_ws, const float* table_pair,
                    const void* dO, const float* LSE, const float* delta, const float* grad_scale,
                    float* dQ, float* dtable, void* stream);

/* Backward, key side:  dK, dV [n_prob][heads][Np][32] float, dkey_a, dkey_b [n_prob*groups][Np] float
 *   (dkey_* are ACCUMULATED over the heads of a group; caller zeroes them).
 *   Qt, dOt: [..][heads][32][Mp] E with the same in-32 permutation as Vt (over the packed query index). */
int bevr_attn_bwd_k(const bevr_attn_desc* d, const void* Q, const void* Qt, const void* K, const void* V,
                    const float* key_a, const float* key_b, const float* table_pair,
                    const void* dO, const void* dOt, const float* LSE, const float* delta, const float* grad_scale,
                    float* dK, float* dV, float* dkey_a, float* dkey_b, void* stream);

/* bevr_attn_bwd_k with the rare key blocks of the general path (a block of 384 consecutive keys whose table slab does
 * not fit the main kernel's LDS ring) dispatched from a device work list: the main launch appends each such block to
 * `ws`, and a second launch of a FIXED number of workgroups shares (listed block, range of query tiles) items out --
 * instead of one workgroup per block of the whole grid that first finds out whether it has anything to do.  All four
 * precisions.  Same arguments and results as bevr_attn_bwd_k; the blocks of the general path are summed with float
 * atomics over a different split of the query sweep, so their dK / dV / dkey_* differ from bevr_attn_bwd_k's in the
 * order of the sums (as two runs of bevr_attn_bwd_k differ), every other block's rows are bit-equal.
 *   ws              device scratch of bevr_attn_bwd_k_ws_bytes(d) bytes, 16-byte aligned: a count and one int per
 *                   (problem-head, key block).  The entry point clears the count on `stream` itself; the contents
 *                   afterwards are unspecified.  One ws per call in flight.
 *   max_workgroups  0: as many workgroups as the device holds at once; > 0: at most that many (tests: items then
 *                   outnumber the workgroups).  < 0: BEVR_E_SHAPE. */
size_t bevr_attn_bwd_k_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_bwd_k_ws(const bevr_attn_desc* d, const void* Q, const void* Qt, const void* K, const void* V,
                       const float* key_a, const float* key_b, const float* table_pair,
                       const void* dO, const void* dOt, const float* LSE, const float* delta, const float* grad_scale,
                       float* dK, float* dV, float* dkey_a, float* dkey_b, void* ws, int max_workgroups, void* stream);

/* Attention dropout (nn.Dropout on the softmax weights: model/SCA_deform_attn.py:155,402-409,
 * model/TSA_deform_attn.py:90,313-323): the three entry points above with a keep mask.  The mask is not stored: pair
 * (problem-head ph = prob * heads + head, packed query mq, key n) is kept iff
 *     (mix(seed ^ ph * 0x9E3779B1 ^ mq * 0x85EBCA77 ^ n * 0xC2B2AE3D) >> 16) >= drop_thr,
 *     mix(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16      (32-bit arithmetic)
 * with drop_thr = round(p * 65536) < 65536, and a kept weight is scaled by 65536 / (65536 - drop_thr).  The forward
 * masks the weights AFTER the normalisation (LSE is of the unmasked logits, as the reference's softmax-then-dropout);
 * the backward entry points evaluate the same function (same seed): dS = P (D dP - delta), dV from D P.  delta is
 * still rowsum(dO * O).  grad_scale as for bevr_attn_bwd_q / _bwd_k with every Pmax of its contract read as D Pmax,
 * D = 65536 / (65536 - drop_thr): s D Pmax bound <= 2^30; fp16: D Pmax 2^kp <= 2^14 and D Pmax bound 2^kp c2 <= 2^14
 * (|D dP - delta| <= D bound: the fixed-point contributions and the fp16 operands D P', P' (D dP - delta) c2 stay in
 * range).  The forward applies D after the normalisation, to the output (its fp16 operands are the unscaled weights).
 * bevrender_amd/ops.py:dropout_keep_mask is the host twin.  The cell entry points have no mask: a caller with dropout
 * keeps their keys on these entry points.  The gather forward and the one-band slab bwd_q have dropout variants in the
 * 16-bit modes (bevr_attn_gather_fwd_dropout, bevr_attn_slab_bwd_q_dropout below: the same mask over the same key
 * numbering, so either may stand in for its region counterpart beside the other two); the split-bf16 gather, the
 * row-band and the split-bf16 slab entry points have none.  The tap entry points have dropout variants of their own
 * (bevr_attn_tap_*_dropout below), which hash the same function with an offset into the caller's key order. */
int bevr_attn_fwd_dropout(const bevr_attn_desc* d, const void* Q, const void* K, const void* Vt,
                          const void* key_ws, const float* table_pair, float* O, float* LSE,
                          unsigned drop_thr, unsigned drop_seed, void* stream);
int bevr_attn_bwd_q_dropout(const bevr_attn_desc* d, const void* Q, const void* K, const void* Kt, const void* V,
                            const void* key_ws, const float* table_pair, const void* dO, const float* LSE,
                            const float* delta, const float* grad_scale, float* dQ, float* dtable,
                            unsigned drop_thr, unsigned drop_seed, void* stream);
int bevr_attn_bwd_k_dropout(const bevr_attn_desc* d, const void* Q, const void* Qt, const void* K, const void* V,
                            const float* key_a, const float* key_b, const float* table_pair, const void* dO,
                            const void* dOt, const float* LSE, const float* delta, const float* grad_scale,
                            float* dK, float* dV, float* dkey_a, float* dkey_b, unsigned drop_thr, unsigned drop_seed,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cell-sorted key segments: the same attention with the relative-position bias (and its table gradient) as a small
 * matrix product on the matrix cores (csrc/attn_cell.h).  Same descriptor, operand layouts, table, key workspace
 * (bevr_attn_key_prep) and gradient semantics as the entry points above.  Fast when the keys of every aligned run
 * of 32 span fewer than 4 table columns and 4 table rows including their second taps -- what sorting keys that
 * crowd a few table cells by cell gives (the pillar points a camera does not see are all pinned to pixel (0, 0),
 * model/bev_cmr_proj.py:76 of the reference: two thirds of an SCA view's keys) -- correct for any keys (runs that do
 * not fit are gathered per pair from the table in global memory).  A workgroup is one BEV column: a wave per 32-row
 * block + a producer wave, 16 at most, and a Q (+ dO) slot per wave in LDS: BEVR_E_SHAPE for Sp > 480, and from
 * bevr_attn_cell_bwd_q with float-sized operands (BEVR_PREC_F32, BEVR_PREC_BF16X3) for Sp > 256 (160 KB of LDS); the
 * caller then keeps every key on the region entry points (bevrender_amd/ops.py:attention_core does).
 *
 * One softmax over two key segments: run bevr_attn_fwd on the scattered keys, then bevr_attn_cell_fwd on the sorted
 * ones with (O_in, LSE_in) = the first call's (O, LSE plane 0): the result is the softmax over both.  O_in == NULL:
 * a single segment.  The backward entry points of both segments take the FINAL LSE and delta;
 * bevr_attn_cell_bwd_q ADDS its share to dQ and dtable (call it after bevr_attn_bwd_q, or on zeroed buffers).
 *   O_in [n_prob][heads][Mp][32] float, LSE_in [n_prob][heads][Mp] float; O, LSE as bevr_attn_fwd (LSE: 2 planes). */
int bevr_attn_cell_fwd(const bevr_attn_desc* d, const void* Q, const void* K, const void* Vt,
                       const void* key_ws, const float* table_pair, const float* O_in, const float* LSE_in,
                       float* O, float* LSE, void* stream);
int bevr_attn_cell_bwd_q(const bevr_attn_desc* d, const void* Q, const void* K, const void* Kt, const void* V,
                         const void* key_ws, const float* table_pair, const void* dO, const float* LSE,
                         const float* delta, const float* grad_scale, float* dQ, float* dtable, void* stream);
/* dK, dV written; dkey_a, dkey_b ACCUMULATED (as bevr_attn_bwd_k). */
int bevr_attn_cell_bwd_k(const bevr_attn_desc* d, const void* Q, const void* Qt, const void* K, const void* V,
                         const void* key_ws, const float* table_pair, const void* dO, const void* dOt,
                         const float* LSE, const float* delta, const float* grad_scale, float* dK, float* dV,
                         float* dkey_a, float* dkey_b, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TAP entry points (csrc/attn_tap.h): the same attention for a key segment whose keys all SAMPLE INSIDE THE TOP-LEFT
 * 4 x 3 PIXELS of their feature map -- the pillar points a camera does not see: the projector pins them to pixel (0, 0)
 * (model/bev_cmr_proj.py:76) and the learned offset moves them by less than +-2.5 (Hi-1)/(Hk-1) x +-2.5 (Wi-1)/(Wk-1)
 * pixels (model/SCA_deform_attn.py:261-277).  For those keys K_n = sum_t w_t(n) Kpix_t + bk and V_n alike (bilinear
 * weights w_t over the 12 pixels t = 3 r + c; proj_k / proj_v are linear), so K and V are never formed:
 *   logits  S[n][q] = sum_t w_t(n) G[t][q] + Gb[q] + bias[n][q],     G[t][q] = Q_q . Kpix_t (Q pre-scaled), Gb = Q_q . bk
 *   output  O_q     = sum_t Rn[t][q] Vpix_t + bv,                    Rn = R / R[15],  R[t][q] = sum_n w_t(n) P[n][q]
 * The caller forms G, Gb (thin GEMMs) before and O after the launch, and merges the segment with the other keys of the
 * same softmax through (mref, R[15]): the segment's log2-sum-exp is mref[q] + log2 R[15][q].
 * Geometry, table, descriptor (groups == 1, precision BEVR_PREC_BF16 or BEVR_PREC_F16 -- E below; BEVR_PREC_BF16X3 with
 * the operand format at the end of this comment) as above; keys cell-sorted for
 * speed (any key set is handled: a 32-key run that does not fit one table chunk is processed in several masked passes).
 *   key_a, key_b, key_y, key_x [n_prob][Np] float: table coordinates as above; sampling position in FEATURE PIXELS
 *       ys = (py + 1)/2 (Hi - 1), xs likewise (ys < 3 and xs < 2 or outside the image: the caller's contract)
 *   tap_ws: bevr_attn_tap_ws_bytes(d) bytes, written by bevr_attn_tap_prep, opaque
 *   G   [n_prob][heads][Mp][16] E: slots 0..11 the taps; slots 12, 13 the hi and lo 16-bit parts of the row's logit
 *       offset c = Gb[q] - mref[q] (hi = E(c), lo = E(c - hi): the matrix product adds them against ones on the key side);
 *       slot 14 = -1e30 (E = bf16) / -60000 (fp16): the logit of a masked key; slot 15 zero
 *   mref [n_prob][heads][Mp] float IN/OUT: the softmax reference of each row, AS THE KERNEL SEES IT (Gb - (hi + lo)).  In:
 *       an upper bound of the row's logits minus a HEADROOM (bevrender_amd/ops.py uses max(0, max_t G) + Gb +
 *       max(0, max table) - 64).  The weights 2^(S - mref) <= 2^headroom are rounded to the operand type E before the R
 *       product, so the headroom is bounded per precision: BEVR_PREC_BF16 <= 100 (8 exponent bits), BEVR_PREC_F16 <= 8
 *       (5 exponent bits: 2^15.9 is fp16's largest value; the row sum over up to 2^17 keys is taken in f32.  A larger fp16
 *       headroom gives inf / NaN in R -- the kernel cannot see the headroom, the limit is the caller's to keep;
 *       tools/tap_check.py and bevrender_amd/ops.py (TAP_HEADROOM_F16) run fp16 at 8).  Out: the reference R is relative
 *       to -- unchanged unless every weight of the row underflowed against the bound (looser than ~190 binades), in which
 *       case the column is recomputed with an online maximum and its rows' mref are replaced.
 *       BEVR_PREC_F16 flags sooner: an fp16 weight under 2^-14 is stored with an absolute error of up to 2^-25 (zero under
 *       2^-25), Np keys move a row's sum by up to Np 2^-25, so a column is recomputed as soon as one of its rows has a sum
 *       R[15] under Np 2^-14 (the error could exceed 2^-11 of the sum; with headroom 8 and Np keys: a bound more than
 *       ~22 - log2 Np binades above the row's log2-sum-exp).  The _dropout entry point applies this to the sum of ALL
 *       weights (lsum), bevr_attn_tap_g2_fwd to its R[15].  The recompute keeps every weight <= 1 against the running
 *       maximum.
 *   R   [n_prob][heads][Mp][16] float (written; rows 12, 13 equal row 15)   flags [n_prob*heads][S] int32, ZEROED by the
 *       caller (scratch)
 *
 * TAP entry points in BEVR_PREC_BF16X3 (bevr_attn_tap_fwd, _bwd_q, _bwd_k; the _dropout entry points and BEVR_PREC_F32
 * return BEVR_E_PRECISION -- the mode's keep mask has entry points of its own, bevr_attn_tap_*_x3_dropout below;
 * bevr_attn_tap_prep and bevr_attn_tap_ws_bytes do not look at the precision).  The CALLER
 * splits G and H; the kernels split what they form themselves (tap and bias-cell weights, the table's chunk, P and dS)
 * and multiply in three bf16 products, lo hi + hi lo + hi hi (the logit contraction in all four), everything per pair in f32.  tap_ws, tables, mref, R,
 * flags, dG, dtable, dkey_* are as in the 16-bit modes (float).
 *   G, H  [2][n_prob][heads][Mp][16] bf16: plane 0 = hi, plane 1 = lo (the lo plane n_prob * heads * Mp * 32 bytes behind
 *       the hi plane), both round-to-nearest-even:
 *         slots 0..11: x = the float tap value,  hi = bf16(x), lo = bf16(x - hi)      (hi + lo = x to 2^-17 relative)
 *         slots 12, 13: the row offset c (G: Gb - mref in bevr_attn_tap_fwd, Gb - LSE in the backward; H: Hc) in FOUR
 *           parts, p0 = bf16(c), p1 = bf16(c - p0), p2 = bf16(c - p0 - p1), p3 = bf16(c - p0 - p1 - p2):
 *           slot 12 = (hi p0, lo p1), slot 13 = (hi p2, lo p3).  The key side holds 1 = (hi 1, lo 0) in both slots, so
 *           the product adds p0 + p1 + p2 + p3 = c to the float's last bit: the large constant part of every logit does
 *           not go through the three-term product's 2^-16
 *         slot 14: G hi = -1e30 (the logit of a masked key), lo = 0; H zero.   slot 15: zero
 *       (bevrender_amd/ops.py:tap_split_rows is this builder.)
 *   mref as above: the reference AS THE KERNEL SEES IT, Gb - (p0 + p1 + p2 + p3).  The weights 2^(S - mref) are split into
 *       bf16 hi + lo before the R product: headroom <= 100 as for BEVR_PREC_BF16 (bf16 has the float's exponent range).
 * ---------------------------------------------------------------------------------------------- */
size_t bevr_attn_tap_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_tap_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const float* key_y,
                       const float* key_x, void* tap_ws, void* stream);
int bevr_attn_tap_fwd(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair, float* mref,
                      float* R, int32_t* flags, void* stream);
/* Query-side backward.  With P[n][q] = exp2(S[n][q] - LSE[q]) (LSE: the log2-sum-exp over ALL key segments of the softmax):
 *     dS[n][q] = P[n][q] (sum_t w_t(n) H[t][q] + Hc[q]),     dG[k][q] = sum_n A[n][k] dS[n][q]   (A = the 16 slot weights)
 *   G as above with the offset c = Gb - LSE in slots 12, 13 (padding rows i >= S: c <= -1e30, their weights vanish)
 *   H  [n_prob][heads][Mp][16] E = ln2 * (dO_q . Vpix_t) in slots 0..11, the hi and lo parts of Hc = ln2 * (dO_q . bv - delta_q)
 *      in slots 12, 13, zero in 14, 15
 *   dG [n_prob][heads][Mp][16] float WRITTEN: slots 0..11 the gradient of G, slot 15 the gradient of Gb
 *   dtable as bevr_attn_bwd_q: ACCUMULATED (float atomics). */
int bevr_attn_tap_bwd_q(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                        const float* table_pair, float* dG, float* dtable, void* stream);
/* Key-side backward: the gradients of every key's table coordinates and sampling position (G, H as bevr_attn_tap_bwd_q),
 *   dkey_a, dkey_b, dkey_y, dkey_x [n_prob][Np] float, ACCUMULATED over the heads (caller zeroes them):
 *   d/d key_a, d/d key_b through the bias (bilinear derivative of the table), d/d key_y, d/d key_x through the tap
 *   weights -- both paths of it: the logits (G) and the values (sum_q P H / ln2: H carries ln2 dO . Vpix).  Kinks as F.grid_sample's backward
 *   (floor-based: the derivative of the tap pair the position sits between). */
/* NOTE the table operand: NOT the pair table of the other entry points but the PLAIN packed table
 *   table [heads][Wp][Hp + 1] float, table[h][x][y] = log2(e) * rpe_table[h][y - y_off][x - x_off], zero in the padding --
 *   the transposed, padded table the pair table is built from and the buffer `dtable` mirrors (row pitch Hp + 1).  The
 *   kernel differences it along both axes in hi + lo 16-bit parts; handing it the (h, Wp, Hp, 2) pair table gives silently
 *   wrong dkey_a / dkey_b (tests/test_gpu_tap.py::test_tap_bwd_k_through_the_c_abi_as_the_header_describes). */
int bevr_attn_tap_bwd_k(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                        const float* table, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x, void* stream);

/* bevr_attn_tap_bwd_k with the (32-key tile, BEV column) pairs whose taps do not fit one table chunk dispatched from a
 * device work list: the main launch appends each tile that has such a column to `ws`, and a second launch of a FIXED
 * number of waves claims (listed tile, range of BEV columns) items -- instead of the whole grid launched again to look
 * for them.  BEVR_PREC_BF16 and BEVR_PREC_F16 (BEVR_PREC_BF16X3: BEVR_E_PRECISION -- the split mode and the dropout
 * variant keep the entry points without a work list).  Same arguments and results as bevr_attn_tap_bwd_k up to the
 * order of the float atomics every dkey_* is summed with.
 *   ws              device scratch of bevr_attn_tap_bwd_k_ws_bytes(d) bytes, 16-byte aligned: two counters and one int
 *                   per (problem-head, tile).  The entry point clears the counters on `stream` itself; the contents
 *                   afterwards are unspecified.  One ws per call in flight.
 *   max_workgroups  0: as many workgroups (of four waves) as the device holds at once; > 0: at most that many.
 *                   < 0: BEVR_E_SHAPE. */
size_t bevr_attn_tap_bwd_k_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_tap_bwd_k_ws(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                           const float* table, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                           void* ws, int max_workgroups, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TAP entry points for TWO CHANNEL GROUPS (csrc/attn_tap_*_g2.hip; descriptor groups == 2 and an even number of heads,
 * else BEVR_E_SHAPE; BEVR_PREC_BF16 or BEVR_PREC_F16, else BEVR_E_PRECISION; no keep mask).  Added without a new ABI
 * version: nothing a version-6 caller uses changed, and the entry points above keep returning BEVR_E_SHAPE for
 * groups != 1.  With n_groups = 2 (model/SCA_deform_attn.py:290-321) group g' samples its C / 2 channels at its OWN
 * position, proj_k / proj_v mix all channels, and the bias of a head uses the positions of the head's group
 * g = head / (heads / 2).  For a pinned key n and a head of group g
 *   logits  S[n][q] = sum_g' sum_t w_t^g'(n) G^g'[t][q] + Gb[q] + bias^g[n][q],   G^g'[t][q] = Q_q . Kpix_t^g',
 *                     Kpix_t^g' = Wk[:, channels of g'] f_t[channels of g']   (the 12 pixels' rows, per channel group)
 *   output  O_q     = sum_g' sum_t Rn^g'[t][q] Vpix_t^g' + bv,    R^g'[t][q] = sum_n w_t^g'(n) P[n][q],  Rn = R / R[15]
 * A softmax does not care about the order of its keys, and a head needs (a, b) of its own group only: every
 * (problem, group) ROW p * 2 + g has a key order of its own -- the caller's choice; cell-sorted by group g's table
 * coordinates for speed, as above -- and holds, for the key at each index of THAT order, group g's table coordinates
 * and the sampling positions of BOTH groups.  Head hd reads the records of row prob * 2 + hd / (heads / 2).
 *   key_a, key_b [n_prob * 2][Np] float: row p * 2 + g = group g's table coordinates, in the row's own key order
 *   key_y, key_x [n_prob * 2][2][Np] float: plane g' of row p * 2 + g = the sampling position in feature pixels of group
 *       g' for the key at that index of row p * 2 + g's order (both inside the 4 x 3 pixels: the contract above, for
 *       either group; the bounds-checking build traps a live key of either group outside them)
 *   tap_ws: bevr_attn_tap_g2_ws_bytes(d) bytes (0: bad descriptor), written by bevr_attn_tap_g2_prep, opaque; records
 *       and tile boxes per (problem, group) row
 *   G   [n_prob][heads][Mp][32] E: slots 0..15 EXACTLY the one-group layout with group 0's taps (12, 13 the row offset,
 *       14 the masked key's logit, 15 zero); slots 16..27 group 1's taps; slots 28..31 ZERO
 *   mref, flags, table_pair, table, dtable: as for the one-group entry points.  The static reference needs the bound
 *       sum_g' max(0, max_t G^g'[t][q]) + Gb + max(0, max table): a SUM over the groups (each group's tap weights are
 *       convex up to zero padding), not a maximum.  Flagged columns are recomputed with an online maximum as above.
 *   R   [n_prob][heads][Mp][32] float (written): rows 0..15 as above (row 15 the denominator), rows 16..27 group 1's
 *       weight sums, rows 28..31 zero
 *   H, dG [..][Mp][32] in the same layout: H slots 0..11 and 16..27 = ln2 * (dO_q . Vpix_t^g'), 12, 13 the parts of Hc,
 *       the others zero; dG slots 0..11 and 16..27 the gradient of G, slot 15 the gradient of Gb
 *   dkey_a, dkey_b [n_prob * 2][Np], dkey_y, dkey_x [n_prob * 2][2][Np] float, in the rows' key orders, ACCUMULATED over
 *       the heads of the row's group (caller zeroes them): d/d key_a, key_b through the bias of those heads; plane g' of
 *       d/d key_y, key_x through group g''s tap weights, both paths (logits and values) as bevr_attn_tap_bwd_k.  The
 *       gradient of a key's position of group g' is the sum over BOTH rows' planes g' (after undoing the rows' orders).
 *       (tile, column) pairs that do not fit a table chunk are taken by the main grid launched again: no work list.
 * The second logit product is one more zero-padded depth-32 matrix product per 16 keys x 16 rows.
 * ---------------------------------------------------------------------------------------------- */
size_t bevr_attn_tap_g2_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_tap_g2_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const float* key_y,
                          const float* key_x, void* tap_ws, void* stream);
int bevr_attn_tap_g2_fwd(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair,
                         float* mref, float* R, int32_t* flags, void* stream);
int bevr_attn_tap_g2_bwd_q(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                           const float* table_pair, float* dG, float* dtable, void* stream);
int bevr_attn_tap_g2_bwd_k(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                           const float* table, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x, void* stream);

/* Attention dropout on the tap entry points: the three above with the keep mask of bevr_attn_*_dropout (same hash, same
 * drop_thr = round(p * 65536) < 65536, BEVR_E_SHAPE otherwise).  The pair (ph, mq, key n' of this segment) is hashed
 * with n = key0 + n': key0 is the index of the segment's first key in the caller's key order for the whole call, so
 * that a region segment [0, split) (bevr_attn_*_dropout, which hash from 0) and a tap segment [split, N) with
 * key0 = split evaluate ONE mask over all N keys (bevrender_amd/ops.py:dropout_keep_mask(seed, thr, n_ph, S, N)).  A
 * key that is emitted in several masked passes (a run that does not fit one table chunk) has one keep decision.
 * Dropout acts on the weights after the softmax and the tap formulation is linear in them:
 *   forward   R[slot][q] = sum_n keep w_slot(n) 2^(S[n][q] - mref[q]): the KEPT weights; rows 12, 13, 15 are the kept
 *             mass, not the denominator.  lsum [n_prob][heads][Mp] float WRITTEN: sum_n 2^(S[n][q] - mref[q]) over ALL
 *             keys (the segment's log2-sum-exp is mref + log2 lsum; the mask does not enter it, and the recompute of
 *             underflowed rows is decided on it).  The caller normalises and applies D = 65536 / (65536 - drop_thr):
 *             Rn' = D R[0..11] / lsum, kept mass m' = D R[15] / lsum, O = Rn' Vpix + m' bv.
 *   backward  dS[n][q] = P[n][q] (keep ? sum_t w_t(n) H[t][q] + H[15][q] : 0  +  Hc[q])
 *             H slots 0..11 = D ln2 (dO_q . Vpix_t), slot 15 = D ln2 (dO_q . bv) (the cotangent of the kept mass: the
 *             droppable part of the constant, ONE 16-bit value as the taps'), slots 12, 13 the hi and lo parts of
 *             Hc = -ln2 delta_q (never dropped), slot 14 zero.  delta = sum_n P keep D dP - dLSE: rowsum(dO * O) of the
 *             merged softmax as for the region entry points.  The caller folds D into H; the fp16 operands then carry
 *             D times the cotangent and the caller's power-of-two scaling must leave room for it.
 *             bevr_attn_tap_bwd_k_dropout takes the value path sum_q keep P H / ln2 from the kept weights.
 *   G, tap_ws, tables, dG, dtable, dkey_* as for the entry points above. */
int bevr_attn_tap_fwd_dropout(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair,
                              float* mref, float* R, float* lsum, int32_t* flags, unsigned key0, unsigned drop_thr,
                              unsigned drop_seed, void* stream);
int bevr_attn_tap_bwd_q_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                const float* table_pair, float* dG, float* dtable, unsigned key0, unsigned drop_thr,
                                unsigned drop_seed, void* stream);
int bevr_attn_tap_bwd_k_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                const float* table, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                                unsigned key0, unsigned drop_thr, unsigned drop_seed, void* stream);

/* Attention dropout on the TAP entry points in BEVR_PREC_BF16X3: the three _dropout entry points above in split
 * arithmetic, entry points of their own.  Arguments, checks (in the same order) and semantics are those of
 * bevr_attn_tap_*_dropout; the operands are those of "TAP entry points in BEVR_PREC_BF16X3"; every precision but
 * BEVR_PREC_BF16X3 returns BEVR_E_PRECISION.  The operand words that differ from either:
 *   G, H   the two bf16 planes [2][n_prob][heads][Mp][16] (hi, lo), slots 0..14 as in the split mode without dropout:
 *          H slots 0..11 = D ln2 (dO_q . Vpix_t) as hi = bf16(x), lo = bf16(x - hi); slots 12, 13 the FOUR bf16 parts of
 *          Hc = -ln2 delta_q, slot 12 = (hi p0, lo p1), slot 13 = (hi p2, lo p3), never dropped: a dropped pair keeps
 *          p0 + p1 + p2 + p3, read by the kernel from both planes and summed smallest first; slot 14 zero
 *   H slot 15   D ln2 (dO_q . bv), the cotangent of the kept mass (droppable): where the 16-bit dropout entry points take
 *          ONE 16-bit value, here the slot carries a value in BOTH planes, hi = bf16(x) and lo = bf16(x - hi), against the
 *          key side's w = 1 = (hi 1, lo 0): the product adds hi + lo (x to 2^-17 relative).  The caller's delta must use
 *          that sum.  G slot 15 stays zero
 *   lsum   [n_prob][heads][Mp] float WRITTEN: sum_n 2^(S[n][q] - mref[q]) over ALL keys, summed in float from the weights
 *          before they are split; R (float) holds the kept weights, rows 12, 13, 15 the kept mass.  Columns are flagged on
 *          lsum and recomputed with an online maximum, which rewrites R, lsum and mref of the flagged columns
 *   key0, drop_thr, drop_seed   as above: the same hash at key0 + n', one keep decision per key over masked passes, so a
 *          region segment (bevr_attn_*_dropout in BEVR_PREC_BF16X3) and a tap segment with key0 = split share ONE mask
 * bevr_attn_tap_bwd_k_x3_dropout launches its main grid again for the pairs that miss the table window (no work list). */
int bevr_attn_tap_fwd_x3_dropout(const bevr_attn_desc* d, const void* G, const void* tap_ws, const float* table_pair,
                                 float* mref, float* R, float* lsum, int32_t* flags, unsigned key0, unsigned drop_thr,
                                 unsigned drop_seed, void* stream);
int bevr_attn_tap_bwd_q_x3_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                   const float* table_pair, float* dG, float* dtable, unsigned key0, unsigned drop_thr,
                                   unsigned drop_seed, void* stream);
int bevr_attn_tap_bwd_k_x3_dropout(const bevr_attn_desc* d, const void* G, const void* H, const void* tap_ws,
                                   const float* table, float* dkey_a, float* dkey_b, float* dkey_y, float* dkey_x,
                                   unsigned key0, unsigned drop_thr, unsigned drop_seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gather kernel: the FORWARD of bevr_attn_fwd for SCATTERED keys with the relative-position bias on the matrix cores
 * (csrc/attn_gather_fwd.hip: a sparse contraction whose table side the lanes gather from an LDS window of the table;
 * any key set is handled; there is no gather backward: bevr_attn_bwd_q / _bwd_k or the slab entry point below take the
 * same operands).  BEVR_PREC_BF16 or BEVR_PREC_F16 (any other: BEVR_E_PRECISION), S <= 224 (a window column holds a key's
 * taps for every BEV row of a column; taller: BEVR_E_SHAPE, see bevr_attn_gather_fwd_rows).  Replaces model/SCA_deform_attn.py:331-413 and
 * model/TSA_deform_attn.py:245-333 (reference) like the entry points above.
 *   Q, K, key_ws, O, LSE: as bevr_attn_fwd        V [n_prob][heads][Np][32] rows of the operand type (not transposed)
 *   table_pk [heads][Wp][Hp] dwords: the pair table in the operand type (bf16 / fp16; the key-side bilinear weights are
 *            rounded to it too, as in that mode's other kernels), (T2[y - y_off][x - x_off], T2[y + 1 - y_off][x - x_off]),
 *            round-to-nearest of table_pair
 *   mref [n_prob][heads][Mp] float: the softmax reference of every row, as bevr_attn_tap_fwd's -- an upper bound of the
 *            row's logits minus a headroom (64 binades); rows whose weights all underflow against it (bound looser than
 *            ~160 binades) are recomputed with an online maximum: flags [n_prob * heads][S] int, zeroed by the caller,
 *            marks their columns (scratch: this call's static pass writes it, its exact pass reads it).
 *            BEVR_PREC_F16: headroom <= 8 as for bevr_attn_tap_fwd, and 5 exponent bits make the static reference useful
 *            only near the bound -- a weight under 2^-14 is stored with an absolute error of up to 2^-25 (zero under
 *            2^-25), N keys move a row's sum by up to N 2^-25, so a row whose LARGEST weight is under N 2^-14 (the error
 *            could exceed 2^-11 of the sum) flags its column too.  The exact pass keeps its reference 8 binades under
 *            the running maximum and moves it when a logit exceeds it by 15 binades (bf16: 0 and 40).
 * LSE plane 1 is log2 of an upper bound (within 2 binades) of the row's largest softmax weight. */
int bevr_attn_gather_fwd(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                         const void* key_ws, const void* table_pk, const float* mref, float* O, float* LSE,
                         int* flags, void* stream);
/* The same over the BEV rows [row0, row0 + n_rows) of every BEV column of every (problem, head), for any S that
 * bevr_check_desc accepts: query rows are independent, so a tall column is computed as bands.  Operands and precisions
 * as above (checked in the same order), then row0 >= 0, row0 % 16 == 0, 1 <= n_rows <= 224, row0 + n_rows <= S, else
 * BEVR_E_SHAPE.  O and both LSE planes of rows outside the range are not touched; the call with row0 + n_rows == S
 * also writes the padding rows S .. Sp - 1 of each column as bevr_attn_gather_fwd does (LSE finite there: rows that no
 * 16-row block covers take the last block's values), with one floor: the LSE copied into an uncovered padding row is at
 * least mref of that row - 36 (bf16; never reached by rows of ordinary size) or mref + 70 (fp16; both entry points), so
 * that 2^(bias - LSE), which bevr_attn_bwd_k forms for the zero Q rows there, cannot overflow its operand type.
 * flags [n_prob * heads][S] int is zeroed by the caller before EVERY call. */
int bevr_attn_gather_fwd_rows(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                              const void* key_ws, const void* table_pk, const float* mref, float* O, float* LSE,
                              int* flags, int row0, int n_rows, void* stream);
/* The gather forward in BEVR_PREC_BF16X3 (csrc/attn_gather_fwd_x3.hip: every product three bf16 MFMAs on hi + lo parts,
 * f32 tolerance), over the BEV rows [row0, row0 + n_rows) of every column; a whole column of S <= 224 rows is the range
 * (0, S).  Outputs, mref, flags, the padding rows (LSE floor mref - 36) and the row-range contract as
 * bevr_attn_gather_fwd_rows in bf16; the band limit is 224 rows.  Checked in this order: the descriptor, NULL pointers,
 * 16-byte alignment of Q / K / V / key_ws / O, the precision (any but BEVR_PREC_BF16X3: BEVR_E_PRECISION), the row range
 * (row0 >= 0, row0 % 16 == 0, 1 <= n_rows <= 224, row0 + n_rows <= S, else BEVR_E_SHAPE).  Operands:
 *   Q [n_prob / q_div][heads][Mp][32], K, V [n_prob][heads][Np][32]: float CONTAINERS in the split ROW format of this
 *            mode's other entry points (bevr_pack_kv with BEVR_PREC_BF16X3 writes K and V): a row is 128 bytes, per
 *            16-element half  hi(e0..7) | hi(e8..15) | lo(e0..7) | lo(e8..15)  bf16, hi = bf16(x), lo = bf16(x - hi).
 *            V rows are not transposed.
 *   table_pk2 [2][heads][Wp][Hp] dwords: plane 0 the bf16 pairs (hi(T2[y][x]), hi(T2[y + 1][x])) of the f32 pair table
 *            table_pair, plane 1 the pairs of the lo parts, lo = bf16(T2 - hi(T2)), both round-to-nearest
 *   key_ws, mref (headroom 64), O, LSE, flags: as bevr_attn_gather_fwd in bf16 (flags zeroed by the caller before EVERY
 *            call); the key-side bilinear weights are computed in f32 and split like every other operand.
 * Uses 152 KB of dynamic LDS (one workgroup per CU). */
int bevr_attn_gather_fwd_x3(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                            const void* key_ws, const void* table_pk2, const float* mref, float* O, float* LSE,
                            int* flags, int row0, int n_rows, void* stream);
/* bevr_attn_gather_fwd_rows with the keep mask of bevr_attn_fwd_dropout (csrc/attn_gather_fwd_drop.hip), over the BEV rows
 * [row0, row0 + n_rows) of every column; a whole column of S <= 224 rows is the range (0, S).  Operands, the order of the
 * checks, the row-range contract, flags and the padding rows as bevr_attn_gather_fwd_rows (BEVR_PREC_BF16 and
 * BEVR_PREC_F16; else BEVR_E_PRECISION); drop_thr = round(p * 65536) < 65536, else BEVR_E_SHAPE (checked first).  Pair
 * (ph, mq, n) is kept iff the hash of "Attention dropout" above says so, with n the key's index in the caller's key order
 * (K's row) and mq = j * Sp + i of the ABSOLUTE BEV row i, whichever band the call computes: the bands of a column, the
 * masked strip emissions of a wide key tile and the second pass over flagged columns all evaluate one mask.  Semantics of
 * bevr_attn_fwd_dropout: softmax first -- both LSE planes and the row sum are of ALL the (rounded) weights and equal
 * those of bevr_attn_gather_fwd_rows --, the product with V contracts the kept weights, and D = 65536 / (65536 - drop_thr)
 * multiplies O after the normalisation (the fp16 operands stay the unscaled weights). */
int bevr_attn_gather_fwd_dropout(const bevr_attn_desc* d, const void* Q, const void* K, const void* V,
                                 const void* key_ws, const void* table_pk, const float* mref, float* O, float* LSE,
                                 int* flags, int row0, int n_rows, unsigned drop_thr, unsigned drop_seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SLAB entry points (csrc/attn_slab_bwd_q.hip): bevr_attn_bwd_q -- dQ and the rpe-table gradient of a key segment, same
 * arithmetic per (query, key) pair, same operands and gradient semantics -- with the work cut along the TABLE: a work item
 * owns a slab of <= 24 consecutive table columns of one (problem, head), all rows of them in LDS (values and 64-bit
 * fixed-point gradient cells), and processes the pairs whose left tap column floor(j rx + b_n) falls into the slab; the
 * keys are handed over SORTED BY b per problem, so those are one contiguous run per BEV column.  Every table cell leaves
 * the workgroup once per item (no moving window, no flush traffic to speak of); dQ leaves as float atomics.
 * 16-bit operand modes (BEVR_PREC_BF16, BEVR_PREC_F16), S <= 211; BEVR_E_SHAPE / BEVR_E_PRECISION otherwise (the caller
 * keeps bevr_attn_bwd_q: bevrender_amd/ops.py:slab_supported).  Any key set is handled.
 *   order  [n_prob*groups][N] int32: per problem-group, a permutation of 0..N-1 that sorts key_b ascending
 *   Ks, Vs [n_prob][heads][N][32] E: the K / V rows IN THAT ORDER (row t of (prob, head) = key order[pg][t]), unpadded
 *   slab_ws: bevr_attn_slab_ws_bytes(d) bytes (0: unsupported shape), written by bevr_attn_slab_prep, opaque; a launch
 *           resets the work list's item counter on its stream before it starts, so launches that follow one another on
 *           a stream may share a prep (the launches of one workspace must not overlap: they share that counter)
 *   Q, table_pair, dO, LSE, delta, grad_scale: as bevr_attn_bwd_q
 *   dQ [n_prob][heads][Mp][32] float ACCUMULATED with float atomics (caller zeroes; bevr_attn_bwd_q WRITES its dQ)
 *   dtable ACCUMULATED (as bevr_attn_bwd_q)
 * ---------------------------------------------------------------------------------------------- */
size_t bevr_attn_slab_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                        void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs, const void* slab_ws,
                         const float* table_pair, const void* dO, const float* LSE, const float* delta,
                         const float* grad_scale, float* dQ, float* dtable, void* stream);
/* The same for any S <= 448, over the BEV rows [row0, row0 + n_rows) of every BEV column (csrc/attn_slab_bwd_q_rows.hip:
 * the same kernel with a taller slab column and seven worker waves that take the row blocks row0 / 31 ... of a column).
 * The slab keeps EVERY table row the whole column can reach, whichever band is computed -- a pair's table row depends on
 * the key and the query row alone -- so the bands of a column are independent launches that add into the same dQ
 * (disjoint rows) and dtable: all of them together are bevr_attn_slab_bwd_q's result.  The slab is narrower for it
 * (12 table columns up to S = 403, 10 above), and every band fills the slabs and streams the sorted K / V rows again.
 *   bevr_attn_slab_rows_ws_bytes / _slab_rows_prep: as bevr_attn_slab_ws_bytes / _slab_prep, for this kernel's slab width
 *           (0 / BEVR_E_SHAPE for S > 448, 0 / BEVR_E_PRECISION for a mode that is not 16-bit); the two workspaces are
 *           not interchangeable.  ONE prep serves all bands of a call (launched one after another on a stream: see
 *           slab_ws above).
 *   bevr_attn_slab_bwd_q_rows: operands and checks of bevr_attn_slab_bwd_q, in its order (NULL, precision, shape,
 *           alignment); the shape check also asks for row0 >= 0, row0 % 31 == 0, 1 <= n_rows <= 217 (seven row blocks of
 *           31), row0 + n_rows <= S, and n_rows % 31 == 0 unless row0 + n_rows == S; else BEVR_E_SHAPE.  dQ of rows
 *           outside the range is not touched.  bevrender_amd/ops.py:slab_bands cuts a column into such bands. */
size_t bevr_attn_slab_rows_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_rows_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                             void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q_rows(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs, const void* slab_ws,
                              const float* table_pair, const void* dO, const float* LSE, const float* delta,
                              const float* grad_scale, float* dQ, float* dtable, int row0, int n_rows, void* stream);
/* The same in BEVR_PREC_BF16X3 (csrc/attn_slab_bwd_q_x3.hip: the three matrix products as three-term split-bf16 products,
 * bias taps and table gradient per pair in f32), S <= 211.  A slab cell is the f32 pair and the gradient cell, 16 bytes,
 * so the slab is narrower (15 table columns against 24) and the workspace has entry points of its own.
 *   bevr_attn_slab_x3_ws_bytes / _slab_x3_prep: as bevr_attn_slab_ws_bytes / _slab_prep, for this kernel's slab width
 *           (0 / BEVR_E_SHAPE for S > 211, 0 / BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3); not interchangeable
 *           with the other slab workspaces.
 *   bevr_attn_slab_bwd_q_x3: operands and checks of bevr_attn_slab_bwd_q, in its order (NULL, precision, shape,
 *           alignment).  Q, Ks, Vs and dO are the mode's 128-byte split rows (hi and lo bf16 images per 16-element half,
 *           as bevr_attn_bwd_q takes Q, K and dO in this mode; Ks / Vs: the K / V rows of bevr_pack_kv in the sorted order),
 *           table_pair the f32 pair table.  BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3. */
size_t bevr_attn_slab_x3_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_x3_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                           void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q_x3(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs, const void* slab_ws,
                            const float* table_pair, const void* dO, const float* LSE, const float* delta,
                            const float* grad_scale, float* dQ, float* dtable, void* stream);
/* bevr_attn_slab_bwd_q_x3 for any 2 <= S <= 448 (S < 2 is no side of any descriptor: BEVR_E_SHAPE from the descriptor check,
 * as everywhere), over the BEV rows [row0, row0 + n_rows) of every BEV column
 * (csrc/attn_slab_bwd_q_x3_rows.hip: the split-bf16 kernel with the taller slab columns and the band of row blocks of
 * bevr_attn_slab_bwd_q_rows).  The slab again keeps every table row the whole column can reach, so the bands of a column
 * are independent launches that add into the same dQ (disjoint rows) and dtable; all of them together are
 * bevr_attn_slab_bwd_q_x3's result where that one exists (S <= 211), up to the order of the float atomics.  With 16-byte
 * cells the slab owns 7 table columns up to S = 403 and 6 above; every band fills the slabs and streams the sorted
 * K / V rows again.  No keep mask.
 *   bevr_attn_slab_x3_rows_ws_bytes / _slab_x3_rows_prep: as bevr_attn_slab_ws_bytes / _slab_prep, for this kernel's slab
 *           width (0 / BEVR_E_SHAPE for S > 448, 0 / BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3); not
 *           interchangeable with the other slab workspaces.  ONE prep serves all bands of a call (launched one after
 *           another on a stream: a launch resets the work list's item counter itself, see slab_ws above).
 *   bevr_attn_slab_bwd_q_x3_rows: operands of bevr_attn_slab_bwd_q_x3 (128-byte split rows, the f32 pair table, gscale
 *           folded as there), then (row0, n_rows) as bevr_attn_slab_bwd_q_rows takes them.  Checks in that entry point's
 *           order: NULL, precision (BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3), shape (2 <= S <= 448, and row0 >= 0,
 *           row0 % 31 == 0, 1 <= n_rows <= 217, row0 + n_rows <= S, n_rows % 31 == 0 unless row0 + n_rows == S; else
 *           BEVR_E_SHAPE), alignment.  dQ of rows outside the range is not touched.  bevr_attn_slab_bwd_q_rows keeps
 *           answering BEVR_E_PRECISION to this mode and bevr_attn_slab_bwd_q_x3 BEVR_E_SHAPE to S > 211. */
size_t bevr_attn_slab_x3_rows_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_x3_rows_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                                void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q_x3_rows(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs,
                                 const void* slab_ws, const float* table_pair, const void* dO, const float* LSE,
                                 const float* delta, const float* grad_scale, float* dQ, float* dtable, int row0,
                                 int n_rows, void* stream);
/* bevr_attn_slab_bwd_q with the keep mask of bevr_attn_bwd_q_dropout (csrc/attn_slab_bwd_q_drop.hip), 16-bit modes,
 * S <= 211.  The keys arrive sorted by b, and the mask is of the key's index in the CALLER's order, n = order[pg][t] for
 * sorted position t: the workspace carries that index, so it has entry points of its own.
 *   bevr_attn_slab_drop_ws_bytes / _slab_drop_prep: as bevr_attn_slab_ws_bytes / _slab_prep (same checks and results);
 *           not interchangeable with the other slab workspaces.
 *   bevr_attn_slab_bwd_q_dropout: operands and checks of bevr_attn_slab_bwd_q, in its order, after drop_thr < 65536
 *           (else BEVR_E_SHAPE).  Per pair dS = P (keep ? D dP - delta : -delta), D = 65536 / (65536 - drop_thr), applied
 *           by the kernel to the dP accumulator: dO is the UNSCALED cotangent (the operand bevr_attn_bwd_k_dropout takes)
 *           and delta = rowsum(dO * O) of it; grad_scale as for bevr_attn_bwd_q_dropout, every Pmax of the contract read
 *           as D Pmax (fp16: the c2 and headroom rules of "Attention dropout" above).  The result is that of
 *           bevr_attn_bwd_q_dropout on the same keys in the caller's order, up to the order of the float atomics and one
 *           rounding of the tap weights. */
size_t bevr_attn_slab_drop_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_drop_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                             void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q_dropout(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs,
                                 const void* slab_ws, const float* table_pair, const void* dO, const float* LSE,
                                 const float* delta, const float* grad_scale, float* dQ, float* dtable,
                                 unsigned drop_thr, unsigned drop_seed, void* stream);
/* bevr_attn_slab_bwd_q_x3 with the same keep mask (csrc/attn_slab_bwd_q_x3_drop.hip), BEVR_PREC_BF16X3, S <= 211.  The
 * mask is again of the key's index in the CALLER's order, carried by a workspace of this kernel's own.
 *   bevr_attn_slab_x3_drop_ws_bytes / _slab_x3_drop_prep: as bevr_attn_slab_x3_ws_bytes / _slab_x3_prep (same checks,
 *           same size, slab width and work list: the staged hash words leave the slab its 15 columns; 0 / BEVR_E_SHAPE
 *           for S > 211, 0 / BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3); not interchangeable with the other
 *           slab workspaces.
 *   bevr_attn_slab_bwd_q_x3_dropout: operands and checks of bevr_attn_slab_bwd_q_x3, in its order (NULL, precision,
 *           shape, alignment), after drop_thr < 65536 (else BEVR_E_SHAPE).  Per pair dS = P (keep ? D dP - delta :
 *           -delta), D = 65536 / (65536 - drop_thr), applied by the kernel to the dP accumulator: dO is the UNSCALED
 *           cotangent in the mode's split rows and delta = rowsum(dO * O) of the masked forward, grad_scale as for
 *           bevr_attn_bwd_q_dropout (every Pmax of the contract read as D Pmax) -- the operands bevr_attn_bwd_q_dropout
 *           takes in this mode.  The result is that kernel's on the same keys in the caller's order, up to the order of
 *           the float atomics.  BEVR_E_PRECISION for any mode but BEVR_PREC_BF16X3. */
size_t bevr_attn_slab_x3_drop_ws_bytes(const bevr_attn_desc* d);
int bevr_attn_slab_x3_drop_prep(const bevr_attn_desc* d, const float* key_a, const float* key_b, const int32_t* order,
                                void* slab_ws, void* stream);
int bevr_attn_slab_bwd_q_x3_dropout(const bevr_attn_desc* d, const void* Q, const void* Ks, const void* Vs,
                                    const void* slab_ws, const float* table_pair, const void* dO, const float* LSE,
                                    const float* delta, const float* grad_scale, float* dQ, float* dtable,
                                    unsigned drop_thr, unsigned drop_seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bilinear feature sampling, align_corners=True, zero padding (grid_sample semantics).
 *   feat [nb][Hi][Wi][C] float (channels-last)     pos [nb][N][2] float, (y, x) in [-1, 1] units
 *   out  [nb][N][C] float
 * backward: dfeat [nb][Hi][Wi][C] ACCUMULATED (caller zeroes), dpos [nb][N][2] written.
 * C must be a multiple of 4 and <= 1024.
 * ---------------------------------------------------------------------------------------------- */
int bevr_sample_fwd(const float* feat, const float* pos, float* out,
                    int nb, int Hi, int Wi, int C, int N, void* stream);
int bevr_sample_bwd(const float* feat, const float* pos, const float* dout, float* dfeat, float* dpos,
                    int nb, int Hi, int Wi, int C, int N, void* stream);
/* The same on a bf16 feature map (the backbone's output dtype in the bf16 configurations; `feat` = raw bf16 bits, same
 * shape): half the tap bytes, features stay bf16 in HBM.  out, dout, dfeat (the master gradient), dpos stay float. */
int bevr_sample_fwd_bf16(const void* feat, const float* pos, float* out,
                         int nb, int Hi, int Wi, int C, int N, void* stream);
int bevr_sample_bwd_bf16(const void* feat, const float* pos, const float* dout, float* dfeat, float* dpos,
                         int nb, int Hi, int Wi, int C, int N, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BEV pillar grid -> camera pixels (model/bev_cmr_proj.py:61-113).
 *   points_3d [4][P] float homogeneous IMU-frame points
 *   cam_inv   [ncam][4][4] float = inverse(imu_to_cam)       Kmat [ncam][3][3] float (already rescaled)
 *   out       [ncam][2][P] float, (x, y) normalised to [-1, 1]; points whose int-truncated pixel is
 *             outside [0, W-1) x [0, H-1) are pinned to pixel (0, 0) -> (-1, -1).
 * ---------------------------------------------------------------------------------------------- */
int bevr_project_bev_grid(const float* points_3d, const float* cam_inv, const float* Kmat, float* out,
                          int ncam, int P, int img_w, int img_h, void* stream);
/* The same with the optional grey-pixel mask of model/bev_cmr_proj.py:114-122 (remove_ref_in_gray):
 *   ref_img [ncam][ref_c][ref_h][ref_w] uint8 (device), one reference image per camera, ref_h >= img_h - 1,
 *   ref_w >= img_w - 1; a point whose truncated pixel has exactly three channels equal to 128 is pinned like an
 *   out-of-bound point.  ref_img == NULL: identical to bevr_project_bev_grid. */
int bevr_project_bev_grid_masked(const float* points_3d, const float* cam_inv, const float* Kmat, float* out,
                                 int ncam, int P, int img_w, int img_h, const uint8_t* ref_img, int ref_c,
                                 int ref_h, int ref_w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ground <-> aerial correlation: D[i][j] = 2 - 2 * <cam_i, map_j>  (train.py:554) on raw or
 * L2-normalised rows.   cam [n][E], map [m][E] float; D [n][m] float.
 *   normalize != 0: rows are L2-normalised first (the LpDistance(normalize_embeddings=True) of the
 *   retrieval losses); inv_norm_cam [n], inv_norm_map [m] receive 1/||row|| for the backward.
 *   n, m and E are any positive numbers, n != m included; D, the inverse norms and dD have no alignment contract.
 *   normalize == 0: inv_norm_cam and inv_norm_map are not looked at and may be NULL (in the backward D too).
 *   forward, E % 4 == 0: the rows are read as 16-byte vectors, so cam and map must be 16-byte aligned (BEVR_E_ALIGN
 *   otherwise, nothing is written); E % 4 != 0: no alignment contract.
 * backward: dcam [n][E], dmap [m][E] written from dD [n][m]; D, inv_norm_cam, inv_norm_map are the forward's (read only when
 *   normalize != 0).  No pointer has an alignment contract and no call returns BEVR_E_ALIGN: with cam, map, dcam or dmap
 *   off the 16-byte grid the backward runs on its scalar kernels and computes the same.
 * errors, in this order: a NULL pointer that the call needs BEVR_E_NULL; n, m or E <= 0 BEVR_E_SHAPE; then the forward's
 *   alignment rule.
 *   Aliased operands, cam == map (the same pointer) and n == m: dcam receives the SUM of both sides' gradients (the
 *   gradient of the one matrix both arguments are) and dmap is neither read nor written -- the same for every n, m, E
 *   and alignment.  A caller that wants the two sides apart passes two buffers (a copy of one side).
 * ---------------------------------------------------------------------------------------------- */
int bevr_corr_fwd(const float* cam, const float* map, float* D, float* inv_norm_cam, float* inv_norm_map,
                  int n, int m, int E, int normalize, void* stream);
int bevr_corr_bwd(const float* cam, const float* map, const float* D, const float* dD,
                  const float* inv_norm_cam, const float* inv_norm_map, float* dcam, float* dmap,
                  int n, int m, int E, int normalize, void* stream);
/* Rank of the diagonal within its column (train.py:559-563): rank[k] = #{ i : D[i][k] < D[k][k] }.
 *   D [n][n] float, rank [n] int32, any n > 0 (BEVR_E_SHAPE otherwise; a NULL pointer BEVR_E_NULL); no alignment contract.
 *   The comparison is the float one: an entry equal to the diagonal is not counted, and a NaN counts on neither side
 *   (a NaN diagonal has rank 0). */
int bevr_recall_rank(const float* D, int32_t* rank, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise k x k convolution, one filter per channel, stride 1, zero "same" padding, k odd and <= 5: the local
 * perception units and the MLP's 3x3 of the reference's EncoderLayer (model/encoder.py:363-411,
 * model/model_utils.py:6-35) and TSA's offset head (model/TSA_deform_attn.py:54-68).
 *   x, y  [B][H][W][C] (nhwc = 1) or [B][C][H][W] (nhwc = 0) float      w [C][k][k] float      bias [C] or NULL
 *   flip = 1 correlates with the flipped filter: the input gradient is bevr_dwconv_fwd(dy, w, NULL, dx, ..., flip = 1).
 * bevr_dwconv_bwd_w ACCUMULATES dw [C][k][k] and dbias [C] (dbias may be NULL); the caller zeroes them.
 * ---------------------------------------------------------------------------------------------- */
int bevr_dwconv_fwd(const float* x, const float* w, const float* bias, float* y,
                    int B, int H, int W, int C, int k, int nhwc, int flip, void* stream);
int bevr_dwconv_bwd_w(const float* x, const float* dy, float* dw, float* dbias,
                      int B, int H, int W, int C, int k, int nhwc, void* stream);
/* The MLP's  act(y + dwc(y))  of model/model_utils.py:51-59 (nn.GELU, erf form) with the depthwise 3 x 3, one kernel
 * (ABI 6; channels-last [B][H][W][C], C % 4 == 0, k = 3):
 *   mode 1  y = gelu(x + conv(x) + bias)                               the forward
 *   mode 2  y = aux * gelu'(x + conv(x) + bias)                        backward: gradient at the pre-activation (aux = d out)
 *   mode 3  y = x + conv^T(x)    (flipped filter, bias ignored)        backward: the input gradient from mode 2's result
 * The weight / bias gradients are bevr_dwconv_bwd_w(x, <mode 2's result>). */
int bevr_dwconv_res_gelu(const float* x, const float* w, const float* bias, const float* aux, float* y, int B, int H, int W,
                         int C, int k, int mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operand packing for bevr_attn_* (the reshapes of model/SCA_deform_attn.py:312-321 / TSA_deform_attn.py:226-236:
 * proj_k / proj_v outputs -> per-head operands), one pass instead of a permute / pad / cast / transpose chain.
 *   k, v  rows (n_prob, N, heads*c) float with row stride ld floats (ld >= heads*c; K | V of one GEMM: ld = 2 heads c)
 *         and problem stride pstride ROWS (pstride >= N; a key segment of a longer row array: pstride = its row count)
 *   Kr, Vr [n_prob][heads][Np][32] E   row layout: head_dim c <= 32 zero padded, keys N..Np-1 zero (Np % 64 == 0)
 *   Kt, Vt [n_prob][heads][32][Np] E   transposed, bits 2 <-> 3 of the in-32 key index swapped (either may be NULL)
 *   E = bf16 (BEVR_PREC_BF16) or fp16 (BEVR_PREC_F16), round to nearest even, or float (BEVR_PREC_F32).
 * bevr_unpack_dkv is the adjoint on the gradients of the row layout: dK, dV [n_prob][heads][Np][32] float ->
 * dk, dv rows (n_prob, N, heads*c) with row stride ld (every element of the rows written).
 * ---------------------------------------------------------------------------------------------- */
int bevr_pack_kv(const float* k, const float* v, long long ld, long long pstride, int n_prob, int N, int Np, int heads,
                 int c, int precision, void* Kr, void* Vr, void* Kt, void* Vt, void* stream);
int bevr_unpack_dkv(const float* dK, const float* dV, float* dk, float* dv, long long ld, long long pstride, int n_prob,
                    int N, int Np, int heads, int c, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the channel axis of channels-last rows, forward and backward (LayerNormProxy,
 * model/model_utils.py:37-49; the norm an EncoderLayer shares between its four uses, model/encoder.py:275).
 *   x, y, dy, dx [rows][C] float;  gamma, beta [C];  mean, rstd [rows] (written by the forward, read by the backward)
 *   C % 4 == 0, C / 4 a power of two <= 64.   backward: dx written, dgamma / dbeta [C] ACCUMULATED (caller zeroes).
 * ---------------------------------------------------------------------------------------------- */
int bevr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       long long rows, int C, float eps, void* stream);
int bevr_layernorm_bwd(const float* x, const float* gamma, const float* dy, const float* mean, const float* rstd,
                       float* dx, float* dgamma, float* dbeta, long long rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The attention output on its way to proj_out (ABI 6): the softmax merge of two key segments and the unpacking of the
 * packed per-(problem, head) rows into the layout the projection contracts, one pass each way.  Replaces the
 * concatenation of the per-view outputs along channels before proj_out (model/SCA_deform_attn.py:415-420) and the
 * (B, S S, C) flattening of TSA (model/TSA_deform_attn.py:325-333); with two segments also the merge
 *     L = log2(2^L_r + 2^L_c),  O = 2^(L_r - L) O_r + 2^(L_c - L) O_c
 * of the halves of ONE softmax that two kernel families computed (segment r: bevr_attn_fwd / _gather_fwd (+ _cell_fwd),
 * segment c: bevr_attn_tap_fwd + the caller's R Vpix product).
 *   O_r, O_c, dO_r, dO_c  [n_prob][heads][S * Sp][32] float, row j * Sp + i (the attention kernels' O layout);
 *                         n_prob = B * views, problem b * views + v;  channels c .. 31 and rows i >= S: padding
 *   L_r, L_c, dL_r, dL_c  [n_prob][heads][S * Sp]  log2-sum-exp of the segment (LSE plane 0) and its gradient
 *   out, dout             [B][S * S][views * heads * c], row i * S + j, channel (v * heads + hh) * c + cc
 *   O_c == NULL: one segment (L_r, L_c, dL_r, dO_c, dL_c unused): unpack only.
 *   backward: every element of dO_r (dO_c, dL_r, dL_c) is WRITTEN, the padding with zeros.
 *   Sp a multiple of 32, Sp >= S; c a multiple of 4, <= 32; n_prob a multiple of views.
 * ---------------------------------------------------------------------------------------------- */
int bevr_merge_views_fwd(const float* O_r, const float* L_r, const float* O_c, const float* L_c, float* out, int n_prob,
                         int views, int heads, int S, int Sp, int c, void* stream);
int bevr_merge_views_bwd(const float* dout, const float* O_r, const float* L_r, const float* O_c, const float* L_c,
                         float* dO_r, float* dL_r, float* dO_c, float* dL_c, int n_prob, int views, int heads, int S,
                         int Sp, int c, void* stream);
/* The same with the tap segment's half formed on the way instead of passed in:  O_c = Rn Vp + bv  (csrc/attn_tap.h:
 * V_n = sum_t w_t(n) Vpix_t + bv, so the tap kernels' output is the per-pixel weight sum Rn, not O).
 *   Rn, dRn  [n_prob][heads][S * Sp][12] float (bevr_attn_tap_fwd's R, normalised by the caller)
 *   Vp, dVp  [n_prob][heads][12][32] float: the 12 pixels' value rows per head (channels c .. 31 zero);  bv, dbv [heads][32]
 *   dVp, dbv are ACCUMULATED (the caller zeroes them); everything else is written.  Other arguments as above. */
int bevr_merge_tap_fwd(const float* O_r, const float* L_r, const float* Rn, const float* L_c, const float* Vp, const float* bv,
                       float* out, int n_prob, int views, int heads, int S, int Sp, int c, void* stream);
int bevr_merge_tap_bwd(const float* dout, const float* O_r, const float* L_r, const float* Rn, const float* L_c, const float* Vp,
                       const float* bv, float* dO_r, float* dL_r, float* dRn, float* dL_c, float* dVp, float* dbv, int n_prob,
                       int views, int heads, int S, int Sp, int c, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The cotangent's way into the 16-bit backward kernels (ABI 6), one pass over dO and O:
 *   dO, O   [n_ph][Mp][32] float (n_ph = n_prob * heads): the output's cotangent and the forward's output
 *   scale   one float on the device or NULL: a power of two applied to dO (and to dLSE) before the rounding (fp16 mode)
 *   dLSE, LSE0  [n_ph][Mp] float or NULL: the cotangent of the log2-sum-exp output (a caller that merged this softmax with
 *           another segment sends one) and LSE plane 0 (rows with a non-finite LSE take no dLSE)
 *   dOe     [n_ph][Mp][32] E: the rounded rows -- the dO operand of bevr_attn_bwd_q / _slab_bwd_q / _cell_bwd_q / _bwd_k
 *   dOt     [n_ph][32][Mp] E: the same transposed, position p of a 32-block holding row perm32(p) (bits 2 and 3 of p
 *           swapped): the dOt operand of bevr_attn_bwd_k / _cell_bwd_k
 *   delta   [n_ph][Mp] float: rowsum(dOe o O) - log2(e) scale dLSE: the `delta` operand of every backward entry point
 *   stats   2 floats the caller zeroed: raised (atomic max) to max ||dOe row||^2 and max |delta| -- the bound behind
 *           grad_scale.   Mp % 32 == 0; precision BEVR_PREC_BF16 or BEVR_PREC_F16.
 * Replaces the autograd bookkeeping between the output's cotangent and the kernels (model/SCA_deform_attn.py:331-413).
 * ---------------------------------------------------------------------------------------------- */
int bevr_attn_bwd_prep(const float* dO, const float* O, const float* scale, const float* dLSE, const float* LSE0, void* dOe,
                       void* dOt, float* delta, float* stats, int n_ph, int Mp, int precision, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K | V operands straight from the feature map (16-bit operand modes): bilinear sampling at `pos` -> proj_k | proj_v
 * as one 1x1 GEMM on the matrix cores -> the packed layouts below, in one pass; the sampled features and the projected
 * rows never reach HBM.  Replaces bevr_sample_fwd -> GEMM -> bevr_pack_kv, i.e. F.grid_sample + proj_k / proj_v + the
 * per-head reshapes of model/SCA_deform_attn.py:290-321, model/TSA_deform_attn.py:210-236.
 *   feat [nb][Hi][Wi][C]  float, or bf16 bits if feat_bf16 (channels-last)
 *   groups: channel groups (ABI 5; the reference's n_groups): the C / groups channels of group gi are sampled at group gi's
 *        positions -- x.reshape(B g, C / g, Hi, Wi) against pos (B g, N, 2), model/SCA_deform_attn.py:290-301 -- and the
 *        projection then mixes all C channels as before.  C % groups == 0, (C / groups) % 4 == 0.
 *   pos  (y, x) of key n of problem b, group gi at pos[((b * groups + gi) * pos_pstride + n) * 2]   (a key segment:
 *        pass pos + 2 n0)
 *   Wkv  [2C][C] E (E = bf16 / fp16 per `precision`: the caller rounds the float weights once), rows 0..C-1 = proj_k
 *   bkv  [2C] float or NULL
 *   outputs as bevr_pack_kv: Kr, Vr [nb][heads][Np][32] E, Kt (or NULL), Vt [nb][heads][32][Np] E; keys N..Np-1 zero.
 *   vnorm2_max: one float the caller zeroed, or NULL: raised (atomic max) to the largest squared row norm of V -- the
 *            bound the backward's fixed-point scale needs (grad_scale), for free instead of a pass over V.
 *   knorm2_max (ABI 6): [nb][heads] floats the caller zeroed, or NULL: raised (atomic max) to the largest squared row
 *            norm of K per (problem, head) -- the gather / tap forward's static softmax reference needs max ||K_n||
 *            (bevr_attn_gather_fwd's mref), for free instead of a pass over K.  Both norms are of the UNROUNDED rows.
 *   C = heads * c, c <= 32, C % 16 == 0, C <= 256; Np % 64 == 0.
 * The adjoint stays unfused: bevr_unpack_dkv -> GEMMs -> bevr_sample_bwd on samples recomputed with bevr_sample_fwd.
 * ---------------------------------------------------------------------------------------------- */
int bevr_kv_project(const void* feat, int feat_bf16, const float* pos, long long pos_pstride, const void* Wkv,
                    const float* bkv, int nb, int Hi, int Wi, int C, int N, int Np, int heads, int c, int precision,
                    void* Kr, void* Vr, void* Kt, void* Vt, float* vnorm2_max, float* knorm2_max, int groups,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * bevr_kv_project with SPLIT WEIGHTS (additive in ABI 6): the same pass, the weight operand as two E planes.  A rounded
 * weight is an error common to all keys, which the attention's average over the keys does not shrink; the samples'
 * rounding is per key and does, so the samples stay rounded once to E.
 *   Wkv2   [2][2C][C] E, 16-byte aligned, plane 1 exactly 2C * C elements behind plane 0:
 *            plane 0  hi  = E(w)
 *            plane 1  lo' = E((w - hi) * 2^lo_exp)
 *   lo_exp 0 .. 24 (BEVR_E_SHAPE otherwise).  0: lo' is the plain residual (bf16: its exponent range is float's).  fp16:
 *          the residual of a small weight is subnormal or zero as a plain fp16 value; ops.kv_split_weights passes 11.
 * Summation order: per k-step (16 input channels) the lo' products are issued before the hi products into the same f32
 * accumulators; with lo_exp != 0 every lo' k-step runs first, the accumulators are multiplied once by 2^-lo_exp
 * (exact) and the hi k-steps follow:   row = (sum lo' x) 2^-lo_exp + sum hi x + bias,  x = E(sample).
 * Everything else is bevr_kv_project's contract: the other arguments, the checks and their order (NULL pointers, shapes
 * with lo_exp, the f32-layout modes: BEVR_E_PRECISION, alignment), the outputs, and both norms, which are still of the
 * UNROUNDED rows.  The adjoint is unchanged: it already uses the float weights.
 * ---------------------------------------------------------------------------------------------- */
int bevr_kv_project_w2(const void* feat, int feat_bf16, const float* pos, long long pos_pstride, const void* Wkv2,
                       int lo_exp, const float* bkv, int nb, int Hi, int Wi, int C, int N, int Np, int heads, int c,
                       int precision, void* Kr, void* Vr, void* Kt, void* Vt, float* vnorm2_max, float* knorm2_max,
                       int groups, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Key positions from the offset heads' outputs, in the attention's key order, and the adjoint (one launch each).
 * Replaces model/SCA_deform_attn.py:248-277 (row split of the (b g) d (h n) w head output, tanh * range, + reference
 * point -- or clamp --, per view) and model/TSA_deform_attn.py:170-196, plus the gather into the static key order.
 *   off   [V][P][block] float   one view's head output per problem p = b * G + gi (P = B * G):
 *           sca = 1: block = [S][S][D] (the fused head's channels-last output); component c (0 = y, 1 = x) of key
 *                    n = hk * (S D) + w * D + d is element [(2 hk + c)][w][d]           (N = (S / 2) * S * D)
 *           sca = 0: block = [N][2]   (y, x) per key-grid pixel
 *   ref   [V][N][2] float (y, x)   reference points (SCA) / the regular grid (TSA), in the UNordered key index
 *   order [V][N] int32 or NULL     static key order: output key n' is key order[v][n']
 *   pos   [B][V][G][N][2] float    use_tanh = 1: tanh(off) * (sy, sx) + ref;   0: clamp(off + ref, -1, 1)
 * backward: doff (off's shape) is WRITTEN (the order is a permutation: every element belongs to one key).
 * ---------------------------------------------------------------------------------------------- */
int bevr_key_positions_fwd(const float* off, const float* ref, const int* order, float* pos, int V, int P, int G, int N,
                           int sca, int S, int D, int use_tanh, float sy, float sx, void* stream);
int bevr_key_positions_bwd(const float* off, const float* ref, const int* order, const float* dpos, float* doff, int V,
                           int P, int G, int N, int sca, int S, int D, int use_tanh, float sy, float sx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Offset heads of the deformable attention blocks, fused per BEV pixel (model/SCA_deform_attn.py:56-77 conv_offset_m{v};
 * the LayerNorm -> GELU -> 1x1 tail of model/TSA_deform_attn.py:54-68):
 *   z[c*Mx + m] = x[c] * w0[c*Mx + m] + b0[c*Mx + m]   (depthwise 1x1, channel multiplier Mx; w0 == NULL: z = x, Mx = 1)
 *   out[d] = sum_k W3[d][k] * GELU_erf( LayerNorm_{Cg*Mx}(z)[k] * gamma[k] + beta[k] )
 *   x   [P pixels][xstride] float, the head's Cg <= 64 input channels first (a channel group of a channels-last tensor:
 *       pass the pointer to the group's first channel and xstride = the tensor's channel count)
 *   w0, b0, gamma, beta [Cg*Mx], W3 [Dout][Cg*Mx], out [P][Dout] float.  (Mx, Dout) = (1, 2) or Mx == Dout <= 8.
 * backward: dx [P][xstride] (may be NULL) and every parameter gradient are ACCUMULATED (caller zeroes them);
 *   dw0 / db0 may be NULL (TSA form).
 * ---------------------------------------------------------------------------------------------- */
int bevr_offset_head_fwd(const float* x, const float* w0, const float* b0, const float* gamma, const float* beta,
                         const float* W3, float* out, long long P, int Cg, int xstride, int Mx, int Dout, float eps,
                         void* stream);
int bevr_offset_head_bwd(const float* x, const float* w0, const float* b0, const float* gamma, const float* beta,
                         const float* W3, const float* dout, float* dx, float* dw0, float* db0, float* dgamma,
                         float* dbeta, float* dW3, long long P, int Cg, int xstride, int Mx, int Dout, float eps,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ego-motion warp of the history BEV (model/encoder.py:413-466): one torchvision-style affine resampling,
 * bilinear, zero padding, fill = 0 -- out = bilinear(img) * bilinear(ones) -- for a whole batch.
 *   img, out [B][C][H][W] float      theta [B][6] float (device): torchvision's INVERSE affine matrix in pixel units
 *   about the image centre, rows (m0 m1 m2; m3 m4 m5): the source pixel of output pixel (x, y) is
 *   (m0 X + m1 Y + m2 + (W-1)/2, m3 X + m4 Y + m5 + (H-1)/2), X = x - W/2 + 1/2, Y = y - H/2 + 1/2.
 * backward: dimg ACCUMULATED from dout with the same theta (caller zeroes dimg).
 * ---------------------------------------------------------------------------------------------- */
int bevr_affine_warp_fwd(const float* img, const float* theta, float* out, int B, int C, int H, int W, void* stream);
int bevr_affine_warp_bwd(const float* dout, const float* theta, float* dimg, int B, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVRENDER_HIP_H */
