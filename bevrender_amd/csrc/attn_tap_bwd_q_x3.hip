// Tap bwd_q in the split-bf16 mode (BEVR_PREC_BF16X3, attn_tap.h): the same source as attn_tap_bwd_q.hip, compiled for
// the split instantiations alone -- a separate translation unit so that the 16-bit kernels' code objects are unchanged.
#define BEVR_TAP_X3 1
#include "attn_tap_bwd_q.hip"
