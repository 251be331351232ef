// Tap fwd in the split-bf16 mode with attention dropout: the same source as attn_tap_fwd.hip, compiled for the split
// instantiations with the keep-mask blocks in (attn_tap.h) -- a separate translation unit so that the split kernels
// without dropout and the 16-bit dropout kernels are unchanged.  Entry point: bevr_attn_tap_fwd_x3_dropout.
#define BEVR_TAP_X3 1
#define BEVR_DROP 1
#include "attn_tap_fwd.hip"
