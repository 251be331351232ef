// Gather forward in BEVR_PREC_BF16X3 (split-bf16 products at f32 tolerance) over a row range of every BEV column: the
// same source as attn_gather_fwd.hip, compiled with the split operand images in -- a separate translation unit so that
// the 16-bit kernels are unchanged.
#define BEVR_GATHER_ROWS 1
#define BEVR_GATHER_X3 1
#include "attn_gather_fwd.hip"
