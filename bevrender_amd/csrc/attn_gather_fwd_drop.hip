// Gather forward with attention dropout: the same source as attn_gather_fwd.hip, compiled as the row-range kernel with
// the keep-mask blocks in (bevr_common.h: bevr_drop_keep) -- a separate translation unit so that the kernels without
// dropout are unchanged.
#define BEVR_GATHER_ROWS 1
#define BEVR_DROP 1
#include "attn_gather_fwd.hip"
