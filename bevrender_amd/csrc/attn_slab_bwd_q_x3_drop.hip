// Split-bf16 slab query-side backward with attention dropout: attn_slab_bwd_q_x3.hip (and through it attn_slab.h)
// compiled with the keep-mask blocks in (bevr_common.h: bevr_drop_keep) -- a separate translation unit so that the kernel
// and the preparation without dropout are unchanged.
#define BEVR_DROP 1
#include "attn_slab_bwd_q_x3.hip"
