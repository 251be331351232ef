// Split-bf16 slab query-side backward over a BAND of row blocks of every BEV column (BEV sides up to 448): the same source
// as attn_slab_bwd_q_x3.hip, compiled with the row pitch as a template parameter and the row-block origin in -- a separate
// translation unit so that the S <= 211 kernels are unchanged.
#define BEVR_SLAB_ROWS 1
#include "attn_slab_bwd_q_x3.hip"
