// Tap bwd_q with attention dropout: the same source as attn_tap_bwd_q.hip, compiled with the keep-mask blocks in
// (attn_tap.h, bevr_common.h: bevr_drop_keep) -- a separate translation unit so that the kernel without dropout is unchanged.
#define BEVR_DROP 1
#include "attn_tap_bwd_q.hip"
