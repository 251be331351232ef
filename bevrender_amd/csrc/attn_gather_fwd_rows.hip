// Gather forward over a ROW RANGE of every BEV column (BEV sides above 224): the same source as attn_gather_fwd.hip,
// compiled with the row origin in -- a separate translation unit so that the whole-column kernels are unchanged.
#define BEVR_GATHER_ROWS 1
#include "attn_gather_fwd.hip"
