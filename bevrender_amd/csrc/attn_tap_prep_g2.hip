// The tap kernels for two channel groups (attn_tap.h): attn_tap_prep.hip compiled with the second group's slots -- a
// separate translation unit so that the one-group kernels' code objects are unchanged.
#define BEVR_TAP_G2 1
#define attn_tap_prep_kernel attn_tap_g2_prep_kernel   // a name of its own in traces
#include "attn_tap_prep.hip"
