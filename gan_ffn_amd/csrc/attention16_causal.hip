// attention16_causal.hip — the CAUSAL instantiations of attention16.hip's kernels (GANFFN_ATTN_CAUSAL: query i attends to keys
// j <= i) and their launchers attn16_fwd<true> / attn16_bwd<true>, as a translation unit of their own, so that the kernels
// without the flag are compiled in a module that holds nothing else and keep their instructions (see attention16.hip, host side).
#define GANFFN_A16_CAUSAL_TU
#include "attention16.hip"
