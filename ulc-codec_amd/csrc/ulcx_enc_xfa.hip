// ulcx_enc_xfa.hip - the analysis call's kernels (ulcx_analyse_launch): the MDCT-only transform k_xfa / k_xfa_big and the sums
// without rate logic k_cplxa.  They are the AN = true instantiations of the transform bodies in ulcx_enc_xf.hip, compiled here
// as a translation unit of their own so that the encode call's kernels come out of theirs as they did before.
#define ULCX_XF_ANALYSIS_UNIT
#include "ulcx_enc_xf.hip"
