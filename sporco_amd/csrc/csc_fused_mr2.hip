// csc_fused_mr2.hip -- the column launchers of csc_fused_kernels.inc at the second half of the mixed-radix
// heights (H = 16 N1, N1 in regfft.h SA_MR_LENGTHS_HI; csc_fused_mr.hip: the first half).
#include "csc_fused_kernels.inc"

namespace sporco_amd {
#define SA_FUSED_INSTANTIATE(n) SA_FUSED_LAUNCHERS(template, n)
SA_MR_LENGTHS_HI(SA_FUSED_INSTANTIATE)
}  // namespace sporco_amd
