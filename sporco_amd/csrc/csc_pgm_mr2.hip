// csc_pgm_mr2.hip -- the column launchers of csc_pgm_body.inc at the second half of the mixed-radix
// heights (H = 16 N1, N1 in regfft.h SA_MR_LENGTHS_HI; csc_pgm_mr.hip: the first half).
#include "csc_pgm_body.inc"

namespace sporco_amd {
#define SA_PGM_INSTANTIATE(n) SA_PGM_LAUNCHERS(template, n)
SA_MR_LENGTHS_HI(SA_PGM_INSTANTIATE)
}  // namespace sporco_amd
