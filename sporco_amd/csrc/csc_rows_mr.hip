// csc_rows_mr.hip -- the row launchers of csc_rows_body.inc at the first half of the mixed-radix
// widths (W = 16 N1, N1 in regfft.h SA_MR_LENGTHS_LO; csc_rows_mr2.hip: the second half).
#include "csc_rows_body.inc"

namespace sporco_amd {
#define SA_ROWS_INSTANTIATE(n) SA_ROWS_LAUNCHERS(template, n)
SA_MR_LENGTHS_LO(SA_ROWS_INSTANTIATE)
}  // namespace sporco_amd
