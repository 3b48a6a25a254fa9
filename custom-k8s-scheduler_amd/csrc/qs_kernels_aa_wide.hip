// qs_kernels_aa_wide.hip — pod anti-affinity kernels (kFeatAA, spec S12), wide row layout.
#define QS_AA_WIDE 1
#include "qs_kernels_aa.inc"
