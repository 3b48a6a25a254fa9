// qs_kernels_aa.hip — pod anti-affinity kernels (kFeatAA, spec S12), compact row layout, and k_aa_apply.
#define QS_AA_WIDE 0
#include "qs_kernels_aa.inc"
