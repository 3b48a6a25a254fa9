// qs_kernels_strat_wide.hip — MostAllocated / RequestedToCapacityRatio kernels, wide row layout.
#define QS_STRAT_WIDE 1
#include "qs_kernels_strat.inc"
