// qs_kernels_strat.hip — MostAllocated / RequestedToCapacityRatio kernels, compact row layout.
#define QS_STRAT_WIDE 0
#include "qs_kernels_strat.inc"
