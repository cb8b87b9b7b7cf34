// instances of the wide simulation kernel, part 12 (sim_wide.inc): the bf16x3 tower, Havannah edge size 8 (15x15 array), 64 hidden channels; 20 planes pad to 32
#define MZ_SIM_WIDE_PART 12
#define MZ_SIM_WIDE_CASES(X) X(bf16, 15, 15, 32, 64, kRulesHavannah)
#include "sim_wide.inc"
