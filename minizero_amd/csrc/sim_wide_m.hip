// the wide simulation kernel on the bf16x3 tower (sim_wide_bf16.inc), part 12: Havannah edge size 8 (15x15 array), 64 hidden channels; 20 planes pad to 32
#define MZ_SIM_WIDE_PART 12
#define MZ_SIM_WIDE_BF16_CASE(X) X(15, 15, 32, 64, kRulesHavannah)
#include "sim_wide_bf16.inc"
