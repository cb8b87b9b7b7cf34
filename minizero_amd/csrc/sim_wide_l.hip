// the wide simulation kernel on the bf16x3 tower (sim_wide_bf16.inc), part 11: Hex on its default 11x11 board, 64 hidden channels
#define MZ_SIM_WIDE_PART 11
#define MZ_SIM_WIDE_BF16_CASE(X) X(11, 11, 16, 64, kRulesHex)
#include "sim_wide_bf16.inc"
