// instances of the wide simulation kernel, part 11 (sim_wide.inc): the bf16x3 tower, Hex on its default 11x11 board, 64 hidden channels
#define MZ_SIM_WIDE_PART 11
#define MZ_SIM_WIDE_CASES(X) X(bf16, 11, 11, 16, 64, kRulesHex)
#include "sim_wide.inc"
