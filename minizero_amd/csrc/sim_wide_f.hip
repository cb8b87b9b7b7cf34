// instances of the wide simulation kernel, part 5 (sim_wide.inc): Hex on its default 11x11 board, 64 channels (measured), 32 (tests), 128
#define MZ_SIM_WIDE_PART 5
#define MZ_SIM_WIDE_CASES(X) X(f32, 11, 11, 16, 64, kRulesHex) X(f32, 11, 11, 16, 32, kRulesHex) X(f32, 11, 11, 16, 128, kRulesHex)
#include "sim_wide.inc"
