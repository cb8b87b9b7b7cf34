// instances of the wide simulation kernel, part 9 (sim_wide.inc): Havannah (a game past the rows: game_kind.h), edge size 8 on its 15x15 array with 64 channels
// (measured) and 32, edge size 4 (7x7) with 32 (tests); 20 planes pad to 32
#define MZ_SIM_WIDE_PART 9
#define MZ_SIM_WIDE_CASES(X) X(f32, 15, 15, 32, 64, kRulesHavannah) X(f32, 15, 15, 32, 32, kRulesHavannah) X(f32, 7, 7, 32, 32, kRulesHavannah)
#include "sim_wide.inc"
