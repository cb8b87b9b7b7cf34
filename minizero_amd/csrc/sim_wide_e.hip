// instances of the wide simulation kernel, part 4 (sim_wide.inc): Gomoku on its default 15x15 board, 64 channels (measured), 32 (tests)
#define MZ_SIM_WIDE_PART 4
#define MZ_SIM_WIDE_CASES(X) X(f32, 15, 15, 16, 64, kRulesGomoku) X(f32, 15, 15, 16, 32, kRulesGomoku)
#include "sim_wide.inc"
