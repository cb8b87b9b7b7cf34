// instances of the wide simulation kernel, part 10 (sim_wide.inc): the bf16x3 tower, Gomoku on its default 15x15 board, 64 hidden channels
#define MZ_SIM_WIDE_PART 10
#define MZ_SIM_WIDE_CASES(X) X(bf16, 15, 15, 16, 64, kRulesGomoku)
#include "sim_wide.inc"
