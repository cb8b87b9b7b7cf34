// the wide simulation kernel on the bf16x3 tower (sim_wide_bf16.inc), part 10: Gomoku on its default 15x15 board, 64 hidden channels
#define MZ_SIM_WIDE_PART 10
#define MZ_SIM_WIDE_BF16_CASE(X) X(15, 15, 16, 64, kRulesGomoku)
#include "sim_wide_bf16.inc"
