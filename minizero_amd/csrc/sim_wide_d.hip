// instances of the wide simulation kernel, part 3 (sim_wide.inc): Othello and TicTacToe at the reference's default width, the same phase functions as sim_kernel's
#define MZ_SIM_WIDE_PART 3
#define MZ_SIM_WIDE_CASES(X) X(f32, 8, 8, 16, 128, kRulesOthello) X(f32, 8, 8, 16, 256, kRulesOthello) X(f32, 3, 3, 16, 128, kRulesTicTacToe) X(f32, 3, 3, 16, 256, kRulesTicTacToe)
#include "sim_wide.inc"
