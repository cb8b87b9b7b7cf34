// instances of the wide simulation kernel, part 4 (sim_wide.inc): Gomoku
#define MZ_SIM_WIDE_PART 4
#include "sim_wide.inc"
