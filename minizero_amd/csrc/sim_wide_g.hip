// instances of the wide simulation kernel, part 6 (sim_wide.inc): the bf16x3 tower, 9x9 Go, 128 hidden channels
#define MZ_SIM_WIDE_PART 6
#define MZ_SIM_WIDE_CASES(X) X(bf16, 9, 9, 32, 128, 2)
#include "sim_wide.inc"
