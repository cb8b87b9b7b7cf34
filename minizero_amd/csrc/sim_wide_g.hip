// the wide simulation kernel on the bf16x3 tower (sim_wide_bf16.inc), part 6: 9x9 Go, 128 hidden channels
#define MZ_SIM_WIDE_PART 6
#define MZ_SIM_WIDE_BF16_CASE(X) X(9, 9, 32, 128, 2)
#include "sim_wide_bf16.inc"
