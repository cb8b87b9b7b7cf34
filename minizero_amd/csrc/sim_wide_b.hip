// instances of the wide simulation kernel, part 1 (sim_wide.inc)
#define MZ_SIM_WIDE_PART 1
#define MZ_SIM_WIDE_CASES(X) X(f32, 7, 7, 32, 32, 1) X(f32, 7, 7, 32, 64, 1) X(f32, 7, 7, 32, 256, 1)
#include "sim_wide.inc"
