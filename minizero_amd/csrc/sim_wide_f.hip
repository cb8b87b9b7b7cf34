// instances of the wide simulation kernel, part 5 (sim_wide.inc): Hex
#define MZ_SIM_WIDE_PART 5
#include "sim_wide.inc"
