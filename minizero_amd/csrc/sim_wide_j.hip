// instances of the wide simulation kernel, part 9 (sim_wide.inc): Havannah
#define MZ_SIM_WIDE_PART 9
#include "sim_wide.inc"
