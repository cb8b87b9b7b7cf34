// instances of the wide simulation kernel, part 2 (sim_wide.inc): the shapes whose tile leaves too little LDS for sixteen remembered paths
#define MZ_SIM_WIDE_PART 2
#define MZ_SPEC_WAYS 4 // four remembered paths instead of sixteen (pool_body.h): 7 KB instead of 26 KB of LDS beside a 119 KB tile
#define MZ_SIM_WIDE_CASES(X) X(f32, 19, 19, 32, 64, 6) X(f32, 19, 19, 32, 32, 6) X(f32, 13, 13, 32, 128, 3) X(f32, 9, 9, 32, 256, 2)
#include "sim_wide.inc"
