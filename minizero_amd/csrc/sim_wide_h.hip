// instances of the wide simulation kernel, part 7 (sim_wide.inc): the bf16x3 tower, 9x9 Go, 256 hidden channels (the reference's default width)
#define MZ_SIM_WIDE_PART 7
#define MZ_SPEC_WAYS 4 // four remembered paths instead of sixteen (pool_body.h), as the f32 instance of this shape (sim_wide_c.hip): the tile is 128 KB
#define MZ_SIM_WIDE_CASES(X) X(bf16, 9, 9, 32, 256, 2)
#include "sim_wide.inc"
