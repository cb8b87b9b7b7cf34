// the wide simulation kernel on the bf16x3 tower (sim_wide_bf16.inc), part 7: 9x9 Go, 256 hidden channels (the reference's default width)
#define MZ_SIM_WIDE_PART 7
#define MZ_SPEC_WAYS 4 // four remembered paths instead of sixteen (pool_body.h), as the f32 instance of this shape (sim_wide_c.hip): the tile is 128 KB
#define MZ_SIM_WIDE_BF16_CASE(X) X(9, 9, 32, 256, 2)
#include "sim_wide_bf16.inc"
