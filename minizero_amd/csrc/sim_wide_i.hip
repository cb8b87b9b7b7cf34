// instances of the wide simulation kernel, part 8 (sim_wide.inc): NoGo on Go's 9x9 networks
#define MZ_SIM_WIDE_PART 8
#define MZ_SPEC_WAYS 4 // four remembered paths instead of sixteen (pool_body.h), as the Go instance of the widest shape (sim_wide_c.hip)
#include "sim_wide.inc"
