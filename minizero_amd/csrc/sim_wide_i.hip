// instances of the wide simulation kernel, part 8 (sim_wide.inc): NoGo (a rules variant of Go: game_kind.h) on Go's 9x9 networks, 256 channels (the reference's
// default network), 128, 32 (tests)
#define MZ_SIM_WIDE_PART 8
#define MZ_SPEC_WAYS 4 // four remembered paths instead of sixteen (pool_body.h), as the Go instance of the widest shape (sim_wide_c.hip)
#define MZ_SIM_WIDE_CASES(X) X(f32, 9, 9, 32, 256, kRulesNoGo) X(f32, 9, 9, 32, 128, kRulesNoGo) X(f32, 9, 9, 32, 32, kRulesNoGo)
#include "sim_wide.inc"
