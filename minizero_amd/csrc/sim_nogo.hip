// Instances of the per-game simulation kernel (sim_az_body.h sim_kernel) for the rules variants of Go's row (game_kind.h: NoGo) on the two-tile tower.  A
// translation unit of its own: the simulation kernels of sim.hip compile as they do without it.  The network is Go's 9x9 network, so the tower and the heads
// are the ones of sim_kernel<9, 9, 20, C, 2>; the leaf is nogoLeafBody (go_body.h), run whole by wave 0 in front of the tower — its legal mask decides the
// terminal flag that lets a simulation skip the network.  No tail help and no value-first order (both are tied to Go's two-part leaf).
#include "sim_az_body.h"

namespace mz {

MZ_SPEC_WAYS_IS(16); // (Net::simLaunch, sim.hip, computes this unit's LDS sizes from its own kSpecWords: the same value)

#define MZ_SIM_VARIANT_CASES(X) \
    X(9, 9, 20, 64, kRulesNoGo) /* 9x9 NoGo, 64 channels */ \
    X(9, 9, 20, 8, kRulesNoGo)  /* small 9x9 test nets */

template <int H, int W, int CIN0_PAD, int CPAD, int CPL>
static int launchSimVariantT(const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, size_t lds, hipStream_t s)
{
    MZ_LDS_ATTR((sim_kernel<H, W, CIN0_PAD, CPAD, CPL>), lds);
    hipLaunchKernelGGL((sim_kernel<H, W, CIN0_PAD, CPAD, CPL>), dim3(games), dim3(512), lds, s, d_args, d_rot, sim0, nsims, host_start);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

bool simVariantKernel(int H, int W, int c0, int C, int board_n, int cpl, const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, size_t lds,
                      hipStream_t s, int* rc)
{
#define MZ_SIM_VARIANT_ONE(h, w, cin0, cpad, cp)                                                                                        \
    if (H == h && W == w && c0 == cin0 && C == cpad && board_n == h && cpl == cp) {                                                     \
        if (d_args) { *rc = launchSimVariantT<h, w, cin0, cpad, cp>(d_args, games, d_rot, sim0, nsims, host_start, lds, s); }           \
        return true;                                                                                                                    \
    }
    MZ_SIM_VARIANT_CASES(MZ_SIM_VARIANT_ONE)
#undef MZ_SIM_VARIANT_ONE
    return false;
}

} // namespace mz
