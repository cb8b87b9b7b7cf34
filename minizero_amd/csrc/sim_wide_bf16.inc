// What is bf16-specific of the wide simulation kernel (sim_wide.inc, which includes this file behind its frame): the tower function on the opt-in bf16x3 tower of
// net_bf16_wide_body.h — 9x9 Go AlphaZero with 128 / 256 hidden channels, Gomoku 15x15, Hex 11x11 and Havannah 15x15 with 64 under `mz_nn_precision=bf16x3` — its
// policy and the kernel.  The tower body is the stand-alone launch's (net_bf16_wide.hip) — same code, same order, same bits: the lock-step mode on the bf16x3 tower
// writes the same records.  The LDS plan is the frame's (lf; Net::simWidePlan) around a tile of another size.
#include "net_bf16_wide_body.h"

namespace mz {

template <int H, int W, int C>
__device__ __noinline__ const float* simTowerWideBf16(CSimArgs* __restrict__ a, int g, int tid, float* tile, float* xchg)
{
    g = __builtin_amdgcn_readfirstlane(g); // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    constexpr size_t CP = size_t(C) * H * W;
    return towerBodyBf16Wide<H, W, C>(reinterpret_cast<const unsigned*>(gv.feat), a->wfrag, a->params, *(const TowerArgsBf16*)&a->tb, a->act + size_t(g) * CP,
                                      a->act2 + size_t(g) * CP, nullptr, g, tid, reinterpret_cast<char*>(tile));
}

template <int H, int W, int CIN0Q, int C>
struct WideTowerBf16 {
    using G = Bf16WideGeo<H, W, C>;
    static constexpr int kPrec = 1; // Net::precision()
    static constexpr int kTileFloats = G::kTileBytes / 4;
    static_assert(G::kTileBytes % 4 == 0, "the frame carves the LDS behind the tile in floats");
    static constexpr int CS = G::CS, PW = G::PW;
    static __device__ __forceinline__ const float* run(CSimArgs* __restrict__ a, int g, int tid, float* tile, float* xchg) { return simTowerWideBf16<H, W, C>(a, g, tid, tile, xchg); }
};

template <int H, int W, int CIN0Q, int C, int CPL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void sim_kernel_wide_bf16(const SimArgs* __restrict__ a_, const uint8_t* __restrict__ rot_tab, int sim0,
                                                                                                       int nsims, int host_start, int lf)
{
    simWideFrame<H, W, CPL, WideTowerBf16<H, W, CIN0Q, C>>(a_, rot_tab, sim0, nsims, host_start, lf);
}

} // namespace mz
