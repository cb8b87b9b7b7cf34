// The one-tile bf16x3 tower (net_bf16_wide_body.h) as a stand-alone launch: AlphaZero networks with 128 / 256 hidden channels on 9x9 boards and with 64 on
// 11x11 / 15x15 boards under `mz_nn_precision=bf16x3` — mz_net_forward_az and the lock-step worker.  gfx950, -ffp-contract=off.
#include "net.h"
#include "net_bf16_wide_body.h"

namespace mz {

// bit-packed planes in, f32 NCHW out; gx, gt: [B][C][P] blocks, the workgroups' x in global memory
template <int H, int W, int C>
__global__ __launch_bounds__(512) void tower_fused_bf16_wide(const unsigned* __restrict__ in_bits, const uint4* __restrict__ wfrag, const float* __restrict__ params,
                                                             TowerArgsBf16 ta, float* __restrict__ gx, float* __restrict__ gt, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char tile[];
    constexpr size_t CP = size_t(C) * H * W;
    towerBodyBf16Wide<H, W, C>(in_bits, wfrag, params, ta, gx + blockIdx.x * CP, gt + blockIdx.x * CP, out, blockIdx.x, threadIdx.x, tile);
}

template <int H, int W, int C>
static int launchTowerBf16WideT(const TowerArgsBf16& ta, const uint4* wfrag, const float* params, const unsigned* bits, float* gx, float* gt, float* out, int B, hipStream_t s)
{
    constexpr size_t lds = Bf16WideGeo<H, W, C>::kTileBytes;
    MZ_LDS_ATTR((tower_fused_bf16_wide<H, W, C>), lds);
    hipLaunchKernelGGL((tower_fused_bf16_wide<H, W, C>), dim3(B), dim3(512), lds, s, bits, wfrag, params, ta, gx, gt, out);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

int Net::launchTowerBf16Wide(const TowerArgsBf16& ta, const unsigned* bits, float* gx, float* gt, float* out, int B)
{
    const int H = desc_.hidden_channel_height, W = desc_.hidden_channel_width, C = desc_.num_hidden_channels;
    if (H == 9 && W == 9 && C == 128) { return launchTowerBf16WideT<9, 9, 128>(ta, wfrag_.p, params_.p, bits, gx, gt, out, B, stream_); }
    if (H == 9 && W == 9 && C == 256) { return launchTowerBf16WideT<9, 9, 256>(ta, wfrag_.p, params_.p, bits, gx, gt, out, B, stream_); }
    if (H == 11 && W == 11 && C == 64) { return launchTowerBf16WideT<11, 11, 64>(ta, wfrag_.p, params_.p, bits, gx, gt, out, B, stream_); }
    if (H == 15 && W == 15 && C == 64) { return launchTowerBf16WideT<15, 15, 64>(ta, wfrag_.p, params_.p, bits, gx, gt, out, B, stream_); }
    setError("bf16x3 tower: no one-tile instance for %dx%d x %d channels", H, W, C);
    return MZ_ERR_STATE;
}

} // namespace mz
