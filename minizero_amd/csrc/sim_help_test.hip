// Test access to the towers of the tail help of the simulation kernel (sim_help.h; include/mzgpu.h mz_tail_towers_device).  A translation unit of its own: the
// simulation kernels of sim.hip compile as they do without it.
#include <hip/hip_runtime.h>
#include "common.h"
#include "net.h"
#include "net_dev.h"
#include "net_body.h"
#include "sim_help.h"

namespace mz {

// T towers of given planes on one, two or four workgroups each
struct TailTowersArgs {
    const unsigned* bits; // [towers][cin0 * W32] bit-packed planes
    const float* params;
    unsigned* help;       // [towers][help_words], cleared
    float* out;           // [towers][C][P]
    unsigned* xcc;        // [workgroups] XCC_ID + 1
    const unsigned* expect; // nullptr: only report the XCC_IDs (the placement probe); else what the probe reported
    int* err;             // [0] the error flag of the exchanges, [1] workgroups that run on another XCD than in the probe
    int towers, help_words, fw;
};

// members of tower t: the workgroups t, t + towers, ..  (dealt to the XCDs round-robin: with a multiple of 8 towers they share an XCD).  No member waits for
// another before the placement is known: the probe launch (same kernel, same resources) only reports the XCC_IDs, the host compares the members', and a workgroup
// of the second launch that finds itself on another XCD than in the probe leaves before the first exchange.
template <int NM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void tail_towers_kernel(TailTowersArgs a, TowerArgs ta)
{
    constexpr int H = 9, W = 9, C0 = 20, C = 64, P = H * W;
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    __shared__ int s_abort;
    __shared__ unsigned s_bits[3 * kHpMaxUnits];
    const int tid = threadIdx.x;
    const int tower = blockIdx.x % a.towers, member = blockIdx.x / a.towers;
    const unsigned myxcc = hpXccId();
    if (tid == 0) { s_abort = 0; a.xcc[blockIdx.x] = myxcc; }
    if (!a.expect) { return; }
    if (a.expect[blockIdx.x] != myxcc) {
        if (tid == 0) { atomicAdd(a.err + 1, 1); }
        return;
    }
    if (tid < a.fw) { s_bits[tid] = a.bits[size_t(tower) * a.fw + tid]; }
    __syncthreads();
    HelpCtx c{a.help + size_t(tower) * a.help_words, member, 0u, &s_abort, a.err, tiles + kTowerTiles * 64 * planeStride(H, W)}; // (the slot: behind the tiles)
    const float* xt;
    if constexpr (NM == 4) { xt = towerBodyQuad<H, W, C0, C>(s_bits, a.params, ta, tid, tiles, c); }
    else if constexpr (NM == 2) { xt = towerBodyPair<H, W, C0, C>(s_bits, a.params, ta, tid, tiles, c); }
    else { xt = towerBody<H, W, C0, C>(reinterpret_cast<const float*>(s_bits), a.params, ta, nullptr, 0, tid, tiles); }
    if (!xt || member != 0) { return; }
    __syncthreads();
    for (int i = tid; i < C * P; i += 512) {
        const int ch = i / P, p = i % P;
        a.out[size_t(tower) * C * P + i] = xt[ch * planeStride(H, W) + (p / W + 1) * (W + 2) + p % W + 1];
    }
}

template <int NM>
static int launchTailTowers(const TailTowersArgs& a, const TowerArgs& ta, int wgs, hipStream_t s)
{
    constexpr size_t lds = (size_t(kTowerTiles) * 64 * planeStride(9, 9) + kHpSlotFloats) * sizeof(float);
    MZ_LDS_ATTR((tail_towers_kernel<NM>), lds);
    hipLaunchKernelGGL((tail_towers_kernel<NM>), dim3(wgs), dim3(512), lds, s, a, ta);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

int Net::tailTowers(const unsigned* bits, int towers, int members, float* out, unsigned* xcc, int* err_flag, int* status)
{
    const int H = desc_.hidden_channel_height, W = desc_.hidden_channel_width, C = desc_.num_hidden_channels;
    TowerArgs ta;
    int c0 = 0;
    if (H != 9 || W != 9 || C != 64 || !makeTowerArgs(repr_, true, true, &ta, &c0) || c0 != 20 || ta.OT != 4) { setError("tailTowers: only the 9x9 x 64 tower with a stem of up to 20 planes"); return MZ_ERR_ARG; }
    const int fw = ta.cin0 * ((H * W + 31) / 32), wgs = towers * members;
    if ((members != 1 && members != 2 && members != 4) || towers < 1 || fw > 3 * kHpMaxUnits) { setError("tailTowers: bad arguments"); return MZ_ERR_ARG; }
    if (wgs > cu_count_) { setError("tailTowers: %d workgroups must be resident at once, the device has %d CUs", wgs, cu_count_); return MZ_ERR_ARG; }
    const size_t words = helpWords(C, H * W), P = size_t(H) * W;
    DevBuf<unsigned> d_bits, d_help, d_xcc, d_expect;
    DevBuf<float> d_out;
    DevBuf<int> d_err;
    if (!d_bits.alloc(size_t(towers) * fw) || !d_help.alloc(size_t(towers) * words) || !d_xcc.alloc(wgs) || !d_expect.alloc(wgs) || !d_out.alloc(size_t(towers) * C * P) || !d_err.alloc(2)) {
        setError("tailTowers: hipMalloc failed");
        return MZ_ERR_DEVICE;
    }
    MZ_HIP(hipMemcpyAsync(d_bits.p, bits, d_bits.n * sizeof(unsigned), hipMemcpyHostToDevice, stream_));
    MZ_HIP(hipMemsetAsync(d_help.p, 0, d_help.n * sizeof(unsigned), stream_));
    MZ_HIP(hipMemsetAsync(d_out.p, 0, d_out.n * sizeof(float), stream_));
    MZ_HIP(hipMemsetAsync(d_err.p, 0, 2 * sizeof(int), stream_));
    TailTowersArgs a{d_bits.p, params_.p, d_help.p, d_out.p, d_xcc.p, nullptr, d_err.p, towers, int(words), fw};
    auto launch = [&]() { return members == 4 ? launchTailTowers<4>(a, ta, wgs, stream_) : members == 2 ? launchTailTowers<2>(a, ta, wgs, stream_) : launchTailTowers<1>(a, ta, wgs, stream_); };
    // the placement probe: where do the workgroups of this launch shape run?
    int rc = launch();
    if (rc) { return rc; }
    MZ_HIP(hipMemcpyAsync(xcc, d_xcc.p, size_t(wgs) * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipStreamSynchronize(stream_));
    *status = 0;
    *err_flag = 0;
    for (int t = 0; t < towers; ++t) {
        for (int m = 1; m < members; ++m) { if (xcc[m * towers + t] != xcc[t]) { *status = 1; } }
    }
    if (*status) { return MZ_OK; } // members on different XCDs: no exchange is run
    MZ_HIP(hipMemcpyAsync(d_expect.p, xcc, size_t(wgs) * sizeof(unsigned), hipMemcpyHostToDevice, stream_));
    a.expect = d_expect.p;
    if ((rc = launch())) { return rc; }
    int h_err[2] = {0, 0};
    MZ_HIP(hipMemcpyAsync(xcc, d_xcc.p, size_t(wgs) * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipMemcpyAsync(out, d_out.p, d_out.n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipMemcpyAsync(h_err, d_err.p, sizeof(h_err), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipStreamSynchronize(stream_));
    *err_flag = h_err[0];
    if (h_err[1]) { *status = 1; } // (its partners, if any, ran into the bounded waits of the exchange: the error flag says so)
    return MZ_OK;
}

} // namespace mz

// defined here, beside the kernel, so that the host-only builds of the worker need nothing of it
struct mz_net { mz::Net net; };
extern "C" int mz_tail_towers_device(mz_net* net, const uint32_t* bits, int towers, int members, float* out, uint32_t* xcc_out, int* err_flag_out, int* status_out)
{
    if (!net || !bits || !out || !xcc_out || !err_flag_out || !status_out) { mz::setError("mz_tail_towers_device: bad arguments"); return MZ_ERR_ARG; }
    return net->net.tailTowers(bits, towers, members, out, xcc_out, err_flag_out, status_out);
}
extern "C" int mz_tail_tower_tile(int tile, int* pixels_out)
{
    constexpr mz::TileMap<9, 9> tm{};
    if (tile < 0 || tile >= mz::TileMap<9, 9>::PT || !pixels_out) { mz::setError("mz_tail_tower_tile: bad arguments"); return MZ_ERR_ARG; }
    for (int n = 0; n < 16; ++n) { pixels_out[n] = tm.q[tile * 16 + n]; }
    return MZ_OK;
}
