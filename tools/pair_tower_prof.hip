// The 9x9 x 64 tower of one sample on ONE workgroup (net_body.h towerBody) against the same tower on a PAIR and on a QUAD of workgroups of one XCD (sim_help.h
// towerBodyPair / towerBodyQuad): time per tower with every workgroup of the launch busy, and the activations compared bit for bit with the solo tower's.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I minizero_amd/csrc -I include tools/pair_tower_prof.hip -o tools/_bin/pair_tower_prof
// usage: pair_tower_prof [pairs (a multiple of 16, default 128: every CU busy; 16: 8 quads, four workgroups per XCD)] [towers per workgroup (default 200)]
// The launch has 2 x pairs workgroups in every mode: that many solo towers, `pairs` pair towers or pairs / 2 quad towers per iteration.  The members of tower t are
// the workgroups t, t + towers, t + 2 towers ..: workgroups are dealt to the XCDs round-robin, so with a multiple of 8 towers they share an XCD.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "net_dev.h"
#include "net_body.h"
#include "sim_help.h"
using namespace mz;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int H = 9, W = 9, C0 = 20, C = 64, NL = 13, P = H * W, W32 = 3;

struct Args {
    const unsigned* in;   // [samples][18][3] bit-packed planes
    const float* params;
    unsigned* help;       // [towers][helpWords]
    float* out;           // [samples][C][P] the last tower's activations
    unsigned long long* ticks; // [workgroups] 100-MHz ticks of the loop
    unsigned* xcc;        // [workgroups]
    int* err;
    int towers, iters, help_words;
};

template <int NM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void tower_loop(Args a, TowerArgs ta)
{
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    __shared__ int s_abort;
    __shared__ unsigned s_bits[18 * W32];
    const int tid = threadIdx.x;
    const int sample = NM > 1 ? blockIdx.x % a.towers : blockIdx.x, member = NM > 1 ? blockIdx.x / a.towers : 0;
    if (tid == 0) { s_abort = 0; a.xcc[blockIdx.x] = hpXccId(); }
    if (tid < 18 * W32) { s_bits[tid] = a.in[sample * 18 * W32 + tid]; }
    __syncthreads();
    HelpCtx c{a.help + size_t(sample) * a.help_words, member, 0u, &s_abort, a.err, tiles + kTowerTiles * 64 * planeStride(H, W)}; // (the hand-over slot: behind the tiles)
    const unsigned long long t0 = wall_clock64();
    const float* xt = nullptr;
    for (int it = 0; it < a.iters; ++it) {
        if constexpr (NM == 4) {
            xt = towerBodyQuad<H, W, C0, C>(s_bits, a.params, ta, tid, tiles, c);
            if (!xt) { return; }
        } else if constexpr (NM == 2) {
            xt = towerBodyPair<H, W, C0, C>(s_bits, a.params, ta, tid, tiles, c);
            if (!xt) { return; }
        } else {
            xt = towerBody<H, W, C0, C>(reinterpret_cast<const float*>(s_bits), a.params, ta, nullptr, 0, tid, tiles);
        }
        __syncthreads();
    }
    const unsigned long long t1 = wall_clock64();
    if (tid == 0) { a.ticks[blockIdx.x] = t1 - t0; }
    if (member == 0) {
        for (int i = tid; i < C * P; i += 512) {
            const int ch = i / P, p = i % P;
            a.out[size_t(sample) * C * P + i] = xt[ch * planeStride(H, W) + (p / W + 1) * (W + 2) + p % W + 1];
        }
    }
}

int main(int argc, char** argv)
{
    const int pairs = argc > 1 ? atoi(argv[1]) : 128, iters = argc > 2 ? atoi(argv[2]) : 200;
    if (pairs % 16 != 0 || pairs < 16 || pairs > 128) { fprintf(stderr, "pairs: a multiple of 16, at most 128\n"); return 2; }
    const int wgs = 2 * pairs;
    TowerArgs ta{};
    ta.nlayers = NL; ta.cin0 = 18; ta.C = C; ta.OT = 4; ta.in_bits = 1; ta.has_stem = 1;
    size_t off = 0;
    for (int l = 0; l < NL; ++l) {
        const int cg = (l == 0 ? C0 : C) / 4;
        ta.w_off[l] = unsigned(off); off += size_t(9) * 4 * cg * 64;
        ta.b_off[l] = unsigned(off); off += 64;
    }
    std::vector<float> hp(off);
    for (size_t i = 0; i < off; ++i) { hp[i] = float((i * 2654435761u) % 1000) * 1e-4f - 0.05f; }
    std::vector<unsigned> hin(size_t(wgs) * 18 * W32);
    for (size_t i = 0; i < hin.size(); ++i) { hin[i] = unsigned(i * 2246822519u + 374761393u) ^ unsigned(i >> 3) * 3266489917u; }
    Args a{};
    a.iters = iters; a.help_words = int(helpWords(C, P));
    float* params; unsigned* in;
    CK(hipMalloc(&params, off * 4)); CK(hipMemcpy(params, hp.data(), off * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&in, hin.size() * 4)); CK(hipMemcpy(in, hin.data(), hin.size() * 4, hipMemcpyHostToDevice));
    a.params = params; a.in = in;
    CK(hipMalloc(&a.help, size_t(pairs) * a.help_words * 4));
    CK(hipMalloc(&a.out, size_t(wgs) * C * P * 4));
    CK(hipMalloc(&a.ticks, wgs * 8));
    CK(hipMalloc(&a.xcc, wgs * 4));
    CK(hipMalloc(&a.err, 4)); CK(hipMemset(a.err, 0, 4));
    const size_t lds = (size_t(kTowerTiles) * 64 * planeStride(H, W) + kHpSlotFloats) * 4;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(tower_loop<1>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(tower_loop<2>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(tower_loop<4>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    std::vector<float> solo(size_t(wgs) * C * P), part(size_t(pairs) * C * P);
    std::vector<unsigned long long> ticks(wgs);
    std::vector<unsigned> xcc(wgs);
    void* kp[] = {&a, &ta};
    for (int rep = 0; rep < 3; ++rep) {
        // solo: 2 * pairs workgroups, one tower each per iteration
        a.towers = wgs;
        CK(hipLaunchCooperativeKernel(reinterpret_cast<void*>(tower_loop<1>), dim3(wgs), dim3(512), kp, unsigned(lds), nullptr));
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ticks.data(), a.ticks, wgs * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(solo.data(), a.out, solo.size() * 4, hipMemcpyDeviceToHost));
        unsigned long long mx = 0; double sum = 0;
        for (auto t : ticks) { mx = t > mx ? t : mx; sum += double(t); }
        printf("solo: %d workgroups, %.2f us per tower on average, %.2f the slowest workgroup\n", wgs, sum / wgs / 100.0 / iters, double(mx) / 100.0 / iters);
        // pair, quad: the same number of workgroups, wgs / members towers per iteration (all members of a launch must be resident: cooperative launch)
        for (int nm = 2; nm <= 4; nm += 2) {
            const int towers = wgs / nm;
            const char* name = nm == 2 ? "pair" : "quad";
            a.towers = towers;
            CK(hipMemset(a.help, 0, size_t(towers) * a.help_words * 4));
            CK(hipLaunchCooperativeKernel(nm == 2 ? reinterpret_cast<void*>(tower_loop<2>) : reinterpret_cast<void*>(tower_loop<4>), dim3(wgs), dim3(512), kp, unsigned(lds), nullptr));
            CK(hipDeviceSynchronize());
            int err = 0;
            CK(hipMemcpy(&err, a.err, 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(ticks.data(), a.ticks, wgs * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(xcc.data(), a.xcc, wgs * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(part.data(), a.out, size_t(towers) * C * P * 4, hipMemcpyDeviceToHost));
            if (err) { printf("%s: error flag %d (a member timed out)\n", name, err); return 1; }
            int split = 0;
            for (int t = 0; t < towers; ++t) {
                bool apart = false;
                for (int m = 1; m < nm; ++m) { apart = apart || xcc[t] != xcc[m * towers + t]; }
                split += apart;
            }
            mx = 0; sum = 0;
            for (int t = 0; t < towers; ++t) { mx = ticks[t] > mx ? ticks[t] : mx; sum += double(ticks[t]); }
            const bool same = memcmp(part.data(), solo.data(), size_t(towers) * C * P * 4) == 0;
            printf("%s: %d %ss, %.2f us per tower on average, %.2f the slowest owner; members on different XCDs: %d; activations %s the solo tower's\n", name, towers, name,
                   sum / towers / 100.0 / iters, double(mx) / 100.0 / iters, split, same ? "bit-identical to" : "DIFFER from");
            if (!same || split) { return 1; }
        }
    }
    return 0;
}
