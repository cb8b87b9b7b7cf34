// sim_kernel_wide_bf16 — sim_kernel_wide (sim_wide.inc) with the opt-in bf16x3 tower of net_bf16_wide_body.h: 9x9 Go AlphaZero with 128 / 256 hidden channels,
// Gomoku 15x15, Hex 11x11 and Havannah 15x15 with 64 under `mz_nn_precision=bf16x3`.  Every tree phase is the one sim_kernel and sim_kernel_wide run; the LDS plan is sim_kernel_wide's (lf; Net::simWidePlan) around
// another tile: the tower's hi / lo buffers (64 KB at 128 channels, 128 KB at 256; 44 KB at 11x11 x 64 and 76 KB at 15x15 x 64, the f32 tiles' sizes), over which the last layer leaves the f32 planes the heads read.  The tower
// body is the stand-alone launch's (net_bf16_wide.hip) — same code, same order, same bits: the lock-step mode on the bf16x3 tower writes the same records.
// A kernel of its own, not a template parameter of sim_kernel_wide: the f32 kernels keep their names and their code.
#include "sim_wide.inc"
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

// lf: as sim_kernel_wide
template <int H, int W, int CIN0Q, int C, int CPL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void sim_kernel_wide_bf16(const SimArgs* __restrict__ a_, const uint8_t* __restrict__ rot_tab, int sim0,
                                                                                                       int nsims, int host_start, int lf)
{
    using G = Bf16WideGeo<H, W, C>;
    CSimArgs* a = (CSimArgs*)a_;
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int games = gridDim.x;
    constexpr int WPE = 2;
    constexpr int kTileFloats = G::kTileBytes / 4;
    double* rcp_w = reinterpret_cast<double*>(tiles + kTileFloats);
    for (int i = tid; i < a->rcp_n; i += 512) { rcp_w[i] = a->pv.rcp_tab[i]; }
    __syncthreads();
    LdsCDouble* rcp_lds = (LdsCDouble*)rcp_w;
    SpecMem spec{nullptr, nullptr, nullptr};
    int* spec_w = nullptr;
    const int path_words = 2 * a->pv.max_depth + 2;
    float* xchg = reinterpret_cast<float*>(rcp_w + a->rcp_n) + path_words;
    if (lf & 1) {
        const int tab_n = a->rcp_n - 2;
        double* sqrt_w = rcp_w + a->rcp_n;
        float* bias_w = reinterpret_cast<float*>(sqrt_w + tab_n);
        spec_w = reinterpret_cast<int*>(bias_w + tab_n + (tab_n & 1));
        for (int i = tid; i < tab_n; i += 512) { sqrt_w[i] = a->pv.sqrt_tab[i]; bias_w[i] = a->pv.bias_tab[i]; }
        if (tid < kSpecWays) { spec_w[tid * kSpecWay] = 0; }
        if (tid < 8) { spec_w[kSpecWays * kSpecWay + tid] = 0; }
        if (tid < kHelpSegs) { spec_w[kSpecHelp + tid * kHelpSeg] = 0; }
        __syncthreads();
        spec = SpecMem{(a->no_spec & 1) ? nullptr : (LdsI32*)spec_w, (LdsCFloat*)bias_w, (LdsCDbl*)sqrt_w};
        xchg = reinterpret_cast<float*>(spec_w + kSpecWords) + path_words;
    }
    float* next = xchg + ((simXchgWordsDev(a->gv.A, a->gv.channels, a->gv.W32) + 1) & ~1);
    const uint64_t* seen_lds = nullptr;
    if constexpr (CPL > 0) { // (the superko table and the leaf's block are Go's)
        if (lf & 2) {
            uint64_t* sw = reinterpret_cast<uint64_t*>(next);
            for (int i = tid; i < kGoSeenCap; i += 512) { sw[i] = a->gv.snap[g].seen[i]; }
            __syncthreads();
            seen_lds = sw;
            next = reinterpret_cast<float*>(sw + kGoSeenCap);
        }
    }
    uint64_t* leaf_smem = nullptr;
    if constexpr (CPL > 0) {
        if ((lf & 4) && !(a->no_spec & 8)) {
            leaf_smem = reinterpret_cast<uint64_t*>(next);
            uint64_t* zk = leaf_smem + goLeafKeyWord(a->gv.Ppad, a->gv.W, a->pv.max_depth); // the block's copy of the Zobrist keys (go_body.h)
            for (int i = tid; i < 2 * a->gv.P; i += 512) { zk[i] = a->gv.key[i]; }
            __syncthreads();
            next = reinterpret_cast<float*>(zk + 2 * a->gv.P); // (goLeafSmemBytes: the body's arrays, then the keys)
        }
    }
    float* const hscr = next; // the heads' scratch: (PC * P + P + VH + A + 16) floats
    unsigned long long* prof = a->prof ? a->prof + size_t(g) * 8 : nullptr;
    int* const node_count = reinterpret_cast<int*>(xchg) - 1; // (the spare word of the path block: simPathView)
    if (tid == 0) { *node_count = a->pv.num_nodes[g]; }
    if (prof && tid == 0) { simProfEnter(a->prof + size_t(games) * 8); }
    __syncthreads();
    for (int s = 0; s < nsims; ++s) {
        const int slot = sim0 + s; // simulation index within the move = position slot of its leaf
        const int rot = rot_tab[size_t(s) * games + g];
        unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        if (prof) { t0 = wall_clock64(); }
        if (wave == 0) {
            if (slot == 1 && a->root_noise) { simApplyRootNoise<WPE>(a, g, lane); }
            if (a->use_gumbel) { simGumbelStart<WPE>(a, slot, s == 0 && host_start != 0, g, lane, tiles); }
            simSelectLeaf<CPL, WPE>(a, rot, slot, g, lane, tiles, rcp_lds, spec, xchg, seen_lds, (a->no_spec & 2) ? 0 : s + 1, leaf_smem);
        } else if (wave <= kHelpSegs && spec.w && !(a->no_spec & 2)) {
            simSelectHelper(a, g, lane, wave, s + 1, rcp_lds, spec);
        }
        __syncthreads();
        const bool term = simLeafTerminal(a, xchg); // a terminal leaf: no planes, tower and heads; the same barriers for every wave either way
        if constexpr (CPL > 0) { // (the other games' leaf bodies write their planes themselves: sim_wide.inc)
            if (!term) {
                simLeafPlanes<CPL>(a, rot, g, wave, lane, leaf_smem ? leaf_smem : reinterpret_cast<const uint64_t*>(tiles), xchg);
                __syncthreads();
            }
        }
        if (prof) { t1 = wall_clock64(); }
        const float* xt = nullptr;
        if (!term) { xt = simTowerWideBf16<H, W, C>(a, g, tid, tiles, xchg); } // its own function: its own register budget
        __syncthreads();
        if (prof) { t2 = wall_clock64(); }
        if (leaf_smem && wave >= 6) { simLeafRest<CPL>(a, rot, slot, g, lane, xchg, seen_lds, leaf_smem, 7 - wave); }
        else if (!term) { simHeads<WPE, (H * W + 1 > 128), true>(a, g, tid, hscr, xt, G::CS, G::PW, xchg); }
        else if (leaf_smem) { __syncthreads(); __syncthreads(); } // (the two barriers of the leaf's second half on waves 6 and 7)
        __syncthreads();
        if (prof) { t3 = wall_clock64(); }
        if (wave == 0) { simCandGather<WPE>(a, rot, g, lane, tiles, xchg); }
        __syncthreads();
        {
            const int A = a->gv.A;
            const SimXchg x{A + (A & 1)};
            if (a->cand_coop) { simCandRank(A, reinterpret_cast<const int*>(xchg + x.scalars())[1], wave, lane, tiles, a->cand_coop); }
        }
        __syncthreads();
        {
            const bool split = !a->pv.value_rescale; // backup beside expand on a second wave
            if (wave == 0) { simCandExpand<WPE>(a, rot, slot, g, lane, tiles, xchg, split ? 1 : 0); }
            else if (wave == 1 && split) { simBackupOnly<WPE>(a, slot, g, lane, tiles, xchg); }
        }
        __syncthreads();
        if (prof && tid == 0) {
            t4 = wall_clock64();
            prof[0] += t1 - t0 + (term ? t3 - t1 : 0); prof[1] += term ? 0 : t2 - t1; prof[2] += term ? 0 : t3 - t2; prof[3] += t4 - t3;
            prof[4] += 1 + (static_cast<unsigned long long>(term) << 32); // simulations | those whose network evaluation was skipped
        }
    }
    if (tid == 0) { a->pv.num_nodes[g] = *node_count; }
    if (prof && tid == 0) { simProfExit(a->prof + size_t(games) * 8); }
    if (prof && tid == 0 && spec_w) {
        prof[7] += (static_cast<unsigned long long>(spec_w[kSpecWays * kSpecWay + 1]) << 40) | (static_cast<unsigned long long>(spec_w[kSpecWays * kSpecWay + 5]) << 20) | spec_w[kSpecWays * kSpecWay + 3];
        prof[6] += static_cast<unsigned long long>(spec_w[kSpecWays * kSpecWay + 7]) << 40;
    }
}

template <int H, int W, int CIN0Q, int C, int CPL>
static int launchSimWideBf16T(const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, int lf, size_t lds, hipStream_t s)
{
    MZ_LDS_ATTR((sim_kernel_wide_bf16<H, W, CIN0Q, C, CPL>), lds);
    hipLaunchKernelGGL((sim_kernel_wide_bf16<H, W, CIN0Q, C, CPL>), dim3(games), dim3(512), lds, s, d_args, d_rot, sim0, nsims, host_start, lf);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

// the part's instance: MZ_SIM_WIDE_BF16_CASE = (H, W, input channels of the stem padded to 16, hidden channels, the rules argument)
MZ_SIM_WIDE_SIG_OF(MZ_SIM_WIDE_PART)
{
#define MZ_SIM_WIDE_BF16_ONE(h, w, cin0q, c, cp)                                                                                                   \
    if (H == h && W == w && c0q == cin0q && C == c && cpl == cp && prec == 1) {                                                                    \
        if (tile_bytes) { *tile_bytes = Bf16WideGeo<h, w, c>::kTileBytes; }                                                                        \
        if (spec_words) { *spec_words = kSpecWords; } /* of THIS translation unit (MZ_SPEC_WAYS) */                                                \
        if (d_args) { *rc = launchSimWideBf16T<h, w, cin0q, c, cp>(d_args, games, d_rot, sim0, nsims, host_start, lf, lds, s); }                   \
        return true;                                                                                                                               \
    }
    MZ_SIM_WIDE_BF16_CASE(MZ_SIM_WIDE_BF16_ONE)
#undef MZ_SIM_WIDE_BF16_ONE
    return false;
}

} // namespace mz
