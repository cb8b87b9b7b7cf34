// sim_kernel_wide, sim_kernel_wide_bf16 — the per-game simulation kernel (sim_az_body.h sim_kernel: one workgroup per game runs whole simulations — walk, leaf,
// tower, heads, candidates, expand + backup) on a ONE-TILE tower, for the AlphaZero shapes whose two activation tiles do not fit the LDS: 128 / 256 hidden channels
// (the reference's default network: 1 block x 256 channels, config/configuration.cpp:70-72), 7x7 / 13x13 / 19x19 Go (go_unit.h:11) and the board games' 11x11 and
// 15x15 boards.  Every phase function is the one sim_kernel runs (same bits); what differs is where things live:
//   LDS: [ the tower's tile — the tree phases' scratch while no tower runs ] [ reciprocal table ] [ sqrt / bias tables + path-speculation memory: if they fit ]
//        [ the simulation's path | the phases' hand-over block ] [ root superko table: if it fits ] [ the leaf's block beside the heads: if it fits ] [ heads scratch ]
//   global: the tower's two per-game activation blocks (SimArgs::act, act2; L2-resident).
// The heads cannot take their scratch from a tile here (the only tile holds the activations they read): it is a block of its own.
// One frame (simWideFrame) is the body of both kernels; a tower policy says what differs between them — the tile's size, the strides the heads read with and the
// tower function, which stays a function of its own with its own register budget:
//   WideTowerF32   the f32 tower of net_wide_body.h: the tile is wideTileFloats floats
//   WideTowerBf16  (sim_wide_bf16.inc) the opt-in bf16x3 tower of net_bf16_wide_body.h: the tile holds the tower's hi / lo buffers (64 KB at 128 channels, 128 KB at
//                  256; 44 KB at 11x11 x 64 and 76 KB at 15x15 x 64, the f32 tiles' sizes), over which the last layer leaves the f32 planes the heads read
// Two __global__ functions, not one with the policy as a parameter: the kernels keep their names.
// Compiled in parts (sim_wide_a.hip ...: each defines MZ_SIM_WIDE_PART, its number, and MZ_SIM_WIDE_CASES, its instances) so that make builds them side by side.
#include "sim_az_body.h"
#include "net_wide_body.h"

namespace mz {

template <int H, int W, int CIN0Q, int C>
__device__ __noinline__ const float* simTowerWide(CSimArgs* __restrict__ a, int g, int tid, float* tile, float* xchg)
{
    g = __builtin_amdgcn_readfirstlane(g); // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    constexpr size_t CP = size_t(C) * H * W;
    return wideTowerBody<H, W, CIN0Q, C>(reinterpret_cast<const float*>(gv.feat), a->params, *(const TowerArgs*)&a->ta, a->act + size_t(g) * CP, a->act2 + size_t(g) * CP, g, tid,
                                         tile, true);
}

template <int H, int W, int CIN0Q, int C>
struct WideTowerF32 {
    static constexpr int kPrec = 0; // Net::precision()
    static constexpr int kTileFloats = int(wideTileFloats<H, W, C>(CIN0Q));
    static constexpr int CS = WideGeo<H, W, C>::CS, PW = WideGeo<H, W, C>::PW;
    static __device__ __forceinline__ const float* run(CSimArgs* __restrict__ a, int g, int tid, float* tile, float* xchg) { return simTowerWide<H, W, CIN0Q, C>(a, g, tid, tile, xchg); }
};

// lf: bit 0 = path speculation of the walk (+ its LDS tables), bit 1 = the root's superko table in LDS, bit 2 = the second half of the Go leaf beside the heads
template <int H, int W, int CPL, class Tower>
__device__ __forceinline__ void simWideFrame(const SimArgs* a_, const uint8_t* rot_tab, int sim0, int nsims, int host_start, int lf)
{
    CSimArgs* a = (CSimArgs*)a_;
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int games = gridDim.x;
    constexpr int WPE = 2;
    double* rcp_w = reinterpret_cast<double*>(tiles + Tower::kTileFloats);
    for (int i = tid; i < a->rcp_n; i += 512) { rcp_w[i] = a->pv.rcp_tab[i]; }
    __syncthreads();
    LdsCDouble* rcp_lds = (LdsCDouble*)rcp_w;
    SpecMem spec{nullptr, nullptr, nullptr};
    int* spec_w = nullptr;
    const int path_words = 2 * a->pv.max_depth + 2;
    float* xchg = reinterpret_cast<float*>(rcp_w + a->rcp_n) + path_words;
    if (lf & 1) {
        const SpecStage st = specStage(a->pv, rcp_w, a->rcp_n, tid);
        __syncthreads();
        spec_w = st.spec_w;
        spec = st.mem(!(a->no_spec & 1));
        xchg = st.end() + path_words;
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
        const bool term = simLeafTerminal(a, xchg); // a terminal leaf: no planes, tower and heads (sim_az_body.h sim_kernel); the same barriers for every wave either way
        if constexpr (CPL > 0) { // (the other games' leaf bodies write their planes themselves)
            if (!term) {
                simLeafPlanes<CPL>(a, rot, g, wave, lane, leaf_smem ? leaf_smem : reinterpret_cast<const uint64_t*>(tiles), xchg);
                __syncthreads();
            }
        }
        if (prof) { t1 = wall_clock64(); }
        const float* xt = nullptr;
        if (!term) { xt = Tower::run(a, g, tid, tiles, xchg); }
        __syncthreads();
        if (prof) { t2 = wall_clock64(); }
        if (leaf_smem && wave >= 6) { simLeafRest<CPL>(a, rot, slot, g, lane, xchg, seen_lds, leaf_smem, 7 - wave); }
        else if (!term) { simHeads<WPE, (H * W + 1 > 128), true>(a, g, tid, hscr, xt, Tower::CS, Tower::PW, xchg); }
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
            simProfSim(prof, t0, t1, t2, t3, t4, term);
        }
    }
    if (tid == 0) { a->pv.num_nodes[g] = *node_count; }
    if (prof && tid == 0) { simProfExit(a->prof + size_t(games) * 8); }
    if (prof && tid == 0 && spec_w) { simProfSpec(prof, spec_w); }
}

template <int H, int W, int CIN0Q, int C, int CPL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void sim_kernel_wide(const SimArgs* __restrict__ a_, const uint8_t* __restrict__ rot_tab, int sim0,
                                                                                                  int nsims, int host_start, int lf)
{
    simWideFrame<H, W, CPL, WideTowerF32<H, W, CIN0Q, C>>(a_, rot_tab, sim0, nsims, host_start, lf);
}

} // namespace mz

#include "sim_wide_bf16.inc" // WideTowerBf16, sim_kernel_wide_bf16: here, because they need the frame above and the part function below needs them (templates: an f32 part instantiates none)

namespace mz {

template <auto Kernel> // sim_kernel_wide<...> or sim_kernel_wide_bf16<...>
static int launchSimWideT(const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, int lf, size_t lds, hipStream_t s)
{
    MZ_LDS_ATTR(Kernel, lds);
    hipLaunchKernelGGL(Kernel, dim3(games), dim3(512), lds, s, d_args, d_rot, sim0, nsims, host_start, lf);
    MZ_HIP(hipGetLastError());
    return MZ_OK;
}

// The parts, listed once: part n is simWideLaunchPart<n>, defined by the translation unit built with MZ_SIM_WIDE_PART == n and tried in this order (sim_wide_a.hip)
#define MZ_SIM_WIDE_PARTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#define MZ_SIM_WIDE_FN(n) simWideLaunchPart##n
#define MZ_SIM_WIDE_SIG(n)                                                                                                                                                    \
    bool MZ_SIM_WIDE_FN(n)(int H, int W, int c0q, int C, int cpl, int prec, const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, int lf, size_t lds, \
                           hipStream_t s, size_t* tile_bytes, int* rc, int* spec_words)
#define MZ_SIM_WIDE_SIG_OF(n) MZ_SIM_WIDE_SIG(n) // (expands MZ_SIM_WIDE_PART before it is pasted)

// A part's instances, MZ_SIM_WIDE_CASES(X) of its .hip: X(tower, H, W, input channels of the stem padded to 16, hidden channels, the rules argument: game_kind.h
// rulesArg); tower: f32 or bf16, the instance of Net::precision() 0 or 1
#define MZ_SIM_WIDE_TOWER_f32 WideTowerF32
#define MZ_SIM_WIDE_TOWER_bf16 WideTowerBf16
#define MZ_SIM_WIDE_KERNEL_f32 sim_kernel_wide
#define MZ_SIM_WIDE_KERNEL_bf16 sim_kernel_wide_bf16

// true: this part holds the instance (launched when d_args != nullptr; d_args == nullptr: a query, *tile_bytes = the LDS bytes of the tower's tile, *spec_words = the
// words of the walk's speculation memory as this translation unit was built)
MZ_SIM_WIDE_SIG_OF(MZ_SIM_WIDE_PART)
{
#define MZ_SIM_WIDE_ONE(t, h, w, cin0q, c, cp)                                                                                                     \
    if (H == h && W == w && c0q == cin0q && C == c && cpl == cp && prec == MZ_SIM_WIDE_TOWER_##t<h, w, cin0q, c>::kPrec) {                         \
        if (tile_bytes) { *tile_bytes = MZ_SIM_WIDE_TOWER_##t<h, w, cin0q, c>::kTileFloats * sizeof(float); }                                      \
        if (spec_words) { *spec_words = kSpecWords; } /* of THIS translation unit (MZ_SPEC_WAYS) */                                                \
        if (d_args) { *rc = launchSimWideT<&MZ_SIM_WIDE_KERNEL_##t<h, w, cin0q, c, cp>>(d_args, games, d_rot, sim0, nsims, host_start, lf, lds, s); } \
        return true;                                                                                                                               \
    }
    MZ_SIM_WIDE_CASES(MZ_SIM_WIDE_ONE)
#undef MZ_SIM_WIDE_ONE
    return false;
}

} // namespace mz
