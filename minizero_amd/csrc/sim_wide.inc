// sim_kernel_wide — the per-game simulation kernel (sim_az_body.h sim_kernel: one workgroup per game runs whole simulations — walk, Go leaf, tower, heads,
// candidates, expand + backup) on the ONE-TILE tower of net_wide_body.h, for the AlphaZero shapes whose two activation tiles do not fit the LDS:
// 128 / 256 hidden channels (the reference's default network: 1 block x 256 channels, config/configuration.cpp:70-72) and 7x7 / 13x13 / 19x19 Go
// (go_unit.h:11).  Every phase function is the one sim_kernel runs (same bits); what differs is where things live:
//   LDS: [ the tower's tile — the tree phases' scratch while no tower runs ] [ reciprocal table ] [ sqrt / bias tables + path-speculation memory: if they fit ]
//        [ the simulation's path | the phases' hand-over block ] [ root superko table: if it fits ] [ the leaf's block beside the heads: if it fits ] [ heads scratch ]
//   global: the tower's two per-game activation blocks (SimArgs::act, act2; L2-resident).
// The heads cannot take their scratch from a tile here (the only tile holds the activations they read): it is a block of its own.
// Compiled in parts (sim_wide_a.hip ...: MZ_SIM_WIDE_PART selects the instances) so that make builds them side by side.
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

// lf: bit 0 = path speculation of the walk (+ its LDS tables), bit 1 = the root's superko table in LDS, bit 2 = the second half of the Go leaf beside the heads
template <int H, int W, int CIN0Q, int C, int CPL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 4))) void sim_kernel_wide(const SimArgs* __restrict__ a_, const uint8_t* __restrict__ rot_tab, int sim0,
                                                                                                  int nsims, int host_start, int lf)
{
    using G = WideGeo<H, W, C>;
    CSimArgs* a = (CSimArgs*)a_;
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int games = gridDim.x;
    constexpr int WPE = 2;
    constexpr int kTileFloats = int(wideTileFloats<H, W, C>(CIN0Q));
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
    if constexpr (CPL > 0) {
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
        if constexpr (CPL > 0) {
            if (!term) {
                simLeafPlanes<CPL>(a, rot, g, wave, lane, leaf_smem ? leaf_smem : reinterpret_cast<const uint64_t*>(tiles), xchg);
                __syncthreads();
            }
        }
        if (prof) { t1 = wall_clock64(); }
        const float* xt = nullptr;
        if (!term) { xt = simTowerWide<H, W, CIN0Q, C>(a, g, tid, tiles, xchg); } // its own function: its own register budget
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
            // (a terminal leaf's second half, alone where the heads would be, counts as leaf time: "tower" and "heads" only hold simulations that ran them)
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
static int launchSimWideT(const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, int lf, size_t lds, hipStream_t s)
{
    MZ_LDS_ATTR((sim_kernel_wide<H, W, CIN0Q, C, CPL>), lds);
    hipLaunchKernelGGL((sim_kernel_wide<H, W, CIN0Q, C, CPL>), dim3(games), dim3(512), lds, s, d_args, d_rot, sim0, nsims, host_start, lf);
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

// instances by part: (H, W, input channels of the stem padded to 16, hidden channels, the rules argument: game_kind.h rulesArg); prec: Net::precision() — the
// parts of sim_kernel_wide hold the f32 tower's instances, parts 6, 7 and 10 to 12 (sim_wide_bf16.inc) those of sim_kernel_wide_bf16
#if MZ_SIM_WIDE_PART == 0
#define MZ_SIM_WIDE_PART_CASES(X) X(9, 9, 32, 128, 2) X(9, 9, 32, 32, 2) X(7, 7, 32, 128, 1) X(13, 13, 32, 64, 3)
#elif MZ_SIM_WIDE_PART == 1
#define MZ_SIM_WIDE_PART_CASES(X) X(7, 7, 32, 32, 1) X(7, 7, 32, 64, 1) X(7, 7, 32, 256, 1)
#elif MZ_SIM_WIDE_PART == 2 // (built with MZ_SPEC_WAYS = 4: the shapes whose tile leaves too little LDS for sixteen remembered paths)
#define MZ_SIM_WIDE_PART_CASES(X) X(19, 19, 32, 64, 6) X(19, 19, 32, 32, 6) X(13, 13, 32, 128, 3) X(9, 9, 32, 256, 2)
#elif MZ_SIM_WIDE_PART == 3 // Othello and TicTacToe at the reference's default width: the same phase functions as sim_kernel's
#define MZ_SIM_WIDE_PART_CASES(X) X(8, 8, 16, 128, kRulesOthello) X(8, 8, 16, 256, kRulesOthello) X(3, 3, 16, 128, kRulesTicTacToe) X(3, 3, 16, 256, kRulesTicTacToe)
#elif MZ_SIM_WIDE_PART == 4 // Gomoku on its default 15x15 board: 64 channels (measured), 32 (tests)
#define MZ_SIM_WIDE_PART_CASES(X) X(15, 15, 16, 64, kRulesGomoku) X(15, 15, 16, 32, kRulesGomoku)
#elif MZ_SIM_WIDE_PART == 5 // Hex on its default 11x11 board: 64 channels (measured), 32 (tests), 128
#define MZ_SIM_WIDE_PART_CASES(X) X(11, 11, 16, 64, kRulesHex) X(11, 11, 16, 32, kRulesHex) X(11, 11, 16, 128, kRulesHex)
#elif MZ_SIM_WIDE_PART == 8 // NoGo (a rules variant of Go: game_kind.h) on Go's 9x9 networks: 256 channels (the reference's default network), 128, 32 (tests); MZ_SPEC_WAYS = 4
#define MZ_SIM_WIDE_PART_CASES(X) X(9, 9, 32, 256, kRulesNoGo) X(9, 9, 32, 128, kRulesNoGo) X(9, 9, 32, 32, kRulesNoGo)
#elif MZ_SIM_WIDE_PART == 9 // Havannah (a game past the rows: game_kind.h): edge size 8 on its 15x15 array with 64 channels (measured) and 32, edge size 4 (7x7) with 32 (tests); 20 planes pad to 32
#define MZ_SIM_WIDE_PART_CASES(X) X(15, 15, 32, 64, kRulesHavannah) X(15, 15, 32, 32, kRulesHavannah) X(7, 7, 32, 32, kRulesHavannah)
#elif MZ_SIM_WIDE_PART == 6 || MZ_SIM_WIDE_PART == 7 || (MZ_SIM_WIDE_PART >= 10 && MZ_SIM_WIDE_PART <= 12) // the bf16x3 tower: sim_wide_bf16.inc defines the kernel, its instances and the part's function
#else
#error "MZ_SIM_WIDE_PART: not one of MZ_SIM_WIDE_PARTS"
#endif

// true: this part holds the instance (launched when d_args != nullptr; d_args == nullptr: a query, *tile_bytes = the LDS bytes of the tower's tile, *spec_words = the
// words of the walk's speculation memory as this translation unit was built)
#ifdef MZ_SIM_WIDE_PART_CASES
MZ_SIM_WIDE_SIG_OF(MZ_SIM_WIDE_PART)
{
#define MZ_SIM_WIDE_ONE(h, w, cin0q, c, cp)                                                                                                        \
    if (H == h && W == w && c0q == cin0q && C == c && cpl == cp && prec == 0) {                                                                    \
        if (tile_bytes) { *tile_bytes = wideTileFloats<h, w, c>(cin0q) * sizeof(float); }                                                          \
        if (spec_words) { *spec_words = kSpecWords; } /* of THIS translation unit (MZ_SPEC_WAYS) */                                                \
        if (d_args) { *rc = launchSimWideT<h, w, cin0q, c, cp>(d_args, games, d_rot, sim0, nsims, host_start, lf, lds, s); }                       \
        return true;                                                                                                                               \
    }
    MZ_SIM_WIDE_PART_CASES(MZ_SIM_WIDE_ONE)
#undef MZ_SIM_WIDE_ONE
    return false;
}
#endif

} // namespace mz
