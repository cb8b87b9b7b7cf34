// The device side of the AlphaZero per-game simulation kernel (sim_kernel and the phase functions it shares with the MuZero kernels of sim.hip), as a header:
// sim.hip instantiates the BASELINE shapes (two-tile tower), sim_wide.hip the wide / large-board shapes (one-tile tower, net_wide_body.h).
#pragma once
// sim_kernel — the per-game simulation kernel: workgroup g runs `nsims` complete MCTS simulations of game g without leaving
// the GPU: PUCT selection, the leaf's Go position / planes / legal mask, the residual tower + heads on the 8 waves of the
// workgroup, the candidate list and expand + backup.  The reference steps all games in lock-step, one batched forward per
// cycle (ref actor/actor_group.cpp:81-114); nothing in a game depends on another game, so here every game advances at its own
// pace: a simulation costs ITS path depth, not the deepest of the 256 paths, there are no kernel boundaries inside a move, and
// the tower of one game overlaps the tree phases of the others.  The per-sample arithmetic is that of the stand-alone kernels
// (same device bodies: net_body.h, pool_body.h, go_body.h), so results are bit-identical to the lock-step path.
// The host draws the per-cycle feature rotations in the reference's order (cycle-major, actor-minor) before the launch.
#include "net.h"
#ifdef MZ_SIM_TPROF // experiment: cycles per tower layer inside the simulation kernel (game 0, wave 0), printed by dumpSimProf
__device__ unsigned long long g_tp[64];
__shared__ unsigned long long s_tp_prev;
__shared__ int s_tp_idx;
#define MZ_TPROF(slot)                                                                         \
    do {                                                                                       \
        if ((slot) == 3 && threadIdx.x == 0 && blockIdx.x == 0) {                              \
            const unsigned long long t_ = clock64();                                           \
            g_tp[s_tp_idx & 63] += t_ - s_tp_prev; s_tp_prev = t_; ++s_tp_idx;                 \
        }                                                                                      \
    } while (0)
#endif
#ifdef MZ_SIM_HPROF // experiment: where the time of the in-kernel 601-bin heads goes (game 0)
#ifndef MZ_HPROF_BLOCK
#define MZ_HPROF_BLOCK 0 // cluster mode: 64 = member 1 (reward head) of game 0 in a pool of 64 games
#endif
__device__ unsigned long long g_hp[16];
__shared__ unsigned long long s_hp_prev;
#define MZ_HPROF(k)                                                                                   \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.x == MZ_HPROF_BLOCK) {                                       \
            const unsigned long long t_ = wall_clock64();                                             \
            if ((k) > 0) { g_hp[(k)] += t_ - s_hp_prev; } else { g_hp[15] += 1; }                     \
            s_hp_prev = t_;                                                                           \
        }                                                                                             \
    } while (0)
#endif
#include "net_body.h"
#include "net_bf16_body.h"
#include "net_atari_body.h"
#ifdef MZ_SIM_LPROF // experiment: where the time of the single-wave tree phases goes (game 0)
__device__ unsigned long long g_lp[32];
__shared__ unsigned long long s_lp_prev;
#define MZ_LPROF(k)                                                                                   \
    do {                                                                                              \
        if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) {                                             \
            const unsigned long long t_ = wall_clock64();                                             \
            if ((k) > 0) { g_lp[(k)] += t_ - s_lp_prev; } else { g_lp[31] += 1; }                     \
            s_lp_prev = t_;                                                                           \
        }                                                                                             \
    } while (0)
#endif
#ifdef MZ_SIM_BPROF // experiment: the part of the Go leaf that runs beside the heads (game 0): [role][0] entry -> start, [1] first piece, [2] wait at barrier 1, [3] legal mask, [4] wait at barrier 2
__device__ unsigned long long g_bp[20];
#define MZ_BPROF(role, k)                                                                              \
    do {                                                                                               \
        if (PART == 2 && (threadIdx.x & 63) == 0 && blockIdx.x == 0) {                                 \
            const unsigned long long t_ = wall_clock64();                                              \
            if ((k) == 0) { g_bp[16 + (role)] += 1; g_bp[18 + (role)] = t_; }                          \
            else { g_bp[(role) * 8 + (k)] += t_ - g_bp[18 + (role)]; g_bp[18 + (role)] = t_; }        \
        }                                                                                              \
    } while (0)
#endif
#include "pool_body.h"
#include "go_body.h"
#include "gumbel_body.h"
#include "sim_args.h"
#include "sim_help.h"
#include <algorithm>
#include <type_traits>
#include <cstring>
#include <cstdlib>
#include <vector>

#ifndef MZ_HEADS_FP
#define MZ_HEADS_FP 0 // (experiment switch: the two-tile 9x9 kernels' heads with global / DS loads instead of flat loads)
#endif

namespace mz {


// The heads' outputs and the candidate list of a simulation never leave the CU: they are handed from phase to phase through a small LDS
// block instead of global memory (each hand-over was a store + a dependent load through L2).  The bodies index their arrays with the
// game index, so they get generic pointers moved back by the game's offset.
struct SimXchg { // word offsets inside the block for A actions
    int A;
    __device__ int policy() const { return 0; }
    __device__ int logit() const { return A; }
    __device__ int cpolicy() const { return 2 * A; }
    __device__ int clogit() const { return 3 * A; }
    __device__ int caction() const { return 4 * A; }
    __device__ int scalars() const { return 5 * A; } // value, cand_count, cand_player, value_io, reward_io, leaf_player, terminal, eval, + the backup wave's value / reward
    __device__ int legal() const { return 5 * A + 12; }   // 64-bit words of the leaf's legal mask (8-byte aligned: A is padded to even below)
    __device__ int feat() const { return 5 * A + 12 + 16; } // the leaf's bit-packed planes (the tower's input)
};
inline size_t simXchgWords(int A, int channels, int W32) { return size_t(5) * (A + (A & 1)) + 12 + 16 + size_t(channels) * W32; }
__device__ __forceinline__ int simXchgWordsDev(int A, int channels, int W32) { return 5 * (A + (A & 1)) + 12 + 16 + channels * W32; }


// the leaf's outputs (planes, legal mask, player, terminal flag, result) go to the next phases through the hand-over block too
__device__ __forceinline__ GoDevView simLeafView(GoDevView gv, float* xchg, int g)
{
    const SimXchg x{gv.A + (gv.A & 1)};
    float* sc = xchg + x.scalars();
    gv.leaf_player = reinterpret_cast<int*>(sc + 5) - g;
    gv.terminal = reinterpret_cast<int*>(sc + 6) - g;
    gv.eval = sc + 7 - g;
    gv.legal = reinterpret_cast<uint64_t*>(xchg + x.legal()) - size_t(g) * gv.LW;
    gv.feat = reinterpret_cast<uint32_t*>(xchg + x.feat()) - size_t(g) * gv.channels * gv.W32;
    return gv;
}

// The tree phases are separate (non-inlined) functions: inlined next to the tower they push the kernel to 256 VGPRs with spills in
// the MFMA loop.  SimArgs lives in device memory (not in 1.3 KB of kernel arguments pinned in SGPRs for the whole kernel).
typedef __attribute__((address_space(3))) const double LdsCDouble;

template <int CPL, int WPE, class RcpPtr>
__device__ __noinline__ void simSelectLeaf(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, float* tiles, RcpPtr rcp, SpecMem spec,
                                           float* xchg, const uint64_t* seen_lds, int serial = 0, uint64_t* leaf_smem = nullptr)
{
    serial = __builtin_amdgcn_readfirstlane(serial);
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    rot = __builtin_amdgcn_readfirstlane(rot);
    unsigned long long t0 = 0;
    if (a->prof) { t0 = wall_clock64(); }
    const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
#ifdef MZ_SELECT_TWICE // experiment: the walk again, now with its records in the caches -> the profile shows the arithmetic-only time
    selectBody<WPE == 2>(pv, a->use_gumbel ? a->start : nullptr, g, lane, rcp, spec);
    waveSync();
    if (a->prof) { t0 = wall_clock64(); }
#endif
    selectBody<WPE == 2>(pv, a->use_gumbel ? a->start : nullptr, g, lane, rcp, spec, serial);
    waveSync();
    if (a->prof && lane == 0) {
        a->prof[size_t(g) * 8 + 5] += wall_clock64() - t0;
        a->prof[size_t(g) * 8 + 6] += pv.path_len[g];
    }
    MZ_LPROF(0);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    if constexpr (CPL <= 0) { leafBody<CPL>(gv, pv, rot, slot, g, lane); } // the two-bitboard games (game_kind.h rulesArg)
    else if (leaf_smem) { leafBody<CPL, true, 1>(gv, pv, rot, slot, g, lane, leaf_smem, seen_lds); } // what the network needs; the rest beside the heads (simLeafRest)
    else { leafBody<CPL, true>(gv, pv, rot, slot, g, lane, reinterpret_cast<uint64_t*>(tiles), seen_lds); } // planes: simLeafPlanes, all waves
}

// Go, one game per CU: what only the phases after the network need of the leaf — path hashes, liberties, legal mask, a terminal leaf's score (go_body.h
// leafBody PART 2) — on the workgroup's last two waves BESIDE the heads, in which those waves have no share.  They pass the two barriers headsBody passes.
template <int CPL>
__device__ __noinline__ void simLeafRest(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, float* xchg, const uint64_t* seen_lds, uint64_t* leaf_smem, int role)
{
    role = __builtin_amdgcn_readfirstlane(role);
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    rot = __builtin_amdgcn_readfirstlane(rot);
    if constexpr (CPL > 0) {
        const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
        const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
        if (role == 0) { leafBody<CPL, true, 2, true, 0>(gv, pv, rot, slot, g, lane, leaf_smem, seen_lds); }
        else { leafBody<CPL, true, 2, true, 1>(gv, pv, rot, slot, g, lane, leaf_smem, seen_lds); }
    }
}

// waves 1 .. 3 beside wave 0's walk: levels 17 .. 64 of the path the previous simulation took, 16 per wave (pool_body.h selectSpecHelper): a deep principal variation is
// re-walked by almost every simulation, and the launch lasts as long as its deepest game
template <class RcpPtr>
__device__ __noinline__ void simSelectHelper(CSimArgs* __restrict__ a, int g, int lane, int seg, int serial, RcpPtr rcp, SpecMem spec)
{
    g = __builtin_amdgcn_readfirstlane(g);
    seg = __builtin_amdgcn_readfirstlane(seg);
    serial = __builtin_amdgcn_readfirstlane(serial);
    const PoolView pv = ldc(&a->pv);
    selectSpecHelper(pv, g, lane, seg, serial, rcp, spec);
}

// Go: the 18 feature planes of the leaf, two or three per wave (32 ballots over LDS words: 3.3 us on one wave)
template <int CPL>
__device__ __forceinline__ void simLeafPlanes(CSimArgs* __restrict__ a, int rot, int g, int wave, int lane, const uint64_t* leaf_smem, float* xchg)
{
    if constexpr (CPL > 0) {
        const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
        goPlanesPart<CPL>(gv, a->pv.max_depth, rot, g, wave, 8, lane, leaf_smem);
    }
}

// Candidates + expand + backup in three steps: wave 0 gathers the legal actions, ALL waves count ranks (the sort is VALU-bound and the other
// seven waves would be idle), wave 0 scatters, expands and backs up.  A > 128 actions: wave 0 sorts alone in the first step.
__device__ __forceinline__ float* simCandDense(float* tiles, int A) { return reinterpret_cast<float*>(reinterpret_cast<char*>(tiles) + ((2 * size_t(A) * sizeof(Cand) + kSortStackBytes + 16 + 15) & ~size_t(15))); }

template <int WPE>
__device__ __forceinline__ void simCandGatherImpl(CSimArgs* __restrict__ a, int rot, int g, int lane, float* tiles, float* xchg)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    rot = __builtin_amdgcn_readfirstlane(rot);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    const SimXchg x{gv.A + (gv.A & 1)};
    const size_t ga = size_t(g) * gv.A;
    float* sc = xchg + x.scalars();
    MZ_LPROF(6);
    Cand* cs = reinterpret_cast<Cand*>(tiles);
    const int k = azCandGather(gv, xchg + x.policy() - ga, xchg + x.logit() - ga, rot, g, lane, cs);
    waveSync();
    // (cand_coop 2: boards of more than 128 actions — up to six candidates per lane, candRankPartW)
    if (a->cand_coop == 2 && k > 0 && k <= kCandCoopMaxW) { candDenseW(cs, k, lane, simCandDense(tiles, gv.A)); }
    else if (k > kCandCoopMax || !a->cand_coop) { if (k > 0) { orderCandidates(cs, cs + gv.A, reinterpret_cast<int*>(cs + 2 * gv.A), k, lane, a->err); } }
    else { candDense(cs, k, lane, simCandDense(tiles, gv.A)); }
    if (lane == 0) { reinterpret_cast<int*>(sc)[1] = k; } // cand_count: read by every wave after the barrier
    MZ_LPROF(7);
}

// (a function of its own with its own register budget.  It saves and restores the callee-saved VGPRs it uses — 25 here, 78 in simCandExpand, 256 bytes each per call, one
// wave — which is what is left of BASELINE configs[2]'s HBM traffic; calling the bodies inline in the 128-VGPR kernels was measured and lost: the kernel then spills 47
// VGPRs whose reloads sit in these single-wave phases — 32.5 -> 47.8 MB per cycle, 2.03 -> 2.02 M leaf-evals/s)
template <int WPE>
__device__ __noinline__ void simCandGather(CSimArgs* __restrict__ a, int rot, int g, int lane, float* tiles, float* xchg)
{
    simCandGatherImpl<WPE>(a, rot, g, lane, tiles, xchg);
}

__device__ __forceinline__ void simCandRank(int A, int k, int wave, int lane, float* tiles, int coop = 1)
{
    if (coop == 2) {
        if (k > 0 && k <= kCandCoopMaxW) { float* dense = simCandDense(tiles, A); candRankPartW(dense, k, wave, 8, lane, reinterpret_cast<int*>(dense + kCandCoopMaxW)); }
        return;
    }
    if (k <= 0 || k > kCandCoopMax) { return; }
    float* dense = simCandDense(tiles, A);
    candRankPart(dense, k, wave, 8, lane, reinterpret_cast<int*>(dense + kCandCoopMax));
}

// The backup of a simulation on its own wave (wave 1) beside wave 0's scatter + expand: it only needs the leaf's value (the heads' output, or
// the game result at a terminal leaf: zero_actor.cpp:85) and the path.  Not with value rescaling (its multiset shares the scratch).
template <int WPE>
__device__ __noinline__ void simBackupOnly(CSimArgs* __restrict__ a, int slot, int g, int lane, float* tiles, float* xchg)
{
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
    const SimXchg x{gv.A + (gv.A & 1)};
    float* sc = xchg + x.scalars();
    if (lane == 0) {
        sc[8] = gv.terminal[g] != 0 ? gv.eval[g] : sc[0];
        sc[9] = 0.0f; // board games have no rewards (go.h:50)
    }
    waveSync();
    expandBackupBody(pv, nullptr, nullptr, nullptr, nullptr, nullptr, sc + 8 - g, sc + 9 - g, slot, a->err, g, lane, tiles, 2);
}

// (simCandPipeVf below repeats these steps — scatter, azCandStore, expand — with its own path view: a change here belongs there too.  It does not call this
//  function because a second set of constant arguments would change how the shared bodies are compiled for every caller.)
template <int WPE>
__device__ __forceinline__ void simCandExpandImpl(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, float* tiles, float* xchg, int part)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    rot = __builtin_amdgcn_readfirstlane(rot);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
    const SimXchg x{gv.A + (gv.A & 1)};
    const size_t ga = size_t(g) * gv.A;
    float* sc = xchg + x.scalars();
    int* cand_count = reinterpret_cast<int*>(sc + 1) - g;
    int* cand_player = reinterpret_cast<int*>(sc + 2) - g;
    int* cand_action = reinterpret_cast<int*>(xchg + x.caction()) - ga;
    Cand* cs = reinterpret_cast<Cand*>(tiles);
    Cand* out = cs + gv.A;
    const int k = reinterpret_cast<const int*>(sc)[1];
    if (a->cand_coop == 2) {
        if (k > 0 && k <= kCandCoopMaxW) {
            float* dense = simCandDense(tiles, gv.A);
            candScatterW(cs, out, reinterpret_cast<int*>(out + gv.A), k, 8, lane, reinterpret_cast<const int*>(dense + kCandCoopMaxW), a->err);
        }
    } else if (k > 0 && k <= kCandCoopMax && a->cand_coop) {
        float* dense = simCandDense(tiles, gv.A);
        candScatter(cs, out, reinterpret_cast<int*>(out + gv.A), k, 8, lane, reinterpret_cast<const int*>(dense + kCandCoopMax), a->err);
    }
    MZ_LPROF(8);
    azCandStore(gv, sc - g, out, k, cand_count, cand_action, xchg + x.cpolicy() - ga, xchg + x.clogit() - ga, cand_player, sc + 3 - g, sc + 4 - g, g, lane);
    waveSync();
    MZ_LPROF(9);
    expandBackupBody(pv, cand_count, cand_action, xchg + x.cpolicy() - ga, xchg + x.clogit() - ga, cand_player, sc + 3 - g, sc + 4 - g, slot, a->err, g,
                     lane, tiles, part);
    MZ_LPROF(12);
}

template <int WPE>
__device__ __noinline__ void simCandExpand(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, float* tiles, float* xchg, int part)
{
    simCandExpandImpl<WPE>(a, rot, slot, g, lane, tiles, xchg, part);
}

// ---- The value-first order (the instance with tail help and the split Go leaf; no Gumbel, no value rescaling; MZ_NO_SPEC=64: off) ----
// Behind the heads the next walk only needs the backup, and the backup only needs the value: wave 0 backs up at once and walks simulation s + 1, waves 1 .. 3 run
// their helper segments behind the backup, and waves 4 .. 7 — which have no part in the walk — run candidates + expand of simulation s beside it (wave 4 in wave
// 0's role, the rank sort on the four of them).  The waves meet through LDS words that carry the simulation's serial number s + 1: monotonic, never reset inside a
// launch, written behind a workgroup-scope release fence and read in front of an acquire fence (as waveSync() does), s_sleep between two polls, every poll loop
// bounded (error flag 97).  All eight waves of the workgroup are resident, so no wave waits for one that is not running.
constexpr int kVfBackup = 4;  // serial of the last backup that is done (wave 0 -> the helper segments of waves 1 .. 3)
constexpr int kVfLeaf = 5;    // the leaf of the simulation the candidate pipeline works on, handed over before the next walk overwrites the path block; [6] = 1
constexpr int kVfGather = 7;  // serial of the last gather that is done (wave 4 -> waves 5 .. 7)
constexpr int kVfRank = 8;    // rank parts of waves 5 .. 7 done so far: 3 per simulation
constexpr int kVfExpand = 9;  // serial of the last expand that is done (wave 4 -> wave 0: the joins)
constexpr int kVfStats = 10;  // (MZ_SIM_PROF) walks that arrived at the previous leaf, those that waited there, their ticks, waits at the join in front of the leaf
// lending (sim_help.h; wave 7 in front of the barrier behind the leaf -> every wave behind it)
constexpr int kVfWalked = 14;   // serial of the last walk that is done (wave 0 -> wave 7: the leaf is about to start, the game's offer has to be closed)
constexpr int kVfOffer = 15;    // this simulation's offer was taken by a volunteer
constexpr int kVfLend = 16;     // 0, or 1 + the game whose offer this workgroup has taken, and [17] the sequence number of that offer
constexpr int kVfLendStat = 18; // (MZ_SIM_PROF) offers taken, offers that were gone when the swap arrived, offers withdrawn behind a terminal leaf, ticks waited for the command
constexpr int kVfLendBits = 24; // the planes of the command of a lent tower (3 * kHpMaxUnits words)
constexpr int kVfWords = kVfLendBits + 3 * kHpMaxUnits;
constexpr int kVfErr = 97;

__device__ __forceinline__ bool vfWait(LdsI32* w, int want, int* err, int lane)
{
    int seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    const bool waited = seen < want;
    for (int i = 0; i < kHpPollLimit && seen < want; ++i) {
        __builtin_amdgcn_s_sleep(1);
        seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    if (seen < want && lane == 0) { atomicExch(err, kVfErr); }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return waited;
}
// (every store of the wave so far is visible to the workgroup before the word is)
__device__ __forceinline__ void vfPublish(LdsI32* w, int serial, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { __hip_atomic_store(w, serial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
}

// the walk alone (wave 0; the backup of the simulation before it is done): `join_leaf` >= 0 = the leaf of that simulation, whose expand may still be running
template <class RcpPtr>
__device__ __noinline__ void simWalkVf(CSimArgs* __restrict__ a, int g, int lane, RcpPtr rcp, SpecMem spec, float* xchg, int serial, int join_leaf, int join_want, int* vf_)
{
    serial = __builtin_amdgcn_readfirstlane(serial);
    g = __builtin_amdgcn_readfirstlane(g);
    join_leaf = __builtin_amdgcn_readfirstlane(join_leaf);
    join_want = __builtin_amdgcn_readfirstlane(join_want);
    LdsI32* vf = (LdsI32*)vf_;
    unsigned long long t0 = 0;
    if (a->prof) { t0 = wall_clock64(); }
    const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
    selectBody<true, true>(pv, nullptr, g, lane, rcp, spec, serial, SelectJoin{vf + kVfExpand, vf + kVfStats, join_want, join_leaf, kHpPollLimit, kVfErr, a->err});
    waveSync();
    if (a->prof && lane == 0) {
        a->prof[size_t(g) * 8 + 5] += wall_clock64() - t0;
        a->prof[size_t(g) * 8 + 6] += pv.path_len[g];
    }
}

// the leaf's first half (wave 0, behind the join with the expand of the simulation before), and the hand-over of the leaf node to the candidate pipeline
template <int CPL>
__device__ __noinline__ void simLeafVf(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, float* xchg, const uint64_t* seen_lds, uint64_t* leaf_smem, int* vf)
{
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    rot = __builtin_amdgcn_readfirstlane(rot);
    if constexpr (CPL > 0) {
        const PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
        const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
        if (lane == 0) {
            const int len = pv.path_len[g];
            vf[kVfLeaf] = len > 0 ? (pv.path + size_t(g) * pv.max_depth)[len - 1] : 0;
            vf[kVfLeaf + 1] = len > 0 ? 1 : 0;
        }
        leafBody<CPL, true, 1>(gv, pv, rot, slot, g, lane, leaf_smem, seen_lds);
    }
}

// candidates + expand of simulation `serial - 1` on waves 4 .. 7 (w = wave - 4), beside wave 0's backup and next walk
template <int WPE>
__device__ __noinline__ void simCandPipeVf(CSimArgs* __restrict__ a, int rot, int slot, int g, int lane, int w, int serial, float* tiles, float* xchg, int* vf_)
{
    g = __builtin_amdgcn_readfirstlane(g);
    w = __builtin_amdgcn_readfirstlane(w);
    serial = __builtin_amdgcn_readfirstlane(serial);
    LdsI32* vf = (LdsI32*)vf_;
    const int A = a->gv.A;
    const SimXchg x{A + (A & 1)};
    if (w == 0) {
        simCandGatherImpl<WPE>(a, rot, g, lane, tiles, xchg);
        vfPublish(vf + kVfGather, serial, lane);
    } else {
        vfWait(vf + kVfGather, serial, a->err, lane);
    }
    const int k = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(xchg + x.scalars())[1]);
    float* dense = simCandDense(tiles, A);
    if (k > 0 && k <= kCandCoopMax && a->cand_coop) { // two of the eight shares per wave (otherwise wave 4 has sorted alone in the gather)
        candRankPart(dense, k, w, 8, lane, reinterpret_cast<int*>(dense + kCandCoopMax));
        candRankPart(dense, k, w + 4, 8, lane, reinterpret_cast<int*>(dense + kCandCoopMax));
    }
    if (w != 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) { __hip_atomic_fetch_add(vf + kVfRank, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
        return;
    }
    vfWait(vf + kVfRank, 3 * serial, a->err, lane);
    // scatter, the sorted candidates where the expand reads them, the expand (simCandExpandImpl's steps; the path of the expand is the one node of kVfLeaf)
    slot = __builtin_amdgcn_readfirstlane(slot);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    PoolView pv = simPathView(ldc(&a->pv), reinterpret_cast<int*>(xchg) - 2 * a->pv.max_depth - 2, g);
    pv.path = vf_ + kVfLeaf - size_t(g) * pv.max_depth;
    pv.path_len = vf_ + kVfLeaf + 1 - g;
    const size_t ga = size_t(g) * gv.A;
    float* sc = xchg + x.scalars();
    int* cand_count = reinterpret_cast<int*>(sc + 1) - g;
    int* cand_player = reinterpret_cast<int*>(sc + 2) - g;
    int* cand_action = reinterpret_cast<int*>(xchg + x.caction()) - ga;
    Cand* cs = reinterpret_cast<Cand*>(tiles);
    Cand* out = cs + gv.A;
    if (k > 0 && k <= kCandCoopMax && a->cand_coop) { candScatter(cs, out, reinterpret_cast<int*>(out + gv.A), k, 8, lane, reinterpret_cast<const int*>(dense + kCandCoopMax), a->err); }
    azCandStore(gv, sc - g, out, k, cand_count, cand_action, xchg + x.cpolicy() - ga, xchg + x.clogit() - ga, cand_player, sc + 3 - g, sc + 4 - g, g, lane);
    waveSync();
    expandBackupBody(pv, cand_count, cand_action, xchg + x.cpolicy() - ga, xchg + x.clogit() - ga, cand_player, sc + 3 - g, sc + 4 - g, slot, a->err, g, lane, tiles, 1);
    vfPublish(vf + kVfExpand, serial, lane);
}

// Root exploration noise (ref zero_actor.cpp:194-213): policy = (1 - eps) * policy + eps * noise for the root's children, in storage
// order; the noise values were drawn on the host in the reference's RNG order (their count only depends on the number of legal moves)
template <int WPE>
__device__ __noinline__ void simApplyRootNoise(CSimArgs* __restrict__ a, int g, int lane)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    const PoolView v = ldc(&a->pv);
    const size_t base = size_t(g) * v.cap;
    const int nc = v.rec[base].num_children;
    const size_t fc = base + v.rec[base].first_child;
    const float eps = a->noise_eps;
    for (int i = lane; i < nc; i += 64) {
        const float nz = a->root_noise[size_t(g) * v.A + i];
        if (a->noise_kind == kNoiseDirichlet) { v.rec[fc + i].policy = (1 - eps) * v.rec[fc + i].policy + eps * nz; }
        else { v.logit[fc + i] = v.logit[fc + i] + nz; }
        v.noise[fc + i] = nz;
    }
    waveSync();
}

// Gumbel: sequential halving + the root child the next simulation starts from (slot >= 1); the first simulation of a launch takes the
// start node the host computed when it ran this step itself (it does at every launch boundary, reading the state back first)
// state_lds: the game's Gumbel state lives in LDS for the launch (sim_kernel_mz) instead of the pool's array
template <int WPE>
__device__ __noinline__ void simGumbelStart(CSimArgs* __restrict__ a, int slot, bool host_start, int g, int lane, float* tiles, int* state_lds = nullptr)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    slot = __builtin_amdgcn_readfirstlane(slot);
    if (host_start && slot >= 1) { return; } // a->start[g] was uploaded by the host
    int st = 0;
    if (slot >= 1 && !host_start) {
        const PoolView pv = ldc(&a->pv);
        GumbelView gum = ldc(&a->gum);
        if (state_lds) { gum.state = state_lds - size_t(g) * (3 + kGumbelMaxSample); }
        st = gumbelStepBody(pv, gum, slot, g, lane, tiles);
    }
    if (lane == 0) { a->start[g] = st; }
    waveSync();
}

// the heads read the tower's last activations where they are (an LDS tile); tile 0 (the blocks' temporary) is free for their scratch
template <int WPE, bool BIGA = false, bool FP = BIGA>
__device__ __forceinline__ void simHeadsImpl(CSimArgs* __restrict__ a, int g, int tid, float* tiles, const float* xtile, int xcs, int xpw, float* xchg)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
    xcs = __builtin_amdgcn_readfirstlane(xcs);
    xpw = __builtin_amdgcn_readfirstlane(xpw);
    MZ_HPROF(0);
    const HeadParams hp = ldc(&a->hp);
    const SimXchg x{hp.A + (hp.A & 1)};
    const size_t ga = size_t(g) * hp.A;
    headsBody<BIGA, FP>(nullptr, hp, xchg + x.policy() - ga, xchg + x.logit() - ga, xchg + x.scalars() - g, nullptr, nullptr, 0, g, tid, 512, tiles, xtile, xcs, xpw);
    MZ_HPROF(1);
}
// a non-inlined device function saves the callee-saved VGPRs it uses on entry (scratch stores + loads by all 8 waves): worth it for the
// 9x9 kernels (the heads keep their own register budget, and their version needs none saved), not for the 128-VGPR 8x8 / 3x3 kernels
template <int WPE, bool BIGA = false, bool FP = BIGA>
__device__ __noinline__ void simHeads(CSimArgs* __restrict__ a, int g, int tid, float* tiles, const float* xtile, int xcs, int xpw, float* xchg)
{
    simHeadsImpl<WPE, BIGA, FP>(a, g, tid, tiles, xtile, xcs, xpw, xchg);
}

// sim_kernel<9,9,20,64,2> only: the heads with their operands delivered ahead (net_body.h headsBodyAhead); `hw` is the launch's LDS block of small weights.
// Inlined into the kernel, unlike simHeads: as a function of its own it saved 15 callee-saved VGPRs per wave and call, and it reads the argument block with scalar
// loads this way; the kernel keeps its 248 VGPRs.  The outputs go to the hand-over block through LDS pointers of game 0's indexing.
template <int H, int W>
__device__ __forceinline__ void simHeadsAhead(CSimArgs* __restrict__ a, int tid, float* tiles, const float* xtile, float* xchg, const float* hw)
{
    MZ_HPROF(0);
    const HeadParams hp = ldc(&a->hp);
    const SimXchg x{HeadsAhead::A + (HeadsAhead::A & 1)};
    headsBodyAhead<planeStride(H, W), W + 2>(hp, xchg + x.policy(), xchg + x.logit(), xchg + x.scalars(), tid, tiles, xtile, hw);
    MZ_HPROF(1);
}

// The terminal flag of the simulation's leaf: wave 0 wrote it into the hand-over block before the first barrier of the simulation (the leaf's first half), every
// wave reads it behind that barrier.  Scalar, so that the branch on it is one s_cbranch.  MZ_NO_SPEC=16: the network runs at terminal leaves too (A/B, tests).
__device__ __forceinline__ bool simLeafTerminal(CSimArgs* __restrict__ a, const float* xchg)
{
    if (a->no_spec & 16) { return false; }
    const int A = a->gv.A;
    const SimXchg x{A + (A & 1)};
    return __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(xchg + x.scalars())[6]) != 0;
}

// MZ_SIM_PROF: the words behind the per-game counters (kSimProfTail of them).  [0..3] belong to the launch that is running — earliest start, first and last exit
// of a game (100-MHz ticks from [4], the stamp of the previous fold), sum of the exits; sim_prof_fold (sim.hip) adds them to [8..] between two launches.
constexpr int kSimProfTail = 40; // ([7]: simulations that ran the heads with their operands ahead (simHeadsAhead), a running sum; [16..20]: the value-first order: simulations, walks that arrived at the previous leaf, waits there, their ticks, waits in front of the leaf;
                                 //  tail help: [21] simulations that ran a quad tower, [22] their tower ticks, [23] games whose pair became a quad; why a finished CU stopped looking
                                 //  for a game to help — cause 0: every running game of its XCD with enough simulations left had its helpers, 1: no game of its XCD was running,
                                 //  2: only games with fewer than help_min_left simulations were left — [24 + cause] CUs and [27 + cause] the sum of the ticks at which they
                                 //  stopped, of the running launch; [30 + cause] ticks per CU from there to the last game's exit, summed over the launches by sim_prof_fold;
                                 //  lending: [33] simulations whose tower a volunteer shared, [34] their tower ticks, [35] offers taken, [36] swaps for an offer that came too late,
                                 //  [37] offers withdrawn behind a terminal leaf, [38] ticks the volunteers waited for their commands, [39] ticks they were away from their own games)
__device__ __forceinline__ void simProfEnter(unsigned long long* tail)
{
    atomicMin(tail + 0, wall_clock64() - tail[4]);
}
__device__ __forceinline__ void simProfExit(unsigned long long* tail)
{
    const unsigned long long t = wall_clock64() - tail[4];
    atomicMin(tail + 1, t);
    atomicMax(tail + 2, t);
    atomicAdd(tail + 3, t);
    atomicAdd(tail + 5, 1ull);
}
// One simulation into the game's counters: [0] select + leaf, [1] tower, [2] heads, [3] cand + expand ticks, [4] simulations | (<< 32) those whose network
// evaluation was skipped.  term: a terminal leaf — its second half, alone where the heads would be, counts as leaf time: "tower" and "heads" only hold
// simulations that ran them
__device__ __forceinline__ void simProfSim(unsigned long long* prof, unsigned long long t0, unsigned long long t1, unsigned long long t2, unsigned long long t3, unsigned long long t4,
                                           bool term = false)
{
    prof[0] += t1 - t0 + (term ? t3 - t1 : 0); prof[1] += term ? 0 : t2 - t1; prof[2] += term ? 0 : t3 - t2; prof[3] += t4 - t3;
    prof[4] += 1 + (static_cast<unsigned long long>(term) << 32);
}
// The end of a launch: the walk's speculation counters (pool_body.h) into [7] = passes << 40 | levels taken << 20 | walks that found their path, and
// [6] += levels taken over from the helper waves << 40 (the low bits hold the path lengths)
__device__ __forceinline__ void simProfSpec(unsigned long long* prof, const int* spec_w)
{
    prof[7] += (static_cast<unsigned long long>(spec_w[kSpecPasses]) << 40) | (static_cast<unsigned long long>(spec_w[kSpecLevels]) << 20) | spec_w[kSpecFound];
    prof[6] += static_cast<unsigned long long>(spec_w[kSpecHelped]) << 40;
}

// 8x8 boards: three tower tiles are 80 KB of LDS, so TWO games share a CU (16 waves) if the kernel stays within 128 VGPRs: one game's
// tree phases and barrier bubbles are filled by the other's tower
// waves per SIMD the kernel is compiled for: 4 (= two resident workgroups per CU, 128 VGPRs) for boards up to 64 points, whose tower
// fits that register budget; 9x9 Go keeps 2 (its 6 pixel tiles per wave pair need ~166 VGPRs, and BASELINE's 256 games are one per CU)
template <int H, int W, int CIN0_PAD, int CPAD, bool BF = false>
constexpr int simWavesPerEu() { return (!BF && H * W <= 64 && kTowerTiles * (CIN0_PAD > CPAD ? CIN0_PAD : CPAD) * planeStride(H, W) * 4 <= 76 * 1024) ? 4 : 2; }
// floats of the LDS region the tower works in (the tree phases and the heads take their scratch from its start)
template <int H, int W, int CIN0_PAD, int CPAD, bool BF>
constexpr int simTileFloats() { return BF ? towerBf16LdsBytes<H, W>(true) / 4 : kTowerTiles * (CIN0_PAD > CPAD ? CIN0_PAD : CPAD) * planeStride(H, W); }

template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __noinline__ const float* simTower(CSimArgs* __restrict__ a, int g, int tid, float* tiles, float* xchg)
{
    // arguments of a device function arrive in VGPRs: tell the compiler which ones are wave-uniform
    g = __builtin_amdgcn_readfirstlane(g);
#ifdef MZ_SIM_TPROF
    if (tid == 0 && g == 0) { s_tp_prev = clock64(); s_tp_idx = 0; g_tp[63] += 1; }
#endif
    g = __builtin_amdgcn_readfirstlane(g);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    return towerBody<H, W, CIN0_PAD, CPAD>(reinterpret_cast<const float*>(gv.feat), a->params, *(const TowerArgs*)&a->ta, nullptr, g, tid, tiles);
}

// the opt-in bf16x3 tower inside the simulation kernel: same hand-over (bit-packed planes in, f32 padded planes out) as simTower
template <int H, int W>
__device__ __noinline__ const float* simTowerBf16(CSimArgs* __restrict__ a, int g, int tid, float* tiles, float* xchg)
{
    g = __builtin_amdgcn_readfirstlane(g);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    return towerBodyBf16<H, W>(reinterpret_cast<const unsigned*>(gv.feat), a->wfrag, a->params, *(const TowerArgsBf16*)&a->tb, nullptr, g, tid,
                               reinterpret_cast<char*>(tiles));
}

// Tail help (sim_help.h), owner side: the simulation's tower with the game's helper(s).  Wave 0 first sends the leaf's bit-packed planes — the command: 16-byte
// stores of three words + the command word (sequence number of the simulation, mode, start of the exchange count) each — then the workgroup runs member 0 of the pair
// or quad tower.  Functions of their own beside simTower, so that the solo path keeps its register budget and code.  nullptr: a helper went missing (the error flag
// is raised, the workgroup leaves the kernel).
template <int H, int W, int CIN0_PAD, int CPAD, int MODE>
__device__ __forceinline__ const float* simTowerHelped(CSimArgs* __restrict__ a, int g, int tid, float* tiles, float* xchg, int seq, unsigned xseq, int* abort_lds, bool lent = false)
{
    g = __builtin_amdgcn_readfirstlane(g);
    seq = __builtin_amdgcn_readfirstlane(seq);
    xseq = __builtin_amdgcn_readfirstlane(xseq);
    const GoDevView gv = simLeafView(ldc(&a->gv), xchg, g);
    const unsigned* bits = reinterpret_cast<const unsigned*>(gv.feat) + size_t(g) * gv.channels * gv.W32; // (the view's pointers are moved back by the game's offset)
    unsigned* hb = a->help + size_t(g) * a->help_words;
    const int fw = gv.channels * gv.W32;
    if (tid < helpCmdUnits(fw)) {
        hpu4 u;
        u.x = bits[3 * tid];
        u.y = 3 * tid + 1 < fw ? bits[3 * tid + 1] : 0u;
        u.z = 3 * tid + 2 < fw ? bits[3 * tid + 2] : 0u;
        u.w = hpCmdWord(unsigned(seq), MODE, xseq, lent);
        asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(hb + kHpCmd + 4 * tid), "v"(u) : "memory");
    }
    HelpCtx c{hb, 0, xseq, abort_lds, a->err, tiles + a->pair_slot};
    if constexpr (MODE == kHpModeQuad) { return towerBodyQuad<H, W, CIN0_PAD, CPAD>(bits, a->params, *(const TowerArgs*)&a->ta, tid, tiles, c); }
    else { return towerBodyPair<H, W, CIN0_PAD, CPAD>(bits, a->params, *(const TowerArgs*)&a->ta, tid, tiles, c); }
}
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __noinline__ const float* simTowerPair(CSimArgs* __restrict__ a, int g, int tid, float* tiles, float* xchg, int seq, unsigned xseq, int* abort_lds, int lent)
{
    // (lent: member 1 is the volunteer that took this simulation's offer, not the holder of slot 1)
    return simTowerHelped<H, W, CIN0_PAD, CPAD, kHpModePair>(a, g, tid, tiles, xchg, seq, xseq, abort_lds, __builtin_amdgcn_readfirstlane(lent) != 0);
}
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __noinline__ const float* simTowerQuad(CSimArgs* __restrict__ a, int g, int tid, float* tiles, float* xchg, int seq, unsigned xseq, int* abort_lds)
{
    return simTowerHelped<H, W, CIN0_PAD, CPAD, kHpModeQuad>(a, g, tid, tiles, xchg, seq, xseq, abort_lds);
}

// Tail help, owner side: the tower of this simulation by the game's helper slots (one thread of a wave that has no part in the walk).  Slots 2 and 3 are only
// claimed in a game whose slot 1 is, and only looked at then: a game without a helper pays one load, as before.
__device__ __forceinline__ int simHelpMode(const unsigned* help_blk)
{
    if (hpLoadU(help_blk + kHpHelper) == 0u) { return 0; }
    const unsigned h2 = hpLoadU(help_blk + kHpHelper2), h3 = hpLoadU(help_blk + kHpHelper3);
    return (h2 != 0u && h3 != 0u) ? 2 : 1;
}

// Tail help, helper side: one tower of game `o` as its member `member`.  Pair and quad are functions of their own, each with its own register budget, like the
// owner's (inlined side by side into simHelpTail they spilled into its layer loops).  false: a member went missing.
template <int H, int W, int CIN0_PAD, int CPAD, int MODE>
__device__ __noinline__ bool simHelpTower(CSimArgs* __restrict__ a, int o, int member, unsigned xseq, int tid, float* tiles, const unsigned* bits, int* abort_lds)
{
    o = __builtin_amdgcn_readfirstlane(o);
    member = __builtin_amdgcn_readfirstlane(member);
    xseq = __builtin_amdgcn_readfirstlane(xseq);
    HelpCtx c{a->help + size_t(o) * a->help_words, member, xseq, abort_lds, a->err, tiles + a->pair_slot};
    if constexpr (MODE == kHpModeQuad) { return towerBodyQuad<H, W, CIN0_PAD, CPAD>(bits, a->params, *(const TowerArgs*)&a->ta, tid, tiles, c) != nullptr; }
    else { return towerBodyPair<H, W, CIN0_PAD, CPAD>(bits, a->params, *(const TowerArgs*)&a->ta, tid, tiles, c) != nullptr; }
}

// Lending (sim_help.h), wave 7 in front of the barrier behind the leaf of simulation s, beside wave 0's walk.  A game without a helper in slot 1 opens the offer
// of this simulation and closes it by compare-and-swap once the walk is done (kVfWalked: the swap's round trip lies beside the leaf's first half); a swap that fails
// means a volunteer has taken the offer, and this simulation's tower is a pair tower with it.  Meanwhile the wave looks through the offers of its XCD's games, as
// simHelpTail looks through their slots: the least-progress open offer of a game that trails this one by at least `lend_lead` simulations and has at least
// help_min_left of them left.  Before it takes one it closes its own — a workgroup whose offer is open or taken never waits for anybody — and once it has taken one
// it looks no further: one tower per simulation.  Results: s_help[1] the tower's mode by the slots (simHelpMode), [kVfOffer], [kVfLend], [kVfLend + 1].
__device__ __noinline__ void simLendScan(CSimArgs* __restrict__ a, int g, int lane, int s, int nsims, unsigned* help_blk, int* s_help)
{
    g = __builtin_amdgcn_readfirstlane(g);
    s = __builtin_amdgcn_readfirstlane(s);
    nsims = __builtin_amdgcn_readfirstlane(nsims);
    LdsI32* vf = (LdsI32*)s_help;
    const unsigned seq = unsigned(s) + 1u;
    const int mode = __builtin_amdgcn_readfirstlane(simHelpMode(help_blk));
    int taken = 0, lend = 0, lend_seq = 0, late = 0;
    if (mode == 0) {
        if (lane == 0) { hpStoreU(help_blk + kHpOffer, seq); }
        const int games = gridDim.x, words = a->help_words, min_left = a->help_min_left, lead = a->lend_lead;
        const unsigned myxcc = hpXccId();
        bool open = true, walked = false;
        for (int i = 0; i < kHpPollLimit; ++i) {
            walked = __builtin_amdgcn_readfirstlane(__hip_atomic_load(vf + kVfWalked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) > s;
            // (sequence number of the offer << 10) | game: the host only lets a launch help with at most kHpMaxGames games (sim.hip simLaunch), a launch has far fewer
            // than 2^22 simulations, and the games of an XCD (every eighth) are one pass of the loop up to 512 of them, as in simHelpTail
            static_assert(kHpMaxGames == 1 << 10, "the search key keeps the game in its 10 low bits");
            unsigned key = ~0u;
            if (!walked && !taken && !lend && int(seq) > lead) {
                for (int o = (g & 7) + 8 * lane; o < games; o += 8 * 64) {
                    const unsigned* ob = a->help + size_t(o) * words;
                    const unsigned x = hpLoadU(ob + kHpXcc), q = hpLoadU(ob + kHpOffer);
                    const bool ok = o != g && x == myxcc && q != 0u && q < kHpOfferClaimed && int(q) - 1 + min_left <= nsims && int(q) + lead <= int(seq);
                    const unsigned k = (q << 10) | unsigned(o);
                    if (ok && k < key) { key = k; }
                }
                for (int o = 32; o > 0; o >>= 1) { const unsigned k2 = __shfl_xor(key, o); key = k2 < key ? k2 : key; }
            }
            if (open && (walked || key != ~0u)) { // the own offer: closed for good, or taken
                unsigned expected = seq;
                if (lane == 0) { taken = __hip_atomic_compare_exchange_strong(help_blk + kHpOffer, &expected, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1; }
                taken = __builtin_amdgcn_readfirstlane(taken);
                open = false;
            }
            if (key != ~0u && !taken) {
                const unsigned q = key >> 10;
                unsigned expected = q;
                int got = 0;
                if (lane == 0) {
                    got = __hip_atomic_compare_exchange_strong(a->help + size_t(key & unsigned(kHpMaxGames - 1)) * words + kHpOffer, &expected, q | kHpOfferClaimed, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT) ? 1 : 0;
                }
                got = __builtin_amdgcn_readfirstlane(got);
                if (got) { lend = int(key & unsigned(kHpMaxGames - 1)) + 1; lend_seq = int(q); }
                else { late += 1; }
            }
            if (!open && (walked || taken || lend)) { break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (open) { // the walk never ended within the poll limit: the error flag is raised, and the offer is closed like any other, so that no volunteer is left with it
            unsigned expected = seq;
            if (lane == 0) {
                atomicExch(a->err, kVfErr);
                taken = __hip_atomic_compare_exchange_strong(help_blk + kHpOffer, &expected, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0 : 1;
            }
            taken = __builtin_amdgcn_readfirstlane(taken);
        }
    }
    if (lane == 0) {
        s_help[1] = mode;
        s_help[kVfOffer] = taken;
        s_help[kVfLend] = lend;
        s_help[kVfLend + 1] = lend_seq;
        if (a->prof) { s_help[kVfLendStat] += lend ? 1 : 0; s_help[kVfLendStat + 1] += late; }
    }
}

// Lending, the volunteer behind that barrier: its own walk and leaf are done, the tiles are free, every wave is here.  Wave 0 waits for the command of the offer
// the workgroup has taken — the owner is resident and in front of its tower: it sends the command behind its own leaf and planes — or for the offer's withdrawal
// (the owner's leaf was terminal: no tower), takes the planes into the staging words of s_help, and the workgroup runs that one tower as member 1 of the pair.
// false: the owner went missing (the error flag is raised, the workgroup leaves the kernel).
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __noinline__ bool simLendTower(CSimArgs* __restrict__ a, int o, int seq, int tid, float* tiles, int* s_help)
{
    o = __builtin_amdgcn_readfirstlane(o);
    seq = __builtin_amdgcn_readfirstlane(seq);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fw = a->gv.channels * a->gv.W32, units = helpCmdUnits(fw);
    const unsigned* ob = a->help + size_t(o) * a->help_words;
    unsigned* bits = reinterpret_cast<unsigned*>(s_help + kVfLendBits);
    if (wave == 0) {
        const unsigned long long tw0 = a->prof ? wall_clock64() : 0;
        int st = 0;
        hpu4 u;
        for (int i = 0; i < kHpPollLimit && st == 0; ++i) {
            const unsigned* src = ob + kHpCmd + 4 * (lane < units ? lane : 0);
            asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(u) : "v"(src) : "memory");
            const unsigned cw = __builtin_amdgcn_readfirstlane(u.w);
            if (__all(u.w == cw) && hpCmdSeq(cw) == unsigned(seq) && hpCmdLent(cw) && hpCmdMode(cw) == kHpModePair) { st = 1; }
            else if (hpLoadU(ob + kHpOffer) != (unsigned(seq) | kHpOfferClaimed)) { st = 2; } // withdrawn (behind a tower the word changes only after this member's last exchange)
            else { __builtin_amdgcn_s_sleep(4); }
        }
        if (st == 1 && lane < units) {
            bits[3 * lane] = u.x;
            if (3 * lane + 1 < fw) { bits[3 * lane + 1] = u.y; }
            if (3 * lane + 2 < fw) { bits[3 * lane + 2] = u.z; }
        }
        if (lane == 0) {
            if (st == 0) { atomicExch(a->err, kHpErrLend); }
            s_help[3] = st;
            s_help[2] = int(hpCmdXseq(__builtin_amdgcn_readfirstlane(u.w)));
            if (a->prof) { s_help[kVfLendStat + 2] += st == 2 ? 1 : 0; s_help[kVfLendStat + 3] += int(wall_clock64() - tw0); }
        }
    }
    __syncthreads();
    const int st = __builtin_amdgcn_readfirstlane(s_help[3]);
    const unsigned xseq = unsigned(__builtin_amdgcn_readfirstlane(s_help[2]));
    if (st == 0) { return false; }
    if (st == 1 && !simHelpTower<H, W, CIN0_PAD, CPAD, kHpModePair>(a, o, 1, xseq, tid, tiles, bits, s_help)) { return false; }
    __syncthreads();
    return true;
}

// Tail help, helper side: the workgroup of game g has finished its simulations of this launch and written its results.  It looks among the games of its XCD
// (workgroups are dealt to the XCDs round-robin, so those are the games congruent to g mod 8; the XCC_ID every owner publishes is compared anyway) for the one
// with the least progress that has no helper and at least help_min_left simulations left, and claims its slot 1; if there is none, for the helped game with the
// least progress that has a free slot 2 or 3 (MZ_NO_SPEC=128: slot 1 only, one helper per game).  It computes its member's share of that game's pair or quad towers,
// as the commands say, until that game is done; then it looks again, and leaves when there is nothing to claim.  `bits`: LDS for the planes of a command.
// MZ_SIM_PROF: tail words [6] ticks spent as a helper in this launch, [15] games helped, [24 ..] why it left (kSimProfTail).
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __noinline__ void simHelpTail(CSimArgs* __restrict__ a, int g, int tid, float* tiles, unsigned* bits, int nsims, int* s_help)
{
    g = __builtin_amdgcn_readfirstlane(g);
    nsims = __builtin_amdgcn_readfirstlane(nsims);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int games = gridDim.x, words = a->help_words, min_left = a->help_min_left;
    const int fw = a->gv.channels * a->gv.W32, units = helpCmdUnits(fw);
    const bool more_slots = !(a->no_spec & 128);
    const unsigned myxcc = hpXccId();
    unsigned long long* ptail = a->prof ? a->prof + size_t(games) * 8 : nullptr;
    for (int round = 0; round < 64; ++round) { // (bounded: a round either claims a game, loses the claim to another helper, or ends the search)
        if (wave == 0) {
            unsigned key = ~0u, key2 = ~0u; // (progress << 10) | game: the least progress wins; key2: among the helped games with a free slot
            bool enough = false, running = false;
            for (int o = (g & 7) + 8 * lane; o < games; o += 8 * 64) {
                const unsigned* ob = a->help + size_t(o) * words;
                const unsigned x = hpLoadU(ob + kHpXcc), p = hpLoadU(ob + kHpProgress), h = hpLoadU(ob + kHpHelper);
                const unsigned h2 = hpLoadU(ob + kHpHelper2), h3 = hpLoadU(ob + kHpHelper3);
                const unsigned k = (p << 10) | unsigned(o);
                const bool mine = o != g && x == myxcc, left = int(p) + min_left <= nsims;
                running = running || (mine && int(p) < nsims);
                enough = enough || (mine && left);
                if (mine && left && h == 0u && k < key) { key = k; }
                if (mine && left && more_slots && h != 0u && (h2 == 0u || h3 == 0u) && k < key2) { key2 = k; }
            }
            for (int o = 32; o > 0; o >>= 1) { const unsigned k2 = __shfl_xor(key, o); key = k2 < key ? k2 : key; }
            for (int o = 32; o > 0; o >>= 1) { const unsigned k2 = __shfl_xor(key2, o); key2 = k2 < key2 ? k2 : key2; }
            enough = __any(enough);
            running = __any(running);
            if (lane == 0) {
                int cl = 0, slot = 1;
                if (key != ~0u) {
                    unsigned expected = 0u;
                    unsigned* hw = a->help + size_t(key & 1023u) * words + kHpHelper;
                    cl = __hip_atomic_compare_exchange_strong(hw, &expected, unsigned(g) + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? int(key & 1023u) + 1 : -1;
                } else if (key2 != ~0u) {
                    key = key2;
                    unsigned* hw = a->help + size_t(key & 1023u) * words;
                    cl = -1;
                    for (slot = 2; slot <= 3 && cl < 0; ++slot) {
                        unsigned expected = 0u;
                        if (__hip_atomic_compare_exchange_strong(hw + (slot == 2 ? kHpHelper2 : kHpHelper3), &expected, unsigned(g) + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT)) { cl = int(key & 1023u) + 1; break; }
                    }
                }
                s_help[1] = cl;
                // the owner's progress when it was chosen: every command for this helper has a higher sequence number.  Nothing to claim: why (kSimProfTail)
                s_help[2] = cl != 0 ? int(key >> 10) : (enough ? 0 : running ? 2 : 1);
                s_help[3] = slot;
            }
        }
        __syncthreads();
        const int cl = __builtin_amdgcn_readfirstlane(s_help[1]);
        unsigned last = unsigned(__builtin_amdgcn_readfirstlane(s_help[2]));
        const int slot = __builtin_amdgcn_readfirstlane(s_help[3]);
        __syncthreads();
        if (cl == 0) {
            if (ptail && tid == 0) { atomicAdd(ptail + 24 + last, 1ull); atomicAdd(ptail + 27 + last, wall_clock64() - ptail[4]); }
            return;
        }
        if (cl < 0) { continue; }
        const unsigned long long th0 = ptail ? wall_clock64() : 0;
        unsigned* ob = a->help + size_t(cl - 1) * words;
        for (;;) {
            if (wave == 0) { // the next command, or the end of the owner's launch
                int st = 0;
                hpu4 u;
                for (int i = 0; i < kHpPollLimit && st == 0; ++i) {
                    const unsigned* src = ob + kHpCmd + 4 * (lane < units ? lane : 0);
                    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(u) : "v"(src) : "memory");
                    const unsigned cw = __builtin_amdgcn_readfirstlane(u.w), sq = hpCmdSeq(cw);
                    if (__all(u.w == cw) && sq > last && sq <= unsigned(nsims)) {
                        last = sq;
                        // (the holder of slot 2 or 3 has no part in a pair tower: it waits for the command after it)
                        // ... and no holder of a slot has a part in a tower lent to a volunteer (a claim of slot 1 beside a taken offer)
                        if (!hpCmdLent(cw) && (slot == 1 || hpCmdMode(cw) == kHpModeQuad)) { st = 1 + hpCmdMode(cw); s_help[2] = int(hpCmdXseq(cw)); }
                    }
                    else if (hpLoadU(ob + kHpProgress) >= unsigned(nsims)) { st = 3; }
                    else { __builtin_amdgcn_s_sleep(4); }
                }
                if ((st == 1 || st == 2) && lane < units) {
                    bits[3 * lane] = u.x;
                    if (3 * lane + 1 < fw) { bits[3 * lane + 1] = u.y; }
                    if (3 * lane + 2 < fw) { bits[3 * lane + 2] = u.z; }
                }
                if (lane == 0) {
                    if (st == 0) { atomicExch(a->err, slot == 1 ? 96 : kHpErrQuadCmd); }
                    s_help[1] = st;
                }
            }
            __syncthreads();
            const int st = __builtin_amdgcn_readfirstlane(s_help[1]);
            if (st != 1 && st != 2) {
                if (ptail && tid == 0) { atomicAdd(ptail + 6, wall_clock64() - th0); atomicAdd(ptail + 15, 1ull); }
                if (st == 0) { return; }
                break;
            }
            const unsigned xseq = unsigned(__builtin_amdgcn_readfirstlane(s_help[2]));
            if (!(st == 2 ? simHelpTower<H, W, CIN0_PAD, CPAD, kHpModeQuad>(a, cl - 1, slot, xseq, tid, tiles, bits, s_help)
                          : simHelpTower<H, W, CIN0_PAD, CPAD, kHpModePair>(a, cl - 1, 1, xseq, tid, tiles, bits, s_help))) { return; }
            __syncthreads();
        }
        __syncthreads();
    }
}

template <int H, int W, int CIN0_PAD, int CPAD, int CPL, bool BF = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(simWavesPerEu<H, W, CIN0_PAD, CPAD, BF>(), 4))) void sim_kernel(const SimArgs* __restrict__ a_, const uint8_t* __restrict__ rot_tab, int sim0, int nsims, int host_start)
{
    CSimArgs* a = (CSimArgs*)a_;
    extern __shared__ __attribute__((aligned(16))) float tiles[];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int games = gridDim.x;
    constexpr int WPE = simWavesPerEu<H, W, CIN0_PAD, CPAD, BF>();
    // the reciprocal table of the PUCT divisions lives in LDS above the tower's tiles for the whole launch
    constexpr int kTileFloats = simTileFloats<H, W, CIN0_PAD, CPAD, BF>();
    double* rcp_w = reinterpret_cast<double*>(tiles + kTileFloats);
    for (int i = tid; i < a->rcp_n; i += 512) { rcp_w[i] = a->pv.rcp_tab[i]; }
    __syncthreads();
    LdsCDouble* rcp_lds = (LdsCDouble*)rcp_w;
    // path-speculation memory of the walk (pool_body.h) behind the reciprocal table: LDS copies of the sqrt / bias tables and the remembered
    // paths — only in the one-game-per-CU kernels (9x9: deep principal variations); the 8x8 / 3x3 trees of BASELINE's configs are shallow
    // and those kernels need their LDS to keep two games on a CU
    SpecMem spec{nullptr, nullptr, nullptr};
    int* spec_w = nullptr;
    // the phases' hand-over block (SimXchg) behind whatever the kernel keeps in LDS, with the path of the simulation (2 * max_depth + 2 words) in front
    const int path_words = 2 * a->pv.max_depth + 2;
    float* xchg = reinterpret_cast<float*>(rcp_w + a->rcp_n) + path_words;
    if constexpr (WPE == 2) {
        // (pool_body.h specStage's layout, spelled out: with the helper inlined the compiler allocates this kernel's registers, which are at their limit, another
        //  way — the same counts, 799 other lines in the 9x9 x 64 instance — and this is the kernel bench.py measures)
        const int tab_n = a->rcp_n - 2;
        double* sqrt_w = rcp_w + a->rcp_n;
        float* bias_w = reinterpret_cast<float*>(sqrt_w + tab_n);
        spec_w = reinterpret_cast<int*>(bias_w + tab_n + (tab_n & 1));
        for (int i = tid; i < tab_n; i += 512) { sqrt_w[i] = a->pv.sqrt_tab[i]; bias_w[i] = a->pv.bias_tab[i]; }
        if (tid < kSpecWays) { spec_w[tid * kSpecWay] = 0; }
        if (tid < 8) { spec_w[kSpecNext + tid] = 0; }
        if (tid < kHelpSegs) { spec_w[kSpecHelp + tid * kHelpSeg] = 0; }
        __syncthreads();
        spec = SpecMem{(a->no_spec & 1) ? nullptr : (LdsI32*)spec_w, (LdsCFloat*)bias_w, (LdsCDbl*)sqrt_w};
        xchg = reinterpret_cast<float*>(spec_w + kSpecWords) + path_words;
    }
    // Go, one game per CU: the root's positional-superko table (8 KB, constant during the move) behind the hand-over block
    const uint64_t* seen_lds = nullptr;
    if constexpr (CPL > 0 && WPE == 2) {
        uint64_t* sw = reinterpret_cast<uint64_t*>(xchg + ((simXchgWordsDev(a->gv.A, a->gv.channels, a->gv.W32) + 1) & ~1));
        for (int i = tid; i < kGoSeenCap; i += 512) { sw[i] = a->gv.snap[g].seen[i]; }
        __syncthreads();
        seen_lds = sw;
    }
    // ... and behind it the leaf's scratch block, which then outlives the tower: the part of the leaf only the phases AFTER the network need (path
    // hashes, liberties, legal mask: 4.4 of its 8.1 us on BASELINE configs[1]) runs on waves 6 and 7 beside the heads, in which those waves have no share
    uint64_t* leaf_smem = nullptr;
    if constexpr (CPL > 0 && WPE == 2) {
        const HeadParams hp = ldc(&a->hp);
        if (hp.VH <= 256 && (hp.PC + 1) * hp.P <= 384 && hp.A <= 384 && !(a->no_spec & 8)) { // (MZ_NO_SPEC=8: off)
            leaf_smem = const_cast<uint64_t*>(seen_lds) + kGoSeenCap;
            uint64_t* zk = leaf_smem + goLeafKeyWord(a->gv.Ppad, a->gv.W, a->pv.max_depth); // the block's copy of the Zobrist keys (go_body.h)
            for (int i = tid; i < 2 * a->gv.P; i += 512) { zk[i] = a->gv.key[i]; }
            __syncthreads();
        }
    }
    // 9x9 Go x 64 channels: the small launch-invariant weights of the heads in an LDS block of their own behind everything above (net_body.h HeadsAhead), staged
    // once per launch — the weights only change between launches.  a->heads_lds is the block's word offset, 0 where the launch has no room for it or the network
    // is not of the shape: the old heads then.  MZ_NO_SPEC=512: the old heads beside a staged block (A/B, tests).
    constexpr bool kAhead = !BF && H == 9 && W == 9 && CIN0_PAD == 20 && CPAD == 64 && CPL == 2;
    [[maybe_unused]] const float* heads_w = nullptr;
    [[maybe_unused]] unsigned long long ahead_n = 0; // (MZ_SIM_PROF) simulations whose heads were the new ones
    if constexpr (kAhead) {
        const int off = a->heads_lds;
        if (off > 0) {
            headsAheadStage(ldc(&a->hp), tiles + off, tid, 512); // (the barrier in front of the first simulation is behind it)
            if (!(a->no_spec & 512)) { heads_w = tiles + off; }
        }
    }
    unsigned long long* prof = a->prof ? a->prof + size_t(g) * 8 : nullptr;
    int* const node_count = reinterpret_cast<int*>(xchg) - 1; // (the spare word of the path block: simPathView)
    if (tid == 0) { *node_count = a->pv.num_nodes[g]; }
    if (prof && tid == 0) { simProfEnter(a->prof + size_t(games) * 8); }
    // Tail help (sim_help.h; bit 1 of host_start: this launch helps): the game publishes the XCD it runs on — from here on it can be claimed by a workgroup of
    // that XCD whose own game is done.  s_help: [0] abort flag of the exchanges, [1] the game's tower as of this simulation (0: solo, 1: pair, 2: quad), [2], [3] the
    // helper's scratch (and the volunteer's, simLendTower).
    constexpr bool kHelp = !BF && WPE == 2 && CPL > 0 && pairTowerShape<H, W, CPAD>();
    __shared__ int s_help[kHelp ? kVfWords : 4]; // (+ the words of the value-first order: kVfBackup ..)
    const bool help_on = kHelp && (host_start & 2) != 0;
    unsigned* const help_blk = help_on ? a->help + size_t(g) * a->help_words : nullptr;
    unsigned help_xseq = 0;                        // layer exchanges of this game's pair and quad towers so far
    unsigned long long pair_n = 0, pair_t = 0;     // (MZ_SIM_PROF) simulations that ran a pair tower, their tower ticks
    unsigned long long quad_n = 0, quad_t = 0;     // ... a quad tower
    unsigned long long lent_n = 0, lent_t = 0;     // ... a pair tower with a volunteer (lending), counted by the owner
    unsigned long long lend_t = 0;                 // ... ticks this workgroup spent as a volunteer
    if (help_on && tid == 0) { s_help[0] = 0; s_help[1] = 0; hpStoreU(help_blk + kHpXcc, hpXccId()); }
    // The value-first order (simWalkVf .. simCandPipeVf above): the same for every simulation of the launch and for every wave, so each wave passes the same barriers
    bool vf = false;
    if constexpr (kHelp) {
        vf = leaf_smem != nullptr && !a->use_gumbel && !a->pv.value_rescale && a->cand_coop != 2 && !(a->no_spec & 64); // (MZ_NO_SPEC=64: the order of the other instances;
                                                                                                                         //  cand_coop 2 is the wide boards' sort, which simCandPipeVf does not have: never set for this instance's 82 actions)
        if (tid >= kVfBackup && tid < kVfWords) { s_help[tid] = 0; }
    }
    unsigned long long vf_t0 = 0, vf_n = 0; // (MZ_SIM_PROF) the start of the walk that ran in the iteration before, simulations in the new order
    // Lending (sim_help.h): in a launch that helps, in the value-first order (MZ_NO_SPEC=256: off)
    const bool lend_on = kHelp && help_on && vf && !(a->no_spec & 256);
    __syncthreads();
    for (int s = 0; s < nsims; ++s) {
        const int slot = sim0 + s; // simulation index within the move = position slot of its leaf
        const int rot = rot_tab[size_t(s) * games + g];
        unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        if (prof) { t0 = (vf && s > 0) ? vf_t0 : wall_clock64(); }
        if (kHelp && vf) {
            if constexpr (kHelp) {
                if (wave == 0) {
                    if (s == 0) { // (the first walk of the launch; every later one ran behind the backup of the simulation before it)
                        if (slot == 1 && a->root_noise) { simApplyRootNoise<WPE>(a, g, lane); }
                        simWalkVf(a, g, lane, rcp_lds, spec, xchg, (a->no_spec & 2) ? 0 : 1, -1, 0, s_help);
                        if (lend_on && lane == 0) { __hip_atomic_store((LdsI32*)s_help + kVfWalked, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
                    } else {
                        // the join in front of the leaf: leafBody writes the hand-over block the candidate pipeline reads, and the node count is the expand's
                        const bool waited = vfWait((LdsI32*)s_help + kVfExpand, s, a->err, lane);
                        if (prof && waited && lane == 0) { s_help[kVfStats + 3] += 1; }
                        // (behind the expand of simulation s - 1, i.e. up to one walk later than in the old order, which publishes at the end of iteration s - 1: a finished
                        //  CU that looks for the game with the least progress sees this game one simulation behind for that long; the protocol only needs progress < the next
                        //  command's sequence number s + 1)
                        if (help_on && lane == 0) { hpStoreU(help_blk + kHpProgress, unsigned(s)); }
                    }
                    simLeafVf<CPL>(a, rot, slot, g, lane, xchg, seen_lds, leaf_smem, s_help);
                } else if (s == 0 && wave <= kHelpSegs && spec.w && !(a->no_spec & 2)) {
                    simSelectHelper(a, g, lane, wave, 1, rcp_lds, spec);
                } else if (lend_on && wave == 7) {
                    simLendScan(a, g, lane, s, nsims, help_blk, s_help); // (the game's offer and the offers of the others; s_help[1] like below)
                } else if (help_on && tid == 7 * 64) {
                    // (wave 7 arrives here behind its rank shares of simulation s - 1, not beside the walk as in the old order: a claim made during the walk of s is
                    //  picked up one simulation later)
                    s_help[1] = simHelpMode(help_blk);
                }
            }
        } else if (wave == 0) {
            if (slot == 1 && a->root_noise) { simApplyRootNoise<WPE>(a, g, lane); }
            if (a->use_gumbel) { simGumbelStart<WPE>(a, slot, s == 0 && (host_start & 1) != 0, g, lane, tiles); }
            simSelectLeaf<CPL, WPE>(a, rot, slot, g, lane, tiles, rcp_lds, spec, xchg, seen_lds, (a->no_spec & 2) ? 0 : s + 1, leaf_smem);
        } else if (WPE == 2 && wave <= kHelpSegs && spec.w && !(a->no_spec & 2)) { // (MZ_NO_SPEC=2: helper segments off)
            simSelectHelper(a, g, lane, wave, s + 1, rcp_lds, spec);
        } else if (kHelp && help_on && tid == 7 * 64) {
            // has a helper claimed this game?  Looked up past the vector cache by a wave that has no part in the walk, handed to all waves behind the walk's
            // barrier: the branch "pair tower or solo tower" is uniform over the workgroup, and a game without a helper pays nothing for looking
            s_help[1] = simHelpMode(help_blk);
        }
        __syncthreads();
        const int help_mode = (kHelp && help_on) ? __builtin_amdgcn_readfirstlane(s_help[1]) : 0;
        const bool lent = lend_on && __builtin_amdgcn_readfirstlane(s_help[kVfOffer]) != 0; // a volunteer has taken this simulation's offer: member 1 of its pair tower
        const bool pair = help_mode == 1 || lent, quad = help_mode == 2;
        // A terminal leaf has no children and its value is the game result (zero_actor.cpp:85): nobody reads the network's outputs, so planes, tower and heads
        // are not run for it.  The flag is wave 0's (simLeafTerminal), read by every wave behind the barrier: the branches on it are uniform over the workgroup,
        // and every wave passes the same barriers on either side.  (Each phase is skipped on its own, the barriers behind tower and heads stay where they are:
        // with one branch around all three the 128-VGPR kernels spilled 34 VGPRs instead of 24 (23 before the skip), and BASELINE configs[2] ran 2-3 % slower.)
        const bool term = simLeafTerminal(a, xchg);
        if constexpr (kHelp) {
            if (lend_on) {
                if (lent && term && tid == 7 * 64) { hpStoreU(help_blk + kHpOffer, 0u); } // no tower: the offer is withdrawn, the volunteer goes on
                const int lend_to = __builtin_amdgcn_readfirstlane(s_help[kVfLend]);
                if (lend_to != 0) { // one tower of a game that is behind, then this game's own planes and tower
                    const unsigned long long tl0 = prof ? wall_clock64() : 0;
                    if (!simLendTower<H, W, CIN0_PAD, CPAD>(a, lend_to - 1, __builtin_amdgcn_readfirstlane(s_help[kVfLend + 1]), tid, tiles, s_help)) { return; }
                    if (prof) { const unsigned long long d = wall_clock64() - tl0; t0 += d; lend_t += d; } // (not part of this game's walk and leaf)
                }
            }
        }
        if constexpr (CPL > 0) {
            if (!term) {
                simLeafPlanes<CPL>(a, rot, g, wave, lane, leaf_smem ? leaf_smem : reinterpret_cast<const uint64_t*>(tiles), xchg);
                __syncthreads();
            }
        }
        if (prof) { t1 = wall_clock64(); }
        const float* xt = nullptr;
        if (!term) {
            if constexpr (BF) { xt = simTowerBf16<H, W>(a, g, tid, tiles, xchg); }
            else if constexpr (WPE == 4) {
                // The 128-VGPR build (two games per CU): as a function of its own the tower saved and restored 20 callee-saved VGPRs per call — 8 waves x 5 KB each way
                // per simulation, most of the 118 KB of HBM traffic per leaf evaluation that rocprofv3 showed for BASELINE configs[2] (profiles/r04_pmc_c3.json).  Its
                // 2 pixel tiles per wave fit the kernel's own budget.
                const GoDevView gvt = simLeafView(ldc(&a->gv), xchg, g);
                xt = towerBody<H, W, CIN0_PAD, CPAD>(reinterpret_cast<const float*>(gvt.feat), a->params, *(const TowerArgs*)&a->ta, nullptr, g, tid, tiles);
            }
            else if constexpr (kHelp) {
                if (pair) { // with the game's helper: half of the output channels each (sim_help.h)
                    xt = simTowerPair<H, W, CIN0_PAD, CPAD>(a, g, tid, tiles, xchg, s + 1, help_xseq, s_help, lent ? 1 : 0);
                    if (!xt) { return; } // the helper went missing: the error flag is raised
                    help_xseq += unsigned(a->ta.nlayers);
                    if (lent && tid == 7 * 64) { hpStoreU(help_blk + kHpOffer, 0u); } // (the volunteer's last exchange is read: the word is reset)
                }
                else if (quad) { // with three helpers: one oc-tile each
                    xt = simTowerQuad<H, W, CIN0_PAD, CPAD>(a, g, tid, tiles, xchg, s + 1, help_xseq, s_help);
                    if (!xt) { return; }
                    help_xseq += unsigned(a->ta.nlayers);
                }
                else { xt = simTower<H, W, CIN0_PAD, CPAD>(a, g, tid, tiles, xchg); }
            }
            else { xt = simTower<H, W, CIN0_PAD, CPAD>(a, g, tid, tiles, xchg); } // its own function: its own register budget
        }
        __syncthreads();
        if (prof) { t2 = wall_clock64(); }
        // (the leaf's second half — a terminal leaf's score among it — runs on waves 6 and 7 either way; it passes two barriers, like the heads beside it)
        if constexpr (WPE == 4) { if (!term) { simHeadsImpl<WPE>(a, g, tid, tiles, xt, planeStride(H, W), W + 2, xchg); } }
        else if (leaf_smem && wave >= 6) { simLeafRest<CPL>(a, rot, slot, g, lane, xchg, seen_lds, leaf_smem, 7 - wave); }
        else if (!term) {
            bool ahead = false;
            if constexpr (kAhead) { ahead = heads_w != nullptr; }
            if (ahead) { if constexpr (kAhead) { simHeadsAhead<H, W>(a, tid, tiles, xt, xchg, heads_w); } }
            else { simHeads<WPE, false, (MZ_HEADS_FP != 0)>(a, g, tid, tiles, xt, planeStride(H, W), W + 2, xchg); }
        }
        else if (leaf_smem) { __syncthreads(); __syncthreads(); }
        __syncthreads();
        if (prof) { t3 = wall_clock64(); }
        if (kHelp && vf) {
            if constexpr (kHelp) {
                // no barrier from here to the one behind the next leaf: the waves meet through the words of s_help
                const bool more = s + 1 < nsims;
                if (wave == 0) {
                    simBackupOnly<WPE>(a, slot, g, lane, tiles, xchg);
                    vfPublish((LdsI32*)s_help + kVfBackup, s + 1, lane);
                    if (prof && tid == 0) {
                        t4 = wall_clock64(); // ("cand+expand": what is exposed between the heads and the next walk)
                        simProfSim(prof, t0, t1, t2, t3, t4, term);
                        if (pair && !lent && !term) { pair_n += 1; pair_t += t2 - t1; }
                        if (quad && !term) { quad_n += 1; quad_t += t2 - t1; }
                        if (lent && !term) { lent_n += 1; lent_t += t2 - t1; }
                        if constexpr (kAhead) { if (heads_w && !term) { ahead_n += 1; } }
                        vf_n += 1;
                    }
                    vf_t0 = t4;
                    if (more) {
                        if (slot + 1 == 1 && a->root_noise) { // the noise re-orders the root's priors, which the expand of simulation 0 writes
                            vfWait((LdsI32*)s_help + kVfExpand, s + 1, a->err, lane);
                            simApplyRootNoise<WPE>(a, g, lane);
                        }
                        simWalkVf(a, g, lane, rcp_lds, spec, xchg, (a->no_spec & 2) ? 0 : s + 2, __builtin_amdgcn_readfirstlane(s_help[kVfLeaf]), s + 1, s_help);
                        if (lend_on && lane == 0) { __hip_atomic_store((LdsI32*)s_help + kVfWalked, s + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
                    }
                } else if (wave <= kHelpSegs) {
                    if (more && spec.w && !(a->no_spec & 2)) { // (their blocks claim "with the records as they are": behind the backup)
                        vfWait((LdsI32*)s_help + kVfBackup, s + 1, a->err, lane);
                        simSelectHelper(a, g, lane, wave, s + 2, rcp_lds, spec);
                    }
                } else {
                    simCandPipeVf<WPE>(a, rot, slot, g, lane, wave - 4, s + 1, tiles, xchg, s_help);
                }
            }
            continue;
        }
        if (wave == 0) { simCandGather<WPE>(a, rot, g, lane, tiles, xchg); }
        __syncthreads();
        {
            const int A = a->gv.A;
            const SimXchg x{A + (A & 1)};
            if (a->cand_coop) { simCandRank(A, reinterpret_cast<const int*>(xchg + x.scalars())[1], wave, lane, tiles); }
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
            if (pair && !term) { pair_n += 1; pair_t += t2 - t1; }
            if (quad && !term) { quad_n += 1; quad_t += t2 - t1; }
            if constexpr (kAhead) { if (heads_w && !term) { ahead_n += 1; } }
        }
        if (kHelp && help_on && tid == 0) { hpStoreU(help_blk + kHpProgress, unsigned(s) + 1u); } // (nsims: the game is done, its helper looks for another one)
    }
    if constexpr (kHelp) {
        if (vf) { // the candidate pipeline of the last simulation: the node count and the progress word of the tail help are written behind its expand
            __syncthreads();
            if (help_on && tid == 0) { hpStoreU(help_blk + kHpProgress, unsigned(nsims)); }
            if (prof && tid == 0) {
                unsigned long long* ptail = a->prof + size_t(games) * 8;
                atomicAdd(ptail + 16, vf_n);
                for (int i = 0; i < 4; ++i) { atomicAdd(ptail + 17 + i, static_cast<unsigned long long>(s_help[kVfStats + i])); }
                if (lend_on) { // lending: [33] towers with a volunteer, [34] their tower ticks; the volunteers' side: [35] offers taken, [36] taken too late, [37] withdrawn, [38] ticks
                               // waited for the command, [39] ticks from the barrier behind the leaf to the end of the lent tower
                    atomicAdd(ptail + 33, lent_n); atomicAdd(ptail + 34, lent_t);
                    for (int i = 0; i < 4; ++i) { atomicAdd(ptail + 35 + i, static_cast<unsigned long long>(s_help[kVfLendStat + i])); }
                    atomicAdd(ptail + 39, lend_t);
                }
            }
        }
    }
    if (tid == 0) { a->pv.num_nodes[g] = *node_count; }
    if (prof && tid == 0) {
        simProfExit(a->prof + size_t(games) * 8);
        if constexpr (kAhead) { if (ahead_n) { atomicAdd(a->prof + size_t(games) * 8 + 7, ahead_n); } } // tail word [7]: simulations that ran the heads with their operands ahead
        if (pair_n) { atomicAdd(a->prof + size_t(games) * 8 + 13, pair_n); atomicAdd(a->prof + size_t(games) * 8 + 14, pair_t); }
        if (quad_n) { atomicAdd(a->prof + size_t(games) * 8 + 21, quad_n); atomicAdd(a->prof + size_t(games) * 8 + 22, quad_t); atomicAdd(a->prof + size_t(games) * 8 + 23, pair_n ? 1ull : 0ull); }
    }
    if (prof && tid == 0 && spec_w) { simProfSpec(prof, spec_w); }
    if constexpr (kHelp) {
        // this game is done and its results are written: the CU helps the stragglers of its XCD with their towers instead of idling to the end of the launch
        if (help_on) {
            const int A = a->gv.A;
            const SimXchg x{A + (A & 1)};
            __syncthreads();
            simHelpTail<H, W, CIN0_PAD, CPAD>(a, g, tid, tiles, reinterpret_cast<unsigned*>(xchg + x.feat()), nsims, s_help);
        }
    }
}


} // namespace mz
