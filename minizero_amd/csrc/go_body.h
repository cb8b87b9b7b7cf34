// Device bodies of the device-resident Go leaf environment (see go_dev.h), shared by the stand-alone kernels (go_dev.hip) and the
// per-game simulation kernel (sim.hip).  Each body is run by ONE wave64 for game `g`; waveSync() orders its LDS traffic.
#pragma once
#include "go_dev.h"
#include "sort_emul.h"

#ifndef MZ_LPROF
#define MZ_LPROF(k) // experiment hook (sim.hip -DMZ_SIM_LPROF): time stamps inside the single-wave tree phases
#endif
#ifndef MZ_BPROF
#define MZ_BPROF(role, k) // experiment hook (sim.hip -DMZ_SIM_BPROF): time stamps inside the part of the leaf that runs beside the heads
#endif

namespace mz {

// single-wave phases: make the wave's LDS / global writes visible to its other lanes (no s_barrier: the other waves of a
// 512-thread workgroup are parked at a real barrier while wave 0 runs the tree phases of the simulation kernel)
__device__ __forceinline__ void waveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// (+ behind the arrays of the body: two words handed from PART 1 to PART 2, and a copy of the 2 x P Zobrist keys for the kernels that keep the block for a whole launch)
__host__ __device__ inline size_t goLeafKeyWord(int Ppad, int W, int max_depth) { return (sizeof(uint64_t) * (size_t(Ppad) + max_depth + 4 + 18 * W) + size_t(Ppad) * (4 + 2 + 1)) / sizeof(uint64_t) + 2; }
inline size_t goLeafSmemBytes(const GoDevView& v, int max_depth) { return sizeof(uint64_t) * (goLeafKeyWord(v.Ppad, v.W, max_depth) + 2 * size_t(v.P)); }

struct Cand { int action; float policy, logit; };
struct CandGreater { __host__ __device__ bool operator()(const Cand& l, const Cand& r) const { return l.policy > r.policy; } };
using CandSort = StdSortEmul<Cand, CandGreater>;
constexpr size_t kSortStackBytes = 3 * CandSort::kStack * sizeof(int);
inline size_t azCandSmemBytes(int A) { return 2 * size_t(A) * sizeof(Cand) + kSortStackBytes + 16; }

__device__ inline uint64_t shflXor64(uint64_t v, int o)
{
    const unsigned lo = __shfl_xor(static_cast<unsigned>(v), o), hi = __shfl_xor(static_cast<unsigned>(v >> 32), o);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ inline uint64_t waveXor64(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) { v ^= shflXor64(v, o); }
    return v;
}
__device__ inline uint64_t normH(uint64_t h) { return h ? h : 1; }
__device__ inline int rotOf(const RotPack& r, int g) { return (r.w[g / 10] >> (3 * (g % 10))) & 7; }

// leafBody<CPL>: position + legal mask + feature planes of the leaf selected for game `g`, by the rules that CPL names (game_kind.h rulesArg) — every kernel that
// evaluates a leaf calls this one name.  CPL > 0 is Go, whose body this is (`goLeafBody` in earlier notes and profiles); the overload for the other games
// follows their bodies below.  (Two overloads and not one function that forwards to Go's body: forwarding puts a second inlining level, with its own no-alias
// scopes, around the body and changes its register allocation.)  One wave64; `smem` as sized by goLeafSmemBytes.
// PART 0: everything.  PART 1 / 2 (the one-game-per-CU simulation kernel, whose `smem` block then outlives the tower): 1 = what the network needs — the
// leaf's position (parent + move, stored to its slot), the history block of the planes, the player to move and the terminal flag; 2 = what only the
// phases AFTER the network need — the path's hashes, the groups' liberties and key sums, the legal mask, the score of a terminal leaf — run by another
// wave beside the heads: with SYNC it passes a workgroup barrier after the liberties and after the legal mask (the two barriers inside headsBody), and
// TWO waves share the work — ROLE 0: liberties + key sums | barrier | legal mask of the even 64-point chunks | barrier | score; ROLE 1: the path's hashes |
// barrier | legal mask of the odd chunks | barrier — so that each piece fits the interval of the heads it runs beside
template <int CPL, bool EXT_PLANES = false, int PART = 0, bool SYNC = false, int ROLE = 0, std::enable_if_t<(CPL > 0), int> = 0>
// EXT_PLANES: the caller builds the feature planes itself from the history block this body leaves in `smem` (goPlanesPart, all waves)
// seen_lds: optional LDS copy of the root's positional-superko table (GoRootSnapshot::seen; constant during a move) — the simulation kernel
// makes one per launch so that the probes of every candidate point are LDS reads instead of dependent trips to L2
__device__ __forceinline__ void leafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane, uint64_t* __restrict__ smem,
                                         const uint64_t* __restrict__ seen_lds = nullptr)
{
    const int P = v.P, n = v.n, W = v.W, Ppad = v.Ppad, MD = pv.max_depth;
    uint64_t* gh = smem;                                   // [Ppad] XOR of the keys of a group, by group id
    uint64_t* ph = gh + Ppad;                              // [MD + 4] (normalised) hashes of the positions along the path, 0-padded to a multiple of 4
    uint64_t* hb = ph + MD + 4;                            // [8][2][W] stones k moves before the leaf
    uint64_t* cur = hb + 16 * W;                           // [2][W] stones at the leaf
    int* libs = reinterpret_cast<int*>(cur + 2 * W);       // [Ppad] liberties of a group, by group id
    uint16_t* lab = reinterpret_cast<uint16_t*>(libs + Ppad); // [Ppad] group id per point
    uint8_t* col = reinterpret_cast<uint8_t*>(lab + Ppad);  // [Ppad] 0 empty, 1 black, 2 white, 3 off board
    uint64_t* stash = reinterpret_cast<uint64_t*>(col + Ppad); // [2] PART 1 -> PART 2: the leaf's hash; terminal flag, player to move, move / pass counters (Ppad is a multiple of 64: aligned)
    // the Zobrist keys: with PART 1 / 2 the caller keeps a copy behind the stash (LDS) — a key is on the walk's critical path at every move
    const uint64_t* zkey = PART != 0 ? smem + goLeafKeyWord(Ppad, W, MD) : v.key;

    const int len = pv.path_len[g];
    const int* path = pv.path + size_t(g) * MD;
    const int* pact = pv.path_action + size_t(g) * MD;
    const int depth = len - 1;
    const GoRootSnapshot& S = v.snap[g];
    const int root_turn = S.turn, root_hist_len = S.hist_len;
    const size_t sb = size_t(g) * v.slots;
    const int* hs = pv.hslot + size_t(g) * pv.cap;
    const int src = depth == 0 ? 0 : hs[path[len - 2]];

    int c[CPL], l[CPL];
    short nb[CPL][4];
    uint64_t sbw[CPL], sww[CPL];
    uint64_t hash = 0;
    int nmoves = 0, passes = 0;
    int t = (depth & 1) ? 3 - root_turn : root_turn; // the player to move at the leaf
    bool terminal = false;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int p = i * 64 + lane;
        nb[i][0] = nb[i][1] = nb[i][2] = nb[i][3] = -1;
        if (p < P) {
            const int x = p % n, y = p / n;
            if (y + 1 < n) { nb[i][0] = static_cast<short>(p + n); }
            if (x + 1 < n) { nb[i][1] = static_cast<short>(p + 1); }
            if (y > 0) { nb[i][2] = static_cast<short>(p - n); }
            if (x > 0) { nb[i][3] = static_cast<short>(p - 1); }
        }
    }
    if constexpr (PART == 2) { // the leaf as PART 1 left it in the block
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            c[i] = col[p];
            l[i] = lab[p];
            sbw[i] = cur[i];
            sww[i] = cur[W + i];
        }
        hash = stash[0];
        terminal = (stash[1] & 1) != 0;
        t = static_cast<int>((stash[1] >> 1) & 3); // (no trip to the root's snapshot in global memory)
        passes = static_cast<int>((stash[1] >> 4) & 15);
        nmoves = static_cast<int>(stash[1] >> 8);
    }
    if constexpr (PART != 2) {
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int p = i * 64 + lane;
        sbw[i] = v.stones[((sb + src) * 2 + 0) * W + i];
        sww[i] = v.stones[((sb + src) * 2 + 1) * W + i];
        c[i] = 3;
        l[i] = 0;
        if (p < P) {
            c[i] = ((sbw[i] >> lane) & 1) ? 1 : (((sww[i] >> lane) & 1) ? 2 : 0);
            l[i] = v.lab[(sb + src) * Ppad + p];
        }
        col[p] = static_cast<uint8_t>(c[i]);
        lab[p] = static_cast<uint16_t>(l[i]);
    }
    hash = v.hash[sb + src];
    nmoves = v.meta[(sb + src) * 2]; passes = v.meta[(sb + src) * 2 + 1];
    waveSync();
    MZ_LPROF(1); // parent slot loaded

    if (depth >= 1) { // leaf = parent + one move (ref go.cpp:132-190, observable effects only)
        const int a = pact[len - 1], m = 3 - t;
        ++nmoves;
        hash ^= v.turn_key; // situational superko: every move, pass included (ref go.cpp:141); 0 with the positional rule
        if (a >= P) {
            passes = passes + 1 > 2 ? 2 : passes + 1;
        } else {
            passes = 0;
            const int ax = a % n, ay = a / n;
            const int an[4] = {ay + 1 < n ? a + n : -1, ax + 1 < n ? a + 1 : -1, ay > 0 ? a - n : -1, ax > 0 ? a - 1 : -1};
            int own[4], en[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                own[k] = -1;
                en[k] = -1;
                if (an[k] >= 0) {
                    const int cq = col[an[k]];
                    if (cq == m) { own[k] = lab[an[k]]; }
                    else if (cq == 3 - m) { en[k] = lab[an[k]]; }
                }
            }
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                for (int j = 0; j < k; ++j) { if (en[j] == en[k]) { en[k] = -1; } }
            }
            waveSync();
            // place the stone; the own groups it touches become one group whose id is the new point (unused as an id: it was empty)
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int p = i * 64 + lane;
                if (p == a) { c[i] = m; l[i] = a; }
                else if (c[i] == m && (l[i] == own[0] || l[i] == own[1] || l[i] == own[2] || l[i] == own[3])) { l[i] = a; }
                col[p] = static_cast<uint8_t>(c[i]);
                lab[p] = static_cast<uint16_t>(l[i]);
            }
            waveSync();
            // which of the adjacent enemy groups still have a liberty
            unsigned flags = 0;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                if (c[i] != 0) { continue; }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = nb[i][k];
                    if (q >= 0 && col[q] == 3 - m) {
                        const int lq = lab[q];
#pragma unroll
                        for (int j = 0; j < 4; ++j) { if (lq == en[j]) { flags |= 1u << j; } }
                    }
                }
            }
            bool cap[4], any_cap = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cap[j] = en[j] >= 0 && __ballot((flags >> j) & 1) == 0;
                any_cap |= cap[j];
            }
            uint64_t hx = 0;
            if (any_cap) {
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int p = i * 64 + lane;
                    if (c[i] == 3 - m && ((cap[0] && l[i] == en[0]) || (cap[1] && l[i] == en[1]) || (cap[2] && l[i] == en[2]) || (cap[3] && l[i] == en[3]))) {
                        c[i] = 0;
                        col[p] = 0;
                        hx ^= zkey[size_t(2 - m) * P + p];
                    }
                }
                hx = waveXor64(hx);
            }
            hash ^= zkey[size_t(m - 1) * P + a] ^ hx;
            waveSync();
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            sbw[i] = __ballot(c[i] == 1);
            sww[i] = __ballot(c[i] == 2);
            if constexpr (PART != 1) { // (PART 1 leaves the slot's store to PART 2: the next fence would wait for it)
                if (lane == 0) {
                    v.stones[((sb + slot) * 2 + 0) * W + i] = sbw[i];
                    v.stones[((sb + slot) * 2 + 1) * W + i] = sww[i];
                }
                if (p < P) { v.lab[(sb + slot) * Ppad + p] = static_cast<uint16_t>(l[i]); }
            }
        }
        if constexpr (PART != 1) {
            if (lane == 0) {
                v.hash[sb + slot] = hash;
                v.meta[(sb + slot) * 2] = nmoves;
                v.meta[(sb + slot) * 2 + 1] = passes;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        if (lane == 0) { cur[i] = sbw[i]; cur[W + i] = sww[i]; }
    }
    MZ_LPROF(2); // move applied, slot stored
    terminal = passes >= 2 || nmoves > 2 * P; // ref go.cpp:246-257
    if (lane == 0) { stash[0] = hash; stash[1] = (terminal ? 1 : 0) | (static_cast<uint64_t>(t) << 1) | (static_cast<uint64_t>(passes) << 4) | (static_cast<uint64_t>(nmoves) << 8); }
    if constexpr (PART == 1) { // (PART 2 counts the liberties on two waves: the counters are cleared here)
#pragma unroll
        for (int i = 0; i < CPL; ++i) { libs[i * 64 + lane] = 0; gh[i * 64 + lane] = 0; }
    }
    waveSync();
    // ---- feature planes (ref go.cpp:280-308): planes 2k / 2k+1 = own / opponent stones k moves ago, 16 / 17 = black / white to move ----
    const int avail = root_hist_len + depth;
    for (int idx = lane; idx < 16 * W; idx += 64) {
        const int k = idx / (2 * W), cw = idx % (2 * W);
        uint64_t val = 0;
        if (k < avail) {
            if (k == 0) { val = cur[cw]; }
            else if (k < depth) { val = v.stones[(sb + hs[path[len - 1 - k]]) * 2 * W + cw]; }
            else { val = S.hist[(root_hist_len - 1 - (k - depth)) & 7][cw / W][cw % W]; }
        }
        hb[idx] = val;
    }
    waveSync();
    if constexpr (!EXT_PLANES) {
        const uint16_t* map = v.inv + size_t(rot) * P;
        uint32_t* out = v.feat + size_t(g) * 18 * v.W32;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            const int q = p < P ? map[p] : 0;
            uint64_t mine = 0; // lane ch keeps plane ch's word
            for (int ch = 0; ch < 16; ++ch) {
                const int k = ch >> 1, color = (ch & 1) == 0 ? t - 1 : 2 - t;
                const bool bit = p < P && ((hb[(k * 2 + color) * W + (q >> 6)] >> (q & 63)) & 1);
                const uint64_t bal = __ballot(bit);
                if (lane == ch) { mine = bal; }
            }
            const uint64_t ones = __ballot(p < P);
            if (lane == 16) { mine = t == 1 ? ones : 0; }
            if (lane == 17) { mine = t == 2 ? ones : 0; }
            if (lane < 18) {
                if (2 * i < v.W32) { out[lane * v.W32 + 2 * i] = static_cast<uint32_t>(mine); }
                if (2 * i + 1 < v.W32) { out[lane * v.W32 + 2 * i + 1] = static_cast<uint32_t>(mine >> 32); }
            }
        }
    }
    MZ_LPROF(5); // planes
    if (lane == 0) {
        v.leaf_player[g] = t;
        v.terminal[g] = terminal ? 1 : 0;
    }
    } // PART != 2
    if constexpr (PART == 1) { return; }
    constexpr bool kShared = PART == 2 && SYNC; // two waves share PART 2 (ROLE)
    static_assert(PART != 2 || SYNC, "PART 2 is the two-wave version (it also stores the leaf's slot)");
    MZ_BPROF(ROLE, 0);
    // the legal mask of the 64-point chunks i with want(i) (ref go.cpp:208-244): not occupied, not suicide, not a positional-superko repeat
    auto legalMask = [&](auto want) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (!want(i)) { continue; }
            bool bit = false;
            if (c[i] == 0 && !terminal) {
                const int p = i * 64 + lane;
                bool ok = false;
                uint64_t nh = hash ^ v.turn_key ^ zkey[size_t(t - 1) * P + p];
                int capl[4], ncap = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = nb[i][k];
                    if (q < 0) { continue; }
                    const int cq = col[q];
                    if (cq == 0) { ok = true; continue; }
                    const int lq = lab[q];
                    if (cq == t) {
                        if (libs[lq] > 1) { ok = true; }
                    } else if (libs[lq] == 1) { // an enemy group in atari is captured: each group once
                        bool dup = false;
                        for (int j = 0; j < ncap; ++j) { dup |= capl[j] == lq; }
                        if (!dup) { capl[ncap++] = lq; nh ^= gh[lq]; }
                        ok = true;
                    }
                }
                if (ok) {
                    const uint64_t h = normH(nh);
                    bool rep = false;
                    const uint64_t* seen = seen_lds ? seen_lds : S.seen;
                    for (uint32_t s = static_cast<uint32_t>(h) & (kGoSeenCap - 1);; s = (s + 1) & (kGoSeenCap - 1)) {
                        const uint64_t e = seen[s];
                        if (e == 0) { break; }
                        if (e == h) { rep = true; break; }
                    }
                    for (int d = 0; d < depth; d += 4) { // four hashes per step, no early exit: a deep path made this loop the longest part of the leaf
                        const uint64_t a0 = ph[d], a1 = ph[d + 1], a2 = ph[d + 2], a3 = ph[d + 3];
                        rep |= (a0 == h) | (a1 == h) | (a2 == h) | (a3 == h);
                    }
                    bit = !rep;
                }
            }
            uint64_t w = __ballot(bit);
            if (i == (P >> 6)) { w |= 1ull << (P & 63); } // pass is always legal
            if (lane == 0) { v.legal[size_t(g) * v.LW + i] = w; }
        }
    };
    // Shared by two waves, the pieces are laid into the three intervals of the heads (conv1x1 | FCs | softmax + value: 2.2 / 2.9 / 2.2 us on BASELINE configs[1]):
    //   ROLE 0: liberties of the even chunks              | barrier | key sums, legal mask of the even chunks | barrier | score of a terminal leaf, the leaf's scalars
    //   ROLE 1: path hashes, liberties of the odd chunks  | barrier |                                        | barrier | legal mask of the odd chunks
    // ---- hashes along the path (d = 1 .. depth; the root and everything before it is in the root's table) ----
    if (!kShared || ROLE == 1) {
        for (int d = 1 + lane; d <= depth; d += 64) { ph[d - 1] = normH(d == depth ? hash : v.hash[sb + hs[path[d]]]); }
        if (lane < 4) { ph[depth + lane] = 0; } // normH never returns 0: the padding matches no candidate
    }
    // ---- group liberties / key sums at the leaf ----
    if constexpr (!kShared) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) { libs[i * 64 + lane] = 0; gh[i * 64 + lane] = 0; }
        waveSync();
    }
    {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (kShared && (i & 1) != ROLE) { continue; }
            if (c[i] != 0) { continue; }
            int seen_l[4], ns = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = nb[i][k];
                if (q < 0 || col[q] == 0) { continue; }
                const int lq = lab[q];
                bool dup = false;
                for (int j = 0; j < ns; ++j) { dup |= seen_l[j] == lq; }
                if (!dup) { seen_l[ns++] = lq; atomicAdd(&libs[lq], 1); }
            }
        }
    }
    waveSync();
    MZ_BPROF(ROLE, 1);
    if constexpr (SYNC) { __syncthreads(); }
    MZ_BPROF(ROLE, 2);
    if constexpr (kShared && ROLE == 1) { // the leaf's position into its slab slot (PART 1 left it out)
        if (depth >= 1) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int p = i * 64 + lane;
                if (lane == 0) {
                    v.stones[((sb + slot) * 2 + 0) * W + i] = sbw[i];
                    v.stones[((sb + slot) * 2 + 1) * W + i] = sww[i];
                }
                if (p < P) { v.lab[(sb + slot) * Ppad + p] = static_cast<uint16_t>(l[i]); }
            }
            if (lane == 0) {
                v.hash[sb + slot] = hash;
                v.meta[(sb + slot) * 2] = nmoves;
                v.meta[(sb + slot) * 2 + 1] = passes;
            }
        }
    }
    if (!kShared || ROLE == 0) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            if (c[i] == 3 - t && libs[l[i]] == 1) { atomicXor(reinterpret_cast<unsigned long long*>(&gh[l[i]]), static_cast<unsigned long long>(zkey[size_t(2 - t) * P + p])); }
        }
        waveSync();
        MZ_LPROF(3); // path hashes, liberties, key sums
        if constexpr (kShared) { legalMask([](int i) { return (i & 1) == 0; }); }
        else { legalMask([](int) { return true; }); }
        if (v.LW > CPL && lane == 0) { v.legal[size_t(g) * v.LW + CPL] = (P >> 6) == CPL ? 1ull << (P & 63) : 0; } // P a multiple of 64
        MZ_LPROF(4); // legal mask
    }
    MZ_BPROF(ROLE, 3);
    if constexpr (SYNC) { __syncthreads(); }
    MZ_BPROF(ROLE, 4);
    if constexpr (kShared && ROLE == 1) {
        legalMask([](int i) { return (i & 1) == 1; });
        return;
    }
    // ---- terminal: Tromp-Taylor area score + komi (ref go.cpp:259-278,703-723) ----
    float eval = 0.0f;
    if (terminal) {
        waveSync();
        uint16_t* rl = lab; // region id of the empty points: the smallest point of the region
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            rl[p] = static_cast<uint16_t>(p);
            libs[p] = 0;
            gh[p] = 0;
        }
        waveSync();
        while (true) {
            bool changed = false;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                if (c[i] != 0) { continue; }
                const int p = i * 64 + lane;
                int mn = rl[p];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = nb[i][k];
                    if (q >= 0 && col[q] == 0 && rl[q] < mn) { mn = rl[q]; }
                }
                if (mn < rl[p]) { rl[p] = static_cast<uint16_t>(mn); changed = true; }
            }
            waveSync();
            if (__ballot(changed) == 0) { break; }
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (c[i] != 0) { continue; }
            const int p = i * 64 + lane, r = rl[p];
            atomicAdd(&libs[r], 1);
            unsigned long long border = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = nb[i][k];
                if (q >= 0 && (col[q] == 1 || col[q] == 2)) { border |= col[q]; }
            }
            if (border) { atomicOr(reinterpret_cast<unsigned long long*>(&gh[r]), border); }
        }
        waveSync();
        float t1 = 0.0f, t2 = 0.0f;
        for (int i = 0; i < W; ++i) { t1 += static_cast<float>(__popcll(cur[i])); t2 += static_cast<float>(__popcll(cur[W + i])); }
        t2 += v.komi;
#pragma unroll
        for (int i = 0; i < CPL; ++i) { // regions in ascending order of their first point, like the host's scan
            const int p = i * 64 + lane;
            uint64_t roots = __ballot(c[i] == 0 && rl[p] == p);
            while (roots) {
                const int r = i * 64 + __builtin_ctzll(roots);
                roots &= roots - 1;
                const uint64_t border = gh[r];
                const float size = static_cast<float>(libs[r]);
                if ((border & 2) == 0) { t1 += size; }
                else if ((border & 1) == 0) { t2 += size; }
            }
        }
        eval = t1 > t2 ? 1.0f : (t1 < t2 ? -1.0f : 0.0f);
    }
    if (lane == 0) {
        v.leaf_player[g] = t;
        v.terminal[g] = terminal ? 1 : 0;
        v.eval[g] = eval;
    }
}

// The planes of leafBody<CPL, true> (Go), shared by `nw` waves (the per-game simulation kernel: every wave takes the planes ch = w, w + nw, ...):
// planes 2k / 2k+1 = own / opponent stones k moves ago under the rotation, 16 / 17 = black / white to move (ref go.cpp:280-308).
// `smem` is the leaf's scratch block (its history words were filled by the leaf body), the player to move is read from v.leaf_player.
template <int CPL>
__device__ __forceinline__ void goPlanesPart(const GoDevView& v, int max_depth, int rot, int g, int w, int nw, int lane, const uint64_t* __restrict__ smem)
{
    const int P = v.P, W = v.W;
    const uint64_t* hb = smem + v.Ppad + max_depth + 4;
    const int t = v.leaf_player[g];
    const uint16_t* map = v.inv + size_t(rot) * P;
    uint32_t* out = v.feat + size_t(g) * 18 * v.W32;
    for (int ch = w; ch < 18; ch += nw) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int p = i * 64 + lane;
            uint64_t word;
            if (ch < 16) {
                const int q = p < P ? map[p] : 0;
                const int k = ch >> 1, color = (ch & 1) == 0 ? t - 1 : 2 - t;
                word = __ballot(p < P && ((hb[(k * 2 + color) * W + (q >> 6)] >> (q & 63)) & 1));
            } else {
                word = (ch == 16 ? t == 1 : t == 2) ? __ballot(p < P) : 0;
            }
            if (lane == 0) {
                if (2 * i < v.W32) { out[ch * v.W32 + 2 * i] = static_cast<uint32_t>(word); }
                if (2 * i + 1 < v.W32) { out[ch * v.W32 + 2 * i + 1] = static_cast<uint32_t>(word >> 32); }
            }
        }
    }
}

// ---- The frame of the two-bitboard leaf bodies (every game but Go).  A slot holds two bitboards of v.W words and two `meta` words; a leaf is its parent's slot
// plus the last action of the path.  A body is: leafPlace, loadSlot, the game's rules (at depth >= 1: the move, then storeSlot), its legal mask, its planes
// (storePlaneWord), storeLeafResult.  The boards stay in register arrays of a compile-time word count: every word index below is an unrolled constant.
struct LeafPlace {
    int len, depth;            // nodes on the path; the leaf's depth below the root (0: the leaf is the root)
    int t, m;                  // the player to move at the leaf; the player who moved into it (3 - t; depth >= 1)
    int src;                   // the slot the leaf's position starts from: its parent's (the root's slot 0 at depth 0)
    size_t sb;                 // the game's first slot
    const int* path;           // the path's nodes
    const int* pact;           // the action into each of them
    const int* hs;             // a node's slot
    const GoRootSnapshot& S;
    __device__ __forceinline__ int action() const { return pact[len - 1]; } // the action into the leaf (depth >= 1; read where it is used: not at a root)
};
__device__ __forceinline__ LeafPlace leafPlace(const GoDevView& v, const PoolView& pv, int g)
{
    const int len = pv.path_len[g], depth = len - 1;
    const int* path = pv.path + size_t(g) * pv.max_depth;
    const int* hs = pv.hslot + size_t(g) * pv.cap;
    const GoRootSnapshot& S = v.snap[g];
    const int t = (depth & 1) ? 3 - S.turn : S.turn;
    return {len, depth, t, 3 - t, depth == 0 ? 0 : hs[path[len - 2]], size_t(g) * v.slots, path, pv.path_action + size_t(g) * pv.max_depth, hs, S};
}

__device__ __forceinline__ unsigned long long hexUniform(unsigned long long x) // a value every lane holds, moved to scalar registers
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// slot L.src: the boards' words past v.W are 0.  UNIFORM: the words go to scalar registers
template <int NW, bool UNIFORM>
__device__ __forceinline__ void loadSlot(const GoDevView& v, const LeafPlace& L, unsigned long long (&b0)[NW], unsigned long long (&b1)[NW], int& meta0, int& meta1)
{
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const bool in = NW == 1 || i < v.W; // (a board has a word)
        const unsigned long long x0 = in ? v.stones[((L.sb + L.src) * 2 + 0) * v.W + i] : 0ull, x1 = in ? v.stones[((L.sb + L.src) * 2 + 1) * v.W + i] : 0ull;
        b0[i] = UNIFORM ? hexUniform(x0) : x0;
        b1[i] = UNIFORM ? hexUniform(x1) : x1;
    }
    meta0 = v.meta[(L.sb + L.src) * 2];
    meta1 = v.meta[(L.sb + L.src) * 2 + 1];
}

// the leaf's position into its own slot (lane 0 calls it).  META = false: the game keeps nothing in `meta`
template <int NW, bool META = true>
__device__ __forceinline__ void storeSlot(const GoDevView& v, const LeafPlace& L, int slot, const unsigned long long (&b0)[NW], const unsigned long long (&b1)[NW], int meta0, int meta1)
{
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (NW == 1 || i < v.W) {
            v.stones[((L.sb + slot) * 2 + 0) * v.W + i] = b0[i];
            v.stones[((L.sb + slot) * 2 + 1) * v.W + i] = b1[i];
        }
    }
    if (META) {
        v.meta[(L.sb + slot) * 2] = meta0;
        v.meta[(L.sb + slot) * 2 + 1] = meta1;
    }
}

// word i of a plane per lane: lane ch < planes holds plane ch's 64 bits and writes them as the plane's halves 2i and 2i + 1 (the last word may have one half only).
// `out` = leafPlanes(v, g, planes), taken once by the body: inside the loop over the words every word would compute it again
__device__ __forceinline__ uint32_t* leafPlanes(const GoDevView& v, int g, int planes) { return v.feat + size_t(g) * planes * v.W32; }
__device__ __forceinline__ void storePlaneWord(const GoDevView& v, uint32_t* out, int lane, int planes, int i, unsigned long long word)
{
    if (lane < planes) {
        if (2 * i < v.W32) { out[lane * v.W32 + 2 * i] = static_cast<uint32_t>(word); }
        if (2 * i + 1 < v.W32) { out[lane * v.W32 + 2 * i + 1] = static_cast<uint32_t>(word >> 32); }
    }
}
// word i of the four planes of Othello, TicTacToe, Gomoku and Hex: own, opponent, black to move, white to move (`ones`: the points of the word on the board)
__device__ __forceinline__ void storeToMovePlanes(const GoDevView& v, uint32_t* out, int lane, int t, int i, unsigned long long own, unsigned long long opp, unsigned long long ones)
{
    unsigned long long word = 0;
    if (lane == 0) { word = own; }
    if (lane == 1) { word = opp; }
    if (lane == 2) { word = t == 1 ? ones : 0; }
    if (lane == 3) { word = t == 2 ? ones : 0; }
    storePlaneWord(v, out, lane, 4, i, word);
}

// what the search reads of the leaf (lane 0 calls it)
__device__ __forceinline__ void storeLeafResult(const GoDevView& v, int g, int t, bool terminal, float eval)
{
    v.leaf_player[g] = t;
    v.terminal[g] = terminal ? 1 : 0;
    v.eval[g] = eval;
}
__device__ __forceinline__ float winnerEval(int winner) { return winner == 1 ? 1.0f : (winner == 2 ? -1.0f : 0.0f); } // black's point of view

// ---- Othello (ref environment/othello/othello.cpp:61-140,195-255): the whole position is two 64-bit boards, so every lane carries
// it and the rules are scalar bit arithmetic; only the rotated feature planes are built with ballots.  Slot layout: the `stones`
// words of the Go slab hold the two boards, `meta` (moves played, trailing passes).
struct OthMasks { unsigned long long full, not_left, not_right; int n; };
__device__ __forceinline__ unsigned long long othShift(const OthMasks& k, unsigned long long b, int d)
{
    switch (d) {
    case 0: return (b << k.n) & k.full;
    case 1: return b >> k.n;
    case 2: return (b & k.not_left) >> 1;
    case 3: return ((b & k.not_right) << 1) & k.full;
    case 4: return ((b & k.not_left) << (k.n - 1)) & k.full;
    case 5: return ((b & k.not_right) << (k.n + 1)) & k.full;
    case 6: return (b & k.not_right) >> (k.n - 1);
    default: return (b & k.not_left) >> (k.n + 1);
    }
}
__device__ __forceinline__ unsigned long long othMoves(const OthMasks& k, unsigned long long me, unsigned long long op)
{
    const unsigned long long empty = k.full & ~(me | op);
    unsigned long long m = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        unsigned long long x = othShift(k, me, d) & op;
        for (int i = 0; i < k.n - 3; ++i) { x |= othShift(k, x, d) & op; }
        m |= othShift(k, x, d) & empty;
    }
    return m;
}

__device__ __forceinline__ void othLeafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane)
{
    const int P = v.P, n = v.n;
    OthMasks k;
    k.n = n;
    k.full = P == 64 ? ~0ull : ((1ull << P) - 1);
    k.not_left = 0; k.not_right = 0;
    for (int y = 0; y < n; ++y) {
        const unsigned long long row = ((1ull << n) - 1) << (y * n);
        k.not_left |= row & ~(1ull << (y * n));
        k.not_right |= row & ~(1ull << (y * n + n - 1));
    }
    const LeafPlace L = leafPlace(v, pv, g);
    const int t = L.t;
    unsigned long long b[2][1]; // [black, white]
    int nmoves, passes;
    loadSlot<1, false>(v, L, b[0], b[1], nmoves, passes);
    if (L.depth >= 1) {
        const int a = L.action();
        ++nmoves;
        if (a >= P) {
            passes = passes + 1 > 2 ? 2 : passes + 1;
        } else {
            passes = 0;
            unsigned long long& me = b[L.m - 1][0];
            unsigned long long& op = b[2 - L.m][0];
            const unsigned long long placed = 1ull << a;
            unsigned long long flip = 0;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                unsigned long long line = 0, x = othShift(k, placed, d);
                for (int i = 0; i < n && (x & op); ++i) { line |= x; x = othShift(k, x, d); }
                if (x & me) { flip |= line; }
            }
            me |= placed | flip;
            op &= ~flip;
        }
        if (lane == 0) { storeSlot<1>(v, L, slot, b[0], b[1], nmoves, passes); }
    }
    const unsigned long long s[2] = {b[0][0], b[1][0]};
    const bool terminal = passes >= 2; // ref othello.cpp: two consecutive passes
    const unsigned long long mv = terminal ? 0ull : othMoves(k, s[t - 1], s[2 - t]);
    if (lane == 0) { // legal mask: the moves, or pass when there is none (ref othello.cpp:195-201)
        unsigned long long w0 = mv, w1 = 0;
        if (!terminal && mv == 0) { if (P < 64) { w0 |= 1ull << P; } else { w1 = 1ull; } }
        v.legal[size_t(g) * v.LW] = w0;
        if (v.LW > 1) { v.legal[size_t(g) * v.LW + 1] = w1; }
    }
    { // planes (ref othello.cpp:238-262): own, opponent, black to move, white to move — under the cycle's rotation
        const uint16_t* map = v.inv + size_t(rot) * P;
        const int q = lane < P ? map[lane] : 0;
        const unsigned long long own = __ballot(lane < P && ((s[t - 1] >> q) & 1)), opp = __ballot(lane < P && ((s[2 - t] >> q) & 1));
        storeToMovePlanes(v, leafPlanes(v, g, 4), lane, t, 0, own, opp, __ballot(lane < P));
    }
    float eval = 0.0f;
    if (terminal) { // ref othello.cpp:211-236: a winner only once neither side can move
        if (othMoves(k, s[0], s[1]) == 0 && othMoves(k, s[1], s[0]) == 0) {
            const int nb = __popcll(s[0]), nw = __popcll(s[1]);
            eval = nb > nw ? 1.0f : (nb < nw ? -1.0f : 0.0f);
        }
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, eval); }
}

// ---- TicTacToe (ref environment/tictactoe/tictactoe.cpp:19-97): two 9-bit boards per slot; the planes are Othello's (own, opponent,
// black to move, white to move); no pass, terminal = a complete line or a full board.
__device__ __forceinline__ void tttLeafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane)
{
    const int P = 9;
    const LeafPlace L = leafPlace(v, pv, g);
    const int t = L.t;
    unsigned long long b[2][1]; // [black, white]
    int unused0, unused1;       // (nothing is kept in `meta`)
    loadSlot<1, false>(v, L, b[0], b[1], unused0, unused1);
    if (L.depth >= 1) {
        b[L.m - 1][0] |= 1ull << L.action();
        if (lane == 0) { storeSlot<1, false>(v, L, slot, b[0], b[1], 0, 0); }
    }
    const unsigned s[2] = {static_cast<unsigned>(b[0][0]), static_cast<unsigned>(b[1][0])};
    int winner = 0;
    {
        const unsigned lines[8] = {0007, 0070, 0700, 0111, 0222, 0444, 0421, 0124};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (winner == 0 && (s[0] & lines[i]) == lines[i]) { winner = 1; }
            if (winner == 0 && (s[1] & lines[i]) == lines[i]) { winner = 2; }
        }
    }
    const bool terminal = winner != 0 || (s[0] | s[1]) == 0777u;
    if (lane == 0) { v.legal[size_t(g) * v.LW] = terminal ? 0ull : static_cast<unsigned long long>(~(s[0] | s[1]) & 0777u); }
    {
        const uint16_t* map = v.inv + size_t(rot) * P;
        const int q = lane < P ? map[lane] : 0;
        storeToMovePlanes(v, leafPlanes(v, g, 4), lane, t, 0, __ballot(lane < P && ((s[t - 1] >> q) & 1)), __ballot(lane < P && ((s[2 - t] >> q) & 1)), 0777ull);
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, winnerEval(winner)); }
}

// ---- Gomoku (ref environment/gomoku/gomoku.cpp:23-105,140-162): two bitboards of up to kGoMaxW words per slot, `meta` (moves played, the winner).  The
// position is wave-uniform (every lane carries the words; a lane picks the word of its own point with selects, never a dynamic register index).  The
// winner is decided by the move just played alone: lanes 0 .. 3 walk the four lines through its stone.  No pass: the legal mask is the empty points or,
// for the game's first move under outer-open, the outer two rings (gomoku.cpp:48-58) — like the host's, also at a terminal leaf.
__device__ __forceinline__ unsigned long long gmkWord(const unsigned long long (&b)[kGoMaxW], int w)
{
    unsigned long long x = b[0];
#pragma unroll
    for (int i = 1; i < kGoMaxW; ++i) { x = w == i ? b[i] : x; }
    return x;
}
__device__ __forceinline__ bool gmkStone(const unsigned long long (&b)[kGoMaxW], int p) { return (gmkWord(b, p >> 6) >> (p & 63)) & 1; }

__device__ __forceinline__ void gmkLeafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane)
{
    const int P = v.P, n = v.n, W = v.W;
    const LeafPlace L = leafPlace(v, pv, g);
    const int t = L.t, rule = L.S.ruleBits();
    unsigned long long blk[kGoMaxW], wht[kGoMaxW];
    int nmoves, winner;
    loadSlot<kGoMaxW, false>(v, L, blk, wht, nmoves, winner);
    if (L.depth >= 1) {
        const int a = L.action(), m = L.m;
        ++nmoves;
        unsigned long long mine[kGoMaxW];
#pragma unroll
        for (int i = 0; i < kGoMaxW; ++i) {
            const unsigned long long bit = i == (a >> 6) ? 1ull << (a & 63) : 0ull;
            if (m == 1) { blk[i] |= bit; } else { wht[i] |= bit; }
            mine[i] = m == 1 ? blk[i] : wht[i];
        }
        // line d of lanes 0 .. 3: (1, 0) row, (0, 1) column, (1, 1) and (1, -1) the diagonals; its length through `a` (a included)
        const int d = lane & 3, dx = d == 1 ? 0 : 1, dy = d == 0 ? 0 : (d == 3 ? -1 : 1);
        int run = 1;
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            int x = a % n + sgn * dx, y = a / n + sgn * dy;
            while (x >= 0 && x < n && y >= 0 && y < n && gmkStone(mine, y * n + x)) { ++run; x += sgn * dx; y += sgn * dy; }
        }
        const bool five = (rule & kGmkExactlyFive) ? run == 5 : run >= 5;
        winner = __ballot(lane < 4 && five) != 0 ? m : 0; // ref gomoku.cpp:29: the winner is replaced on every move
        if (lane == 0) { storeSlot<kGoMaxW>(v, L, slot, blk, wht, nmoves, winner); }
    }
    int stones = 0;
#pragma unroll
    for (int i = 0; i < kGoMaxW; ++i) { stones += __popcll(blk[i] | wht[i]); }
    const bool terminal = winner != 0 || stones == P; // ref gomoku.cpp:60-63
    const bool first_oo = (rule & kGmkOuterOpen) && nmoves == 0;
    const uint16_t* map = v.inv + size_t(rot) * P;
    uint32_t* out = leafPlanes(v, g, 4);
#pragma unroll
    for (int i = 0; i < kGoMaxW; ++i) {
        if (i >= W) { continue; }
        const int p = 64 * i + lane;
        bool leg = false;
        if (p < P) {
            if (first_oo) {
                const int r = p / n, c = p % n;
                leg = r < 2 || r >= n - 2 || c < 2 || c >= n - 2;
            } else {
                leg = !(((blk[i] | wht[i]) >> lane) & 1);
            }
        }
        const unsigned long long lw = __ballot(leg);
        if (lane == 0) { v.legal[size_t(g) * v.LW + i] = lw; }
        // planes (ref gomoku.cpp:75-98): own, opponent, black to move, white to move — under the cycle's rotation
        const int q = p < P ? map[p] : 0;
        const bool b = gmkStone(blk, q), w = gmkStone(wht, q);
        storeToMovePlanes(v, out, lane, t, i, __ballot(p < P && (t == 1 ? b : w)), __ballot(p < P && (t == 1 ? w : b)), __ballot(p < P));
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, winnerEval(winner)); } // ref gomoku.cpp:65-73
}

// ---- Hex (ref environment/hex/hex.cpp:22-141,307-362): the slot layout of Gomoku — two bitboards of up to kGoMaxW words, `meta` (actions played, the winner).
// Black (1) connects column 0 with column n - 1, White (2) row 0 with row n - 1; a point's neighbours are at -n-1, -n, -1, +1, +n, +n+1 (hex.cpp:319-336).  The
// position is wave-uniform, so the win test is a wave-uniform flood: the set reached from the new stone is dilated by the six shifts (multi-word shifts with
// column masks, every word index static), masked with the mover's stones, until a round adds nothing; then it is tested against the mover's two edge masks.
// NW = the words the board needs (2 up to 11x11, else kGoMaxW), so that the default board does not shift four empty words.
// bit p of a board: the word is gathered with masked ORs (not gmkWord's select chain, which the compiler turns into an indexed load from a scratch copy)
__device__ __forceinline__ bool hexStone(const unsigned long long (&b)[kGoMaxW], int p)
{
    unsigned long long x = 0;
#pragma unroll
    for (int i = 0; i < kGoMaxW; ++i) { x |= i == (p >> 6) ? b[i] : 0ull; }
    return (x >> (p & 63)) & 1;
}

template <int NW>
__device__ __forceinline__ bool hexConnects(const unsigned long long (&stones)[kGoMaxW], int p_in, int colour, int n, int P, int lane)
{
    const int p = __builtin_amdgcn_readfirstlane(p_in);
    unsigned long long mine[NW], ncl[NW], ncr[NW], e0[NW], e1[NW]; // the mover's stones; not column 0; not column n - 1; the mover's two edges
    bool on0 = false, on1 = false;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int q = 64 * i + lane, x = q % n;
        const bool in = q < P;
        mine[i] = hexUniform(stones[i]);
        ncl[i] = __ballot(in && x != 0);
        ncr[i] = __ballot(in && x != n - 1);
        e0[i] = __ballot(in && (colour == 1 ? x == 0 : q < n));          // hex.cpp:51-61
        e1[i] = __ballot(in && (colour == 1 ? x == n - 1 : q >= P - n));
        on0 |= (mine[i] & e0[i]) != 0;
        on1 |= (mine[i] & e1[i]) != 0;
    }
    if (!on0 || !on1) { return false; } // no stone of the mover on one of the edges: nothing to flood
    unsigned long long r[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) { r[i] = i == (p >> 6) ? 1ull << (p & 63) : 0ull; }
    const int s1 = n, s2 = n + 1; // (both below 64: n <= 19)
    for (int round = 0; round < P; ++round) {
        unsigned long long grow[NW], any = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const unsigned long long below = i > 0 ? r[i - 1] : 0ull, above = i + 1 < NW ? r[i + 1] : 0ull;
            const unsigned long long up1 = (r[i] << 1) | (below >> 63), dn1 = (r[i] >> 1) | (above << 63);
            const unsigned long long upn = (r[i] << s1) | (below >> (64 - s1)), dnn = (r[i] >> s1) | (above << (64 - s1));
            const unsigned long long upd = (r[i] << s2) | (below >> (64 - s2)), dnd = (r[i] >> s2) | (above << (64 - s2));
            grow[i] = (((up1 | upd) & ncl[i]) | ((dn1 | dnd) & ncr[i]) | upn | dnn) & mine[i] & ~r[i];
            any |= grow[i];
        }
        if (any == 0) { break; }
#pragma unroll
        for (int i = 0; i < NW; ++i) { r[i] |= grow[i]; }
    }
    bool at0 = false, at1 = false;
#pragma unroll
    for (int i = 0; i < NW; ++i) { at0 |= (r[i] & e0[i]) != 0; at1 |= (r[i] & e1[i]) != 0; }
    return at0 && at1;
}

__device__ __forceinline__ void hexLeafBody(const GoDevView& v, const PoolView& pv, int /*rot: Hex has no symmetries, hex.cpp:128*/, int slot, int g, int lane)
{
    const int P = v.P, n = v.n, W = v.W;
    const LeafPlace L = leafPlace(v, pv, g);
    const int t = L.t, rule = L.S.ruleBits();
    unsigned long long blk[kGoMaxW], wht[kGoMaxW];
    int nact, winner;
    loadSlot<kGoMaxW, false>(v, L, blk, wht, nact, winner);
    if (L.depth >= 1) {
        const int a = L.action(), m = L.m;
        // the swap (hex.cpp:28-47), recognised from the position alone: rule on, one action played, the chosen cell occupied — the stone there goes, the mover's
        // lands on its reflection (row, col) -> (n - 1 - col, n - 1 - row)
        const bool swap = (rule & kHexSwap) && nact == 1 && (hexStone(blk, a) || hexStone(wht, a));
        const int p = swap ? (n - 1 - a % n) * n + (n - 1 - a / n) : a;
        ++nact;
        unsigned long long mine[kGoMaxW];
#pragma unroll
        for (int i = 0; i < kGoMaxW; ++i) {
            const unsigned long long gone = (swap && i == (a >> 6)) ? 1ull << (a & 63) : 0ull;
            const unsigned long long bit = i == (p >> 6) ? 1ull << (p & 63) : 0ull;
            blk[i] &= ~gone;
            wht[i] &= ~gone;
            if (m == 1) { blk[i] |= bit; } else { wht[i] |= bit; }
            mine[i] = m == 1 ? blk[i] : wht[i];
        }
        if (winner == 0) { // a winner never goes away (and the flood is skipped)
            const bool won = W <= 2 ? hexConnects<2>(mine, p, m, n, P, lane) : hexConnects<kGoMaxW>(mine, p, m, n, P, lane);
            if (won) { winner = m; }
        }
        if (lane == 0) { storeSlot<kGoMaxW>(v, L, slot, blk, wht, nact, winner); }
    }
    const bool terminal = winner != 0; // ref hex.cpp:101-104: there is no draw
    const bool any_cell = (rule & kHexSwap) && nact == 1; // hex.cpp:97: every cell is legal on the second action
    uint32_t* out = leafPlanes(v, g, 4);
#pragma unroll
    for (int i = 0; i < kGoMaxW; ++i) {
        if (i >= W) { continue; }
        const int p = 64 * i + lane;
        const bool b = (blk[i] >> lane) & 1, w = (wht[i] >> lane) & 1;
        const unsigned long long lw = __ballot(p < P && (any_cell || !(b || w)));
        if (lane == 0) { v.legal[size_t(g) * v.LW + i] = lw; }
        // planes (ref hex.cpp:118-141): own, opponent, black to move, white to move
        storeToMovePlanes(v, out, lane, t, i, __ballot(p < P && (t == 1 ? b : w)), __ballot(p < P && (t == 1 ? w : b)), __ballot(p < P));
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, winnerEval(winner)); } // ref hex.cpp:106-116
}

// ---- NoGo (ref nogo.h:25-76; a rules variant of Go, game_kind.h kNoGo): boards up to 9x9, so a position is two bitboards of two words, and the slot layout is
// Gomoku's — the `stones` words, `meta` (moves played, unused).  Nothing is ever captured: the leaf is its parent's stones plus one, and the position k moves
// before the leaf is the slot of the k-th ancestor (older than the root: the root's ring), as in Go.  The legal mask needs the liberties of whole blocks and no
// block ids: every lane that holds a stone floods its OWN block — dilate by the four shifts, mask with the colour's stones, until no lane's block grows — and
// counts popc(dilate(block) & empty).  A ballot of the enemy stones whose block has one liberty, dilated onto the empty points, is the set of capturing moves
// (an empty point next to such a stone IS that liberty); a ballot of the own stones whose block has two or more, dilated, together with dilate(empty), is the
// set of moves that are no suicide.  Terminal <=> the mask is empty; the result is the player not to move.
struct NoGoMasks { unsigned long long full[2], ncl[2], ncr[2]; int n; }; // on the board; not column 0; not column n - 1
__device__ __forceinline__ void nogoDilate(const NoGoMasks& k, const unsigned long long (&b)[2], unsigned long long (&out)[2])
{
    const int n = k.n; // 2 <= n <= 9: every shift count below is in 1 .. 63
    const unsigned long long up1[2] = {b[0] << 1, (b[1] << 1) | (b[0] >> 63)}, dn1[2] = {(b[0] >> 1) | (b[1] << 63), b[1] >> 1};
    const unsigned long long upn[2] = {b[0] << n, (b[1] << n) | (b[0] >> (64 - n))}, dnn[2] = {(b[0] >> n) | (b[1] << (64 - n)), b[1] >> n};
#pragma unroll
    for (int i = 0; i < 2; ++i) { out[i] = ((up1[i] & k.ncl[i]) | (dn1[i] & k.ncr[i]) | upn[i] | dnn[i]) & k.full[i]; }
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    const unsigned lo = __shfl(static_cast<unsigned>(v), src), hi = __shfl(static_cast<unsigned>(v >> 32), src);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ void nogoLeafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane)
{
    const int P = v.P, n = v.n, W = v.W; // W <= 2 (GoDevice::init: boards up to gameMaxBoard(kNoGo))
    const LeafPlace L = leafPlace(v, pv, g);
    const GoRootSnapshot& S = L.S;
    const int t = L.t, depth = L.depth, len = L.len, root_hist_len = S.hist_len;
    const size_t sb = L.sb;
    const int *path = L.path, *hs = L.hs;
    unsigned long long st[2][2]; // [colour][word]
    int nmoves, unused;          // (the second `meta` word is written 0 and never read)
    loadSlot<2, true>(v, L, st[0], st[1], nmoves, unused);
    if (depth >= 1) { // GoEnv::act of a move that captures nothing (ref go.cpp:132-190): the stone is placed
        const int a = L.action(), m = L.m;
        ++nmoves;
#pragma unroll
        for (int i = 0; i < 2; ++i) { // (selects, never a dynamic register index)
            const unsigned long long bit = (a < P && i == (a >> 6)) ? 1ull << (a & 63) : 0ull;
            st[0][i] |= m == 1 ? bit : 0ull;
            st[1][i] |= m == 2 ? bit : 0ull;
        }
        if (lane == 0) { storeSlot<2>(v, L, slot, st[0], st[1], nmoves, 0); }
    }
    NoGoMasks k;
    k.n = n;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = 64 * i + lane, x = p % n;
        k.full[i] = __ballot(p < P);
        k.ncl[i] = __ballot(p < P && x != 0);
        k.ncr[i] = __ballot(p < P && x != n - 1);
    }
    const unsigned long long empty[2] = {k.full[0] & ~(st[0][0] | st[1][0]), k.full[1] & ~(st[0][1] | st[1][1])};
    // ---- the block of the lane's stone in each word (point 64 * i + lane), flooded; safe[i] / atari[i]: the stones of player t whose block has >= 2 liberties,
    // the stones of the other player whose block has exactly one
    unsigned long long safe[2] = {0, 0}, atari[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (i >= W) { continue; }
        const bool isb = (st[0][i] >> lane) & 1, isw = (st[1][i] >> lane) & 1, has = isb || isw;
        const unsigned long long mine[2] = {isb ? st[0][0] : st[1][0], isb ? st[0][1] : st[1][1]}; // the stones of the lane's colour
        unsigned long long blk[2] = {(has && i == 0) ? 1ull << lane : 0ull, (has && i == 1) ? 1ull << lane : 0ull}, d[2];
        for (int round = 0; round < P; ++round) { // (a block's diameter is below P: the bound is never what ends the loop)
            nogoDilate(k, blk, d);
            const unsigned long long g0 = d[0] & mine[0] & ~blk[0], g1 = d[1] & mine[1] & ~blk[1];
            blk[0] |= g0; blk[1] |= g1;
            if (__ballot((g0 | g1) != 0) == 0) { break; }
        }
        nogoDilate(k, blk, d);
        const int libs = __popcll(d[0] & empty[0]) + __popcll(d[1] & empty[1]);
        const int colour = isb ? 1 : 2;
        safe[i] = __ballot(has && colour == t && libs >= 2);
        atari[i] = __ballot(has && colour != t && libs == 1);
    }
    unsigned long long dsafe[2], datari[2], dempty[2];
    nogoDilate(k, safe, dsafe);
    nogoDilate(k, atari, datari);
    nogoDilate(k, empty, dempty);
    const unsigned long long legal[2] = {empty[0] & (dempty[0] | dsafe[0]) & ~datari[0], empty[1] & (dempty[1] | dsafe[1]) & ~datari[1]};
    const bool terminal = (legal[0] | legal[1]) == 0; // ref nogo.h:59-66
    if (lane == 0) { // (the pass slot, bit P, is never legal: nogo.h:30)
        v.legal[size_t(g) * v.LW] = legal[0];
        if (v.LW > 1) { v.legal[size_t(g) * v.LW + 1] = legal[1]; }
    }
    // ---- planes (ref go.cpp:280-308): 2k / 2k+1 = own / opponent stones k moves before the leaf under the rotation, 16 / 17 = black / white to move.  Lane j < 16 * W
    // holds word j of the history block [8][2][W]; a point's bit is fetched from the lane of its word
    {
        const int avail = root_hist_len + depth;
        uint64_t hw = 0;
        if (lane < 16 * W) {
            const int kk = lane / (2 * W), cw = lane % (2 * W);
            if (kk < avail) {
                if (kk == 0) { hw = cw / W == 0 ? (cw % W == 0 ? st[0][0] : st[0][1]) : (cw % W == 0 ? st[1][0] : st[1][1]); }
                else if (kk < depth) { hw = v.stones[(sb + hs[path[len - 1 - kk]]) * 2 * W + cw]; }
                else { hw = S.hist[(root_hist_len - 1 - (kk - depth)) & 7][cw / W][cw % W]; }
            }
        }
        const uint16_t* map = v.inv + size_t(rot) * P;
        uint32_t* out = leafPlanes(v, g, 18);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= W) { continue; }
            const int p = 64 * i + lane;
            const int q = p < P ? map[p] : 0;
            uint64_t mine = 0; // lane ch keeps plane ch's word
            for (int ch = 0; ch < 16; ++ch) {
                const int kk = ch >> 1, colour = (ch & 1) == 0 ? t - 1 : 2 - t;
                const uint64_t word = shfl64(hw, (kk * 2 + colour) * W + (q >> 6));
                const uint64_t bal = __ballot(p < P && ((word >> (q & 63)) & 1));
                if (lane == ch) { mine = bal; }
            }
            if (lane == 16) { mine = t == 1 ? k.full[i] : 0; }
            if (lane == 17) { mine = t == 2 ? k.full[i] : 0; }
            storePlaneWord(v, out, lane, 18, i, mine);
        }
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, t == 2 ? 1.0f : -1.0f); } // ref nogo.h:68-76: the player not to move
}

// ---- Havannah (ref havannah.cpp:38-231,272-496; a game past the rows, game_kind.h kHavannah): the view's board is the E x E array (E = 2N - 1 for edge
// size N, game_kind.h networkBoard), cell (r, c) = id r * E + c is on the board iff N - 1 <= r + c <= 3N - 3, a cell's neighbours are at -E, -E+1, -1, +1,
// +E-1, +E (havannah.cpp:301-303).  The slot layout is Gomoku's: the two FEATURE bitboards as the reference keeps them — after a swap the cell is in both,
// havannah.cpp:147 only sets — and `meta` (actions played, the winner); a cell's owner is black = fb[0] & ~fb[1], white = fb[1], so a swap is nothing but
// White's bit on an occupied cell.  History planes as in NoGo: the position k actions before the leaf is the slot of the k-th ancestor, older ones are in the
// root's ring.  The position is wave-uniform, so every set below is a bitboard of NW scalar words (1, 2, 4 or kGoMaxW as the array needs; word indices static):
//   group   = flood of the mover's cells from the new stone by six-shift dilation to a fixpoint;
//   bridge  = the group holds two of the six corners, fork = it meets three of the six sides (masks by ballot from the lane's (r, c); havannah.cpp:64-86);
//   ring    = >= 6 cells, the new stone has >= 2 own neighbours, and either a neighbour of the new stone has six own neighbours (six shifted ANDs) or the
//             complement of the group, flooded inside the array from the array's rim, leaves a cell out (detectHole, havannah.cpp:407-496: its bounding
//             box plus frame is this flood restricted to where it can matter — DESIGN.md §3.13).  Most leaves fail a gate and never flood the complement.
template <int NW>
struct HavGeo {
    unsigned long long full[NW], ncl[NW], ncr[NW], board[NW]; // in the array; not column 0; not column E - 1; on the board
    int r[NW], c[NW];                                         // the lane's cell 64 * i + lane
    int E, N, lane;
};

// the six neighbour terms of a set: any[i] = cells with a neighbour in b (the dilation), all[i] = cells whose six neighbours are all in b
template <int NW>
__device__ __forceinline__ void havTerms(const HavGeo<NW>& k, const unsigned long long (&b)[NW], unsigned long long (&any)[NW], unsigned long long (&all)[NW])
{
    const int s1 = k.E, sm = k.E - 1; // 6 <= sm < s1 <= 19: every shift count below is in 1 .. 63
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const unsigned long long below = i > 0 ? b[i - 1] : 0ull, above = i + 1 < NW ? b[i + 1] : 0ull;
        const unsigned long long a1 = ((b[i] << 1) | (below >> 63)) & k.ncl[i];          // bit x = b[x - 1]:     (r, c - 1)
        const unsigned long long a2 = ((b[i] >> 1) | (above << 63)) & k.ncr[i];          // bit x = b[x + 1]:     (r, c + 1)
        const unsigned long long a3 = (b[i] << s1) | (below >> (64 - s1));               // bit x = b[x - E]:     (r - 1, c)
        const unsigned long long a4 = (b[i] >> s1) | (above << (64 - s1));               // bit x = b[x + E]:     (r + 1, c)
        const unsigned long long a5 = ((b[i] << sm) | (below >> (64 - sm))) & k.ncr[i];  // bit x = b[x - E + 1]: (r - 1, c + 1)
        const unsigned long long a6 = ((b[i] >> sm) | (above << (64 - sm))) & k.ncl[i];  // bit x = b[x + E - 1]: (r + 1, c - 1)
        any[i] = (a1 | a2 | a3 | a4 | a5 | a6) & k.full[i];
        all[i] = a1 & a2 & a3 & a4 & a5 & a6 & k.full[i];
    }
}

// `seed`, grown through `through` to a fixpoint (seed must lie in `through`)
template <int NW>
__device__ __forceinline__ void havFlood(const HavGeo<NW>& k, const unsigned long long (&through)[NW], unsigned long long (&r)[NW])
{
    for (int round = 0; round < k.E * k.E; ++round) { // (a set's diameter is below the cell count: the bound is never what ends the loop)
        unsigned long long d[NW], all[NW], grown = 0;
        havTerms<NW>(k, r, d, all);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const unsigned long long grow = d[i] & through[i] & ~r[i];
            r[i] |= grow;
            grown |= grow;
        }
        if (grown == 0) { break; }
    }
}

// has the mover, whose cells are `mine`, won with the stone at `a`?  (updateWinner, havannah.cpp:272-291)
template <int NW>
__device__ __forceinline__ bool havWins(const HavGeo<NW>& k, const unsigned long long (&mine)[NW], int a)
{
    const int E = k.E, N = k.N;
    unsigned long long one[NW], grp[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) { one[i] = i == (a >> 6) ? 1ull << (a & 63) : 0ull; grp[i] = one[i]; }
    havFlood<NW>(k, mine, grp);
    int corners = 0, size = 0;
    unsigned sides = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int r = k.r[i], c = k.c[i], s = r + c;
        const bool e0 = r == 0, e1 = s == N - 1, e2 = c == 0, e3 = r == E - 1, e4 = s == 3 * N - 3, e5 = c == E - 1; // the six edge lines of the hexagon
        const int lines = int(e0) + int(e1) + int(e2) + int(e3) + int(e4) + int(e5);
        const bool onb = (k.board[i] >> k.lane) & 1;
        corners += __popcll(grp[i] & __ballot(onb && lines == 2)); // a corner lies on two lines (havannah.cpp:79-85), a side cell on one (havannah.cpp:64-76)
        sides |= (grp[i] & __ballot(onb && lines == 1 && e0)) != 0 ? 1u : 0u;
        sides |= (grp[i] & __ballot(onb && lines == 1 && e1)) != 0 ? 2u : 0u;
        sides |= (grp[i] & __ballot(onb && lines == 1 && e2)) != 0 ? 4u : 0u;
        sides |= (grp[i] & __ballot(onb && lines == 1 && e3)) != 0 ? 8u : 0u;
        sides |= (grp[i] & __ballot(onb && lines == 1 && e4)) != 0 ? 16u : 0u;
        sides |= (grp[i] & __ballot(onb && lines == 1 && e5)) != 0 ? 32u : 0u;
        size += __popcll(grp[i]);
    }
    if (corners >= 2 || __popc(sides) >= 3) { return true; } // bridge, fork
    // ring (isCycle, havannah.cpp:377-395): the two gates, the shortcut, then the flood of the complement
    if (size < 6) { return false; }
    unsigned long long near[NW], inner[NW], unused[NW];
    havTerms<NW>(k, one, near, unused);  // the neighbours of the new stone
    havTerms<NW>(k, mine, unused, inner); // the cells with six own neighbours (of any colour, empty or not: havannah.cpp:388-391)
    int own = 0;
    unsigned long long blob = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { own += __popcll(near[i] & mine[i]); blob |= near[i] & inner[i]; }
    if (own < 2) { return false; }
    if (blob != 0) { return true; }
    unsigned long long bg[NW], reach[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const bool in = (k.full[i] >> k.lane) & 1;
        bg[i] = k.full[i] & ~grp[i];
        reach[i] = bg[i] & __ballot(in && (k.r[i] == 0 || k.c[i] == 0 || k.r[i] == E - 1 || k.c[i] == E - 1));
    }
    havFlood<NW>(k, bg, reach);
    unsigned long long hole = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { hole |= bg[i] & ~reach[i]; }
    return hole != 0;
}

template <int NW>
__device__ __forceinline__ void havLeafBodyT(const GoDevView& v, const PoolView& pv, int slot, int g, int lane)
{
    const int P = v.P, E = v.n, W = v.W; // W <= NW
    const LeafPlace L = leafPlace(v, pv, g);
    const GoRootSnapshot& S = L.S;
    const int t = L.t, depth = L.depth, len = L.len, root_hist_len = S.hist_len;
    const bool rule = (S.hash & kHavSwap) != 0;
    const size_t sb = L.sb;
    const int *path = L.path, *hs = L.hs;
    unsigned long long fb[2][NW]; // [black, white][word]: the feature bitboards
    int nact, winner;
    loadSlot<NW, true>(v, L, fb[0], fb[1], nact, winner);
    nact = __builtin_amdgcn_readfirstlane(nact);
    winner = __builtin_amdgcn_readfirstlane(winner);
    HavGeo<NW> k;
    k.E = E;
    k.N = (E + 1) / 2;
    k.lane = lane;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int q = 64 * i + lane, r = q / E, c = q - r * E;
        const bool in = q < P;
        k.r[i] = r;
        k.c[i] = c;
        k.full[i] = __ballot(in);
        k.ncl[i] = __ballot(in && c != 0);
        k.ncr[i] = __ballot(in && c != E - 1);
        k.board[i] = __ballot(in && r + c >= k.N - 1 && r + c <= 3 * k.N - 3); // havannah.cpp:321-327
    }
    if (depth >= 1) { // havannah.cpp:107-151
        const int a = __builtin_amdgcn_readfirstlane(L.action()), m = L.m;
        ++nact;
        unsigned long long mine[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) { // (selects, never a dynamic register index)
            const unsigned long long bit = i == (a >> 6) ? 1ull << (a & 63) : 0ull;
            fb[0][i] |= m == 1 ? bit : 0ull;
            fb[1][i] |= m == 2 ? bit : 0ull; // on the occupied cell, on the second action: the swap — the cell is White's from here on
            mine[i] = m == 1 ? fb[0][i] & ~fb[1][i] : fb[1][i];
        }
        if (winner == 0 && havWins<NW>(k, mine, a)) { winner = m; } // a winner never goes away (and the floods are skipped)
        if (lane == 0) { storeSlot<NW>(v, L, slot, fb[0], fb[1], nact, winner); }
    }
    int stones = 0, cells = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { stones += __popcll(fb[0][i] | fb[1][i]); cells += __popcll(k.board[i]); }
    const bool terminal = winner != 0 || stones == cells; // ref havannah.cpp:179-184: a full board is a draw
    const bool swappable = rule && nact == 1;             // havannah.cpp:174-176: every cell of the board is legal on the second action
    // planes (ref havannah.cpp:196-231): lane ch < 16 holds plane ch = own / opponent feature bitboard ch / 2 actions before the leaf (no rotation: the maps are
    // the identity, so a plane's word is the history word itself), lanes 16 .. 19 the board, swappable, black to move, white to move
    const int avail = root_hist_len + depth;
    const int kk = lane >> 1, colour = (lane & 1) == 0 ? t - 1 : 2 - t;
    uint32_t* out = leafPlanes(v, g, 20);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (i >= W) { continue; }
        if (lane == 0) { v.legal[size_t(g) * v.LW + i] = swappable ? k.board[i] : k.board[i] & ~(fb[0][i] | fb[1][i]); }
        unsigned long long word = 0;
        if (lane < 16) {
            if (kk < avail) {
                if (kk == 0) { word = colour == 0 ? fb[0][i] : fb[1][i]; }
                else if (kk < depth) { word = v.stones[((sb + hs[path[len - 1 - kk]]) * 2 + colour) * W + i]; }
                else { word = S.hist[(root_hist_len - 1 - (kk - depth)) & 7][colour][i]; }
            }
        }
        if (lane == 16) { word = k.board[i]; }
        if (lane == 17) { word = swappable ? k.full[i] : 0ull; }
        if (lane == 18) { word = t == 1 ? k.full[i] : 0ull; }
        if (lane == 19) { word = t == 2 ? k.full[i] : 0ull; }
        storePlaneWord(v, out, lane, 20, i, word);
    }
    if (lane == 0) { storeLeafResult(v, g, t, terminal, winnerEval(winner)); } // ref havannah.cpp:186-194
}

__device__ __forceinline__ void havLeafBody(const GoDevView& v, const PoolView& pv, int /*rot: no symmetries, havannah.h:71*/, int slot, int g, int lane)
{
    // NW = the words the array needs: 1 for N = 4 (7x7), 2 up to N = 6, 4 for the default N = 8 (15x15), kGoMaxW up to N = 10 (19x19)
    if (v.W <= 1) { havLeafBodyT<1>(v, pv, slot, g, lane); }
    else if (v.W <= 2) { havLeafBodyT<2>(v, pv, slot, g, lane); }
    else if (v.W <= 4) { havLeafBodyT<4>(v, pv, slot, g, lane); }
    else { havLeafBodyT<kGoMaxW>(v, pv, slot, g, lane); }
}

// leafBody<CPL> of the two-bitboard games (the template arguments behind CPL, `smem` and `seen_lds` are Go's: unused here)
template <int CPL, bool EXT_PLANES = false, int PART = 0, bool SYNC = false, int ROLE = 0, std::enable_if_t<(CPL <= 0), int> = 0>
__device__ __forceinline__ void leafBody(const GoDevView& v, const PoolView& pv, int rot, int slot, int g, int lane, uint64_t* = nullptr, const uint64_t* = nullptr)
{
    static_assert(CPL == kRulesTicTacToe || CPL == kRulesOthello || CPL == kRulesGomoku || CPL == kRulesHex || CPL == kRulesNoGo || CPL == kRulesHavannah, "no leaf body for this rules argument");
    if constexpr (CPL == kRulesTicTacToe) { tttLeafBody(v, pv, rot, slot, g, lane); }
    else if constexpr (CPL == kRulesOthello) { othLeafBody(v, pv, rot, slot, g, lane); }
    else if constexpr (CPL == kRulesGomoku) { gmkLeafBody(v, pv, rot, slot, g, lane); }
    else if constexpr (CPL == kRulesNoGo) { nogoLeafBody(v, pv, rot, slot, g, lane); }
    else if constexpr (CPL == kRulesHavannah) { havLeafBody(v, pv, rot, slot, g, lane); }
    else { hexLeafBody(v, pv, rot, slot, g, lane); }
}

// order `k` candidates in cs[] like the reference's std::sort(policy descending): result in out[]
__device__ void orderCandidates(Cand* cs, Cand* out, int* stack, int k, int lane, int* err)
{
    bool tie = false;
    for (int i = lane; i < k; i += 64) {
        const float pi = cs[i].policy;
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            const float pj = cs[j].policy;
            rank += (pj > pi) || (pj == pi && j < i);
            tie |= (pj == pi && j != i);
        }
        out[rank] = cs[i];
    }
    waveSync();
    if (k > 16 && __ballot(tie) != 0) { // ties among > 16 elements: only the exact introsort gives the reference's order
        if (lane == 0) {
            StdSortEmul<Cand, CandGreater> s{cs, CandGreater()};
            if (!s.sort(k, stack) && err) { atomicExch(err, MZ_ERR_CAPACITY); }
        }
        waveSync();
        for (int i = lane; i < k; i += 64) { out[i] = cs[i]; }
        waveSync();
    }
}

// The same order computed by ALL waves of a workgroup (the per-game simulation kernel: 7 of its 8 waves idle while wave 0 runs the tree
// phases, and the rank sort is VALU-bound: k^2 comparisons — 3.7 of the 8.5 us of candidates + expand + backup at 82 candidates).
//   candDense   (one wave)   policies of cs[0..k) into a dense float array `dense` [128], padding below every softmax output
//   candRankPart(every wave) wave w of nw counts, for each candidate i, the candidates j of ITS share of j that rank before i / tie with i
//   candScatter (one wave)   sums the partial counts, writes out[rank] = cs[i]; ties among > 16 candidates -> the exact introsort replay
// Workgroup barriers between the three steps are the caller's.  k <= 128.
constexpr int kCandCoopMax = 128;
__device__ __forceinline__ void candDense(const Cand* cs, int k, int lane, float* dense)
{
    dense[lane] = lane < k ? cs[lane].policy : -3.402823466e+38f;
    dense[64 + lane] = 64 + lane < k ? cs[64 + lane].policy : -3.402823466e+38f;
}
__device__ __forceinline__ void candRankPart(const float* dense, int k, int w, int nw, int lane, int* part /* [nw][4][64] */)
{
    const float p0 = dense[lane], p1 = dense[64 + lane];
    const int groups = (k + 3) >> 2, per = (32 + nw - 1) / nw;
    int r0 = 0, r1 = 0, e0 = 0, e1 = 0;
    for (int q = w * per; q < (w + 1) * per && q < groups; ++q) {
        const float4 d = reinterpret_cast<const float4*>(dense)[q];
        const float dj[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * q + e;
            r0 += (dj[e] > p0) || (dj[e] == p0 && j < lane);
            r1 += (dj[e] > p1) || (dj[e] == p1 && j < 64 + lane);
            e0 += (dj[e] == p0);
            e1 += (dj[e] == p1);
        }
    }
    int* mine = part + w * 256;
    mine[lane] = r0; mine[64 + lane] = r1; mine[128 + lane] = e0; mine[192 + lane] = e1;
}
__device__ __forceinline__ void candScatter(Cand* cs, Cand* out, int* stack, int k, int nw, int lane, const int* part, int* err)
{
    int r0 = 0, r1 = 0, e0 = 0, e1 = 0;
    for (int w = 0; w < nw; ++w) { const int* p = part + w * 256; r0 += p[lane]; r1 += p[64 + lane]; e0 += p[128 + lane]; e1 += p[192 + lane]; }
    const bool has0 = lane < k, has1 = 64 + lane < k;
    const bool tie = (has0 && e0 > 1) || (has1 && e1 > 1); // every candidate equals itself once
    if (has0) { out[r0] = cs[lane]; }
    if (has1) { out[r1] = cs[64 + lane]; }
    waveSync();
    if (k > 16 && __ballot(tie) != 0) { // ties among > 16 elements: only the exact introsort gives the reference's order
        if (lane == 0) {
            StdSortEmul<Cand, CandGreater> s{cs, CandGreater()};
            if (!s.sort(k, stack) && err) { atomicExch(err, MZ_ERR_CAPACITY); }
        }
        waveSync();
        for (int i = lane; i < k; i += 64) { out[i] = cs[i]; }
        waveSync();
    }
}

// ... and for boards of more than 128 actions (13x13 / 19x19 Go: up to 362 candidates, whose rank sort on ONE wave is k^2 / 64 = 2 000 dependent LDS reads
// per lane): the same three steps with up to six candidates per lane.  dense [384] floats, part [nw][2][384] counts.  k <= 384.
constexpr int kCandCoopMaxW = 384;
__device__ __forceinline__ void candDenseW(const Cand* cs, int k, int lane, float* dense)
{
#pragma unroll
    for (int c = 0; c < kCandCoopMaxW / 64; ++c) { const int i = 64 * c + lane; dense[i] = i < k ? cs[i].policy : -3.402823466e+38f; }
}
__device__ __forceinline__ void candRankPartW(const float* dense, int k, int w, int nw, int lane, int* part /* [nw][2][384] */)
{
    constexpr int NC = kCandCoopMaxW / 64;
    float p[NC];
    int r[NC], eq[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { p[c] = dense[64 * c + lane]; r[c] = 0; eq[c] = 0; }
    const int groups = (k + 3) >> 2, per = (groups + nw - 1) / nw;
    for (int q = w * per; q < (w + 1) * per && q < groups; ++q) {
        const float4 d = reinterpret_cast<const float4*>(dense)[q];
        const float dj[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = 4 * q + e;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                r[c] += (dj[e] > p[c]) || (dj[e] == p[c] && j < 64 * c + lane);
                eq[c] += (dj[e] == p[c]);
            }
        }
    }
    int* mine = part + w * 2 * kCandCoopMaxW;
#pragma unroll
    for (int c = 0; c < NC; ++c) { mine[64 * c + lane] = r[c]; mine[kCandCoopMaxW + 64 * c + lane] = eq[c]; }
}
__device__ __forceinline__ void candScatterW(Cand* cs, Cand* out, int* stack, int k, int nw, int lane, const int* part, int* err)
{
    constexpr int NC = kCandCoopMaxW / 64;
    bool tie = false;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int i = 64 * c + lane;
        int r = 0, e = 0;
        for (int w = 0; w < nw; ++w) { const int* p = part + w * 2 * kCandCoopMaxW; r += p[i]; e += p[kCandCoopMaxW + i]; }
        if (i < k) { out[r] = cs[i]; tie = tie || e > 1; } // every candidate equals itself once
    }
    waveSync();
    if (k > 16 && __ballot(tie) != 0) { // ties among > 16 elements: only the exact introsort gives the reference's order
        if (lane == 0) {
            StdSortEmul<Cand, CandGreater> s{cs, CandGreater()};
            if (!s.sort(k, stack) && err) { atomicExch(err, MZ_ERR_CAPACITY); }
        }
        waveSync();
        for (int i = lane; i < k; i += 64) { out[i] = cs[i]; }
        waveSync();
    }
}

// AlphaZero candidates of a leaf (ref zero_actor.cpp:215-245): legal actions in action order, policy / logit looked up through
// the rotation, sorted by policy; a terminal leaf has no children and its value is the game result (zero_actor.cpp:85)
// step 1: the legal actions of the leaf, in action order, into cs[]; returns their number (0 at a terminal leaf)
__device__ __forceinline__ int azCandGather(const GoDevView& v, const float* __restrict__ policy, const float* __restrict__ logit, int rot, int g, int lane,
                                            Cand* __restrict__ cs)
{
    const int A = v.A;
    int k = 0;
    if (v.terminal[g] != 0) { return 0; }
    const uint16_t* fwd = v.fwd + size_t(rot) * A;
    for (int base = 0; base < A; base += 64) {
        const int a = base + lane;
        const bool leg = a < A && ((v.legal[size_t(g) * v.LW + (a >> 6)] >> (a & 63)) & 1);
        const uint64_t m = __ballot(leg);
        if (leg) {
            const int pos = k + __popcll(m & ((1ull << lane) - 1));
            const int f = fwd[a];
            cs[pos] = Cand{a, policy[size_t(g) * A + f], logit[size_t(g) * A + f]};
        }
        k += __popcll(m);
    }
    return k;
}
// step 3: the sorted candidates and the leaf's scalars where expand + backup read them
__device__ __forceinline__ void azCandStore(const GoDevView& v, const float* __restrict__ value, const Cand* __restrict__ out, int k, int* __restrict__ cand_count,
                                            int* __restrict__ cand_action, float* __restrict__ cand_policy, float* __restrict__ cand_logit,
                                            int* __restrict__ cand_player, float* __restrict__ value_out, float* __restrict__ reward_out, int g, int lane)
{
    const int A = v.A;
    for (int i = lane; i < k; i += 64) {
        cand_action[size_t(g) * A + i] = out[i].action;
        cand_policy[size_t(g) * A + i] = out[i].policy;
        cand_logit[size_t(g) * A + i] = out[i].logit;
    }
    if (lane == 0) {
        const bool terminal = v.terminal[g] != 0;
        cand_count[g] = k;
        cand_player[g] = v.leaf_player[g];
        value_out[g] = terminal ? v.eval[g] : value[g];
        reward_out[g] = 0.0f;
    }
}
__device__ __forceinline__ void azCandBody(const GoDevView& v, const float* __restrict__ policy, const float* __restrict__ logit,
                                           const float* __restrict__ value, int rot, int* __restrict__ cand_count, int* __restrict__ cand_action,
                                           float* __restrict__ cand_policy, float* __restrict__ cand_logit, int* __restrict__ cand_player,
                                           float* __restrict__ value_out, float* __restrict__ reward_out, int* __restrict__ err, int g, int lane,
                                           uint64_t* __restrict__ smem)
{
    Cand* cs = reinterpret_cast<Cand*>(smem);
    Cand* out = cs + v.A;
    int* stack = reinterpret_cast<int*>(out + v.A);
    const int k = azCandGather(v, policy, logit, rot, g, lane, cs);
    if (k > 0) {
        waveSync();
        orderCandidates(cs, out, stack, k, lane, err);
    }
    azCandStore(v, value, out, k, cand_count, cand_action, cand_policy, cand_logit, cand_player, value_out, reward_out, g, lane);
}

// scratch of the cooperative variant behind the cs / out / stack block: dense[128] floats + nw x 256 partial counts
inline size_t candCoopOffsetBytes(int A) { return (azCandSmemBytes(A) + 15) & ~size_t(15); }
inline size_t candCoopSmemBytes(int A, int nw) { return candCoopOffsetBytes(A) + kCandCoopMax * sizeof(float) + size_t(nw) * 256 * sizeof(int); }
inline size_t candCoopSmemBytesW(int A, int nw) { return candCoopOffsetBytes(A) + kCandCoopMaxW * sizeof(float) + size_t(nw) * 2 * kCandCoopMaxW * sizeof(int); }

} // namespace mz
