// Tail help of the one-game-per-CU simulation kernel (sim_az_body.h): a workgroup whose game has finished the launch's simulations becomes the HELPER of a game
// of its XCD that is still running and computes half of the output channels of that game's tower.
//
// The games of a launch do not cost the same (terminal leaves skip the network, paths differ in depth), the launch lasts as long as its slowest game, and a CU
// whose game is done has nothing else to run: every phase of a game is a dependent chain on one CU.  What an idle CU can take over is half of another game's
// tower, with the building blocks of the MuZero cluster (sim_cluster.h):
//  * pair tower: member m (0 = the game's own workgroup, the owner; 1 = the helper) computes oc-tiles 2 m and 2 m + 1 of every layer for all pixel tiles — 12
//    (oc-tile, pixel-tile) units on 8 waves, three tiles per SIMD — with the layer function of the solo tower (tower_layer_geo, XOUT epilogue): every output is the
//    same tap-major, k-ordered chain, so the activations are bit-identical to the solo tower's;
//  * after each layer the members swap their 32 x P outputs through two alternating buffers in global memory, i.e. through the L2 of the XCD they share, with
//    self-validating words (the phase of the exchange in the sign bit of the ReLU outputs) and loads past the vector cache; after the last layer only the owner reads;
//  * the owner tells the helper what to compute with 16-byte stores that each carry the simulation's sequence number (three words of the leaf's bit-packed
//    planes + the sequence number), so the helper needs no other input and never touches the tree.
//    No whole (oc-tile, pixel-tile) dealing gets below 3 x 144 = 432 MFMAs on one SIMD (20 full units over 8 SIMDs), where the work is 392 per SIMD.  So ONE chain
//    per oc-tile is split: SIMDs s and s + 1 (s = 0, 2) share oc-tile 2 m + s / 2.  On SIMD s the low wave has tiles {0, 1}, its partner (wave s + 4) brings tile
//    2 up to tap kPairCut = 6 — 96 MFMAs, no epilogue —, stores its f32x4 accumulator to a slot in LDS (64 lanes x 16 bytes per oc-tile) and publishes the number
//    of the layer behind it (hpHandOut).  On SIMD s + 1 the low wave has tiles {3, 4}; its partner runs the corner tile's chain and epilogue as before (64 MFMAs),
//    polls for the layer's number, takes the accumulator (hpHandIn) and runs taps 6 .. 8 of tile 2 in the same k order (48 MFMAs) and that tile's epilogue:
//    384 and 400 MFMAs per SIMD and layer, and every output is still the one tap-major, k-ordered chain (tower_layer_geo TAP0 / TAP1 / ACC_IN / EPI).
//    The wait cannot hang: the first wave waits for nobody before it publishes, both waves belong to one resident workgroup, the poll is bounded (kHpPollLimit
//    rounds of s_sleep; then the abort flag and kHpErrHand are raised and the exchange behind the layer makes the workgroup leave).  The two barriers of the
//    exchange lie between one use of the slot and the next; the words are cleared at the start of a tower and the layers count from 1, so a word left by an earlier
//    layer or tower never matches.  Measured (profiles/r20_pair_split_tower.txt): 93.35 -> 88.0 us per pair tower.
//    (Tried beside it and dropped: waves that are done with their epilogue polling for the other member's half at once instead of behind the exchange's first
//    barrier — the planes they write are read by nobody during the layer.  89.8 us against 88.8: the early polls cost the waves that still compute more than
//    they take off the end of the layer.)
// Every wait is bounded; a time-out raises the pool's error flag and both sides leave the kernel.  No workgroup waits for one that is not running: a helper only
// claims a game that has published its XCC_ID in this launch, an owner only waits for a helper that has claimed it.
//
// Up to three helpers per game (quad tower, below): a game has three helper slots.  A finished workgroup first looks for a running game without a helper (slot
// 1), and only if its XCD has none for a helped game with a free slot 2 or 3, least progress first, so that two idle CUs converge on one game.  The owner reads
// slot 1 at every simulation and, once it is claimed, slots 2 and 3: with all three claimed the simulation's tower is a quad tower (one oc-tile per member), with
// slot 1 alone a pair tower (three members would split 2 / 1 / 1), otherwise the solo tower.  The sequence word of every command unit also carries the mode
// and the low bits of the game's exchange count at which this tower starts (hpCmdWord): a helper that joins in mid-launch has not counted the exchanges before.
// The holder of slot 2 or 3 skips the commands of pair towers and waits — bounded, error flag kHpErrQuadCmd — for the first quad command, or leaves when the
// owner's progress word says the game is done (its third partner never came) and searches again.  A helper stays with its game until that game is done, so a
// game's mode only ever goes solo -> pair -> quad within a launch.  The invariants above hold as they are: every wait is a bounded poll with s_sleep (error flags
// 95 / 96 for the pair's exchange and command, kHpErrQuad / kHpErrQuadCmd for the quad's); a slot is only claimed in a game that published its XCC_ID in this
// launch, by a workgroup that runs on the same XCD; the owner waits only for members whose slots it has seen claimed; no cooperative launch is needed.
//
// Lending: a game that is AHEAD lends one tower to a game of its XCD that is behind, in mid-launch.  A CU only becomes a helper once its own game is done; by then few
// games are left.  A game that leads another by `lend_lead` simulations has the same slack earlier and can spend it on pair towers, one at a time, spread over all
// the slow games (sim_az_body.h simLendScan / simLendTower; only in the value-first order, MZ_NO_SPEC=256: off).
//  * The offer word (kHpOffer) of a game: 0 closed, s = open for the game's simulation s (its sequence number, 1 ..), s | kHpOfferClaimed = taken by a volunteer.
//    Wave 7 of a game WITHOUT a helper in slot 1 opens the offer of simulation s when it arrives in front of the barrier behind the leaf — beside wave 0's walk — and
//    closes it by compare-and-swap s -> 0 when the walk is done, beside the leaf's first half.  A swap that fails has met s | kHpOfferClaimed: this simulation's tower
//    is a pair tower with the volunteer as member 1, commanded exactly as a slot-1 helper is.  A terminal leaf has no tower: the owner stores 0 (the offer is
//    withdrawn).  Behind the tower the owner stores 0 too.  The sequence number in the word keeps a late swap from hitting a later offer.
//  * The volunteer: while its own offer is open, wave 7 reads the XCC_ID and offer words of the games of its XCD past the vector cache (the loop of simHelpTail).
//    It takes the open offer of least progress of a game that published the same XCC_ID, has at least help_min_left simulations left and trails by at least
//    `lend_lead` — by compare-and-swap s -> s | kHpOfferClaimed, and only after it has closed its OWN offer of this simulation by compare-and-swap (a swap that
//    fails there means it has a volunteer itself and takes nothing).  Behind the barrier — its own walk and leaf are done, its hand-over block is complete, the tiles
//    are free, every wave is present — it waits for the command of simulation s, takes the planes into staging words of its own (not its hand-over block, which
//    holds its own leaf), runs ONE pair tower as member 1 and goes on with its own planes and tower.
//  * Whom a command is for: bit 27 of the command word (hpCmdLent; the sequence number keeps 27 bits).  A finished workgroup that claims slot 1 of a game in the
//    same simulation in which a volunteer has taken its offer skips the lent command like the holder of slot 2 skips a pair command, and a volunteer only takes a
//    command with the bit set and its offer's sequence number.  help_xseq advances by nlayers for a lent tower like for any pair tower, and the command carries it.
// The invariants, with lending: every wait is a bounded poll (kHpPollLimit) that raises the pool's error flag and leaves (kHpErrLend: the volunteer's wait for its
// command; kVfErr: wave 7's wait for the end of the walk, behind which it still closes its offer like any other, so that nobody who might take it is left waiting).  A volunteer waits only for an owner that is resident and in front of its tower: the offer it took was
// open, so the owner had not passed the barrier behind its leaf, and an owner whose offer is taken does not lend in that simulation — it sends the command behind its
// own leaf and planes, or withdraws the offer.  An owner waits (in the tower's first exchange) only for a volunteer whose claim it has seen.  Nobody waits for a
// workgroup that has an offer of its own open: a volunteer has closed its own before it takes one, so chains and cycles of waiting workgroups cannot form.  There
// is no cooperative launch: owner and volunteer are both resident and running when the claim is made.  Lending stays within one XCD.  Tail help works as before, and
// slots 2 and 3 are never taken by a volunteer.  A game with a helper in slot 1 neither offers nor lends.  The exchange buffers are re-used as between any two pair
// towers of a game: the owner sends the next command — to whichever member 1 — only after it has read the last exchange of the tower before.
#pragma once
#include "net_body.h"

namespace mz {

// per-game help block in global memory (32-bit words); the host clears it before every launch that may help
constexpr int kHpXcc = 0;       // XCC_ID + 1 of the owner (0: the game's workgroup has not started yet)
constexpr int kHpProgress = 1;  // simulations of this launch the owner has finished
constexpr int kHpHelper = 32;   // 0 or (helper's game index + 1), claimed by compare-and-swap (a 128-byte line of its own: the owner reads it at every simulation)
constexpr int kHpCmd = 64;      // up to 32 units of 16 bytes: {three words of the leaf's planes, hpCmdWord of the simulation}
constexpr int kHpHelper2 = 192; // helper slots 2 and 3, like kHpHelper, each on a line of its own behind the command
constexpr int kHpHelper3 = 224;
constexpr int kHpOffer = 256;   // lending: 0 closed, the owner's sequence number = open for that simulation, | kHpOfferClaimed = a volunteer has taken it (a line of its own)
constexpr unsigned kHpOfferClaimed = 0x40000000u;
constexpr int kHpXbuf = 320;    // 2 x [C][P] floats
constexpr int kHpPollLimit = 1 << 21;
constexpr int kHpMaxUnits = 32;
constexpr int kHpMaxGames = 1024; // games of a launch that helps (simLaunch's gate): simHelpTail and simLendScan pack (progress << 10) | game into one search key
constexpr int kHpErrQuad = 98, kHpErrQuadCmd = 99; // error flags: a quad tower's exchange timed out (95: the pair's), the holder of slot 2 or 3 saw no command (96: slot 1)
constexpr int kHpErrLend = 100;                    // a volunteer saw neither the command of the offer it had claimed nor its withdrawal
constexpr int kHpErrHand = 101;                    // pair tower: the second wave of a split chain did not see the first wave's accumulator
constexpr int kHpModePair = 0, kHpModeQuad = 1;
// the hand-over slot of the pair tower's split chains, in the LDS of each member: per oc-tile of the member 64 lanes x 16 bytes of accumulator, behind them one
// sequence word per oc-tile (kHpSlotFloats keeps what follows on 16 bytes)
constexpr int kHpSlotAcc = 2 * 64 * 4, kHpSlotFloats = kHpSlotAcc + 4;
constexpr int kPairCut = 6; // the first wave of a split chain runs taps [0, kPairCut), the second wave the rest
// the last word of every command unit: the simulation's sequence number (1 ..), whether the command is for a volunteer (lending) or for the holders of the helper
// slots, the tower's mode and the exchange count it starts at (its two low bits: hpPart and hpSign use no others); a unit is valid when all units of the command
// carry the same word
__host__ __device__ constexpr unsigned hpCmdWord(unsigned seq, int mode, unsigned xseq, bool lent = false)
{
    return (seq & 0x07FFFFFFu) | (lent ? 0x08000000u : 0u) | (unsigned(mode) << 28) | ((xseq & 3u) << 29);
}
__host__ __device__ constexpr unsigned hpCmdSeq(unsigned w) { return w & 0x07FFFFFFu; }
__host__ __device__ constexpr bool hpCmdLent(unsigned w) { return (w & 0x08000000u) != 0u; }
__host__ __device__ constexpr int hpCmdMode(unsigned w) { return int((w >> 28) & 1u); }
__host__ __device__ constexpr unsigned hpCmdXseq(unsigned w) { return w >> 29; }
typedef unsigned hpu4 __attribute__((ext_vector_type(4)));
inline size_t helpWords(int C, int P) { return (size_t(kHpXbuf) + 2 * size_t(C) * P + 31) / 32 * 32; }
__host__ __device__ constexpr int helpCmdUnits(int feat_words) { return (feat_words + 2) / 3; }

// loads that are served by the L2 (relaxed agent-scope atomic load = global_load_dword sc1), stores that the compiler may not delay or merge
__device__ __forceinline__ unsigned hpLoadU(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float hpLoadF(const float* p) { return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
__device__ __forceinline__ void hpStoreU(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned hpXccId()
{
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    return (id & 15u) + 1u;
}

struct HelpCtx {
    unsigned* hb;   // the helped game's block
    int member;     // 0 owner, 1 helper (quad tower: 1-3, the helper's slot)
    unsigned xseq;  // layer exchanges of this game so far in this launch
    int* abort_lds; // workgroup-wide abort flag
    int* err;
    float* slot = nullptr; // pair tower: kHpSlotFloats floats of LDS, 16-byte aligned (the quad tower has no use for it)
};

// The hand-over of a split chain's accumulator between two waves of a member (towerBodyPair): the first wave stores its lanes' f32x4 and, behind them, the
// layer's number; the second wave polls for that number — bounded, kHpErrHand — and takes the accumulator.  The word is cleared at the start of every tower and a
// tower's layers count 1, 2, ..: a word left by an earlier layer or tower never matches.
typedef __attribute__((address_space(3))) f32x4 HpLdsAcc;
typedef __attribute__((address_space(3))) unsigned HpLdsWord;
__device__ __forceinline__ void hpHandOut(const HelpCtx& c, int half, int lane, const f32x4& acc, unsigned seq)
{
    ((HpLdsAcc*)c.slot)[half * 64 + lane] = acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { __hip_atomic_store((HpLdsWord*)c.slot + kHpSlotAcc + half, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
}
__device__ __forceinline__ bool hpHandIn(const HelpCtx& c, int half, int lane, f32x4& acc, unsigned seq)
{
    HpLdsWord* w = (HpLdsWord*)c.slot + kHpSlotAcc + half;
    unsigned seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    for (int i = 0; i < kHpPollLimit && seen != seq; ++i) {
        __builtin_amdgcn_s_sleep(1);
        seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (seen != seq) {
        if (lane == 0) { *c.abort_lds = 1; atomicExch(c.err, kHpErrHand); }
        return false;
    }
    acc = ((HpLdsAcc*)c.slot)[half * 64 + lane];
    return true;
}

// my 16 x P block of the exchange buffer for the NEXT exchange, and the tag its words carry (the two buffers alternate, the phase flips each time a buffer is
// reused; the host clears them: phase 0 = "never written", the first use writes 1)
template <int CPAD, int P>
__device__ __forceinline__ float* hpPart(const HelpCtx& c, int ot) { return reinterpret_cast<float*>(c.hb + kHpXbuf) + size_t(c.xseq & 1) * CPAD * P + size_t(ot) * 16 * P; }
__device__ __forceinline__ unsigned hpSign(const HelpCtx& c) { return (((c.xseq >> 1) & 1u) ^ 1u) << 31; }

// All 512 threads of both members, after a layer: my 32 channels are in LDS (`tout`, padded planes) and on their way to the exchange buffer; on return the other
// member's 32 channels are in `tout` too.  false: the other member went missing (the caller leaves the kernel).  read = false (the helper after the last layer):
// nobody needs the owner's half any more.  A member overwrites a buffer only after it has read the exchange in between, i.e. after the other one has finished
// reading this one; the helper's skipped read is made up for by its wait for the next simulation's command, which the owner sends after it has read everything.
template <int H, int W, int CPAD>
__device__ __forceinline__ bool hpExchange(HelpCtx& c, float* __restrict__ tout, int tid, bool read)
{
    constexpr int P = H * W, PW = W + 2, CS = planeStride(H, W), HALF = CPAD / 2 * P;
    const unsigned sign = hpSign(c);
    const int other = 1 - c.member;
    const float* xb = reinterpret_cast<const float*>(c.hb + kHpXbuf) + size_t(c.xseq & 1) * CPAD * P + size_t(other) * HALF;
    ++c.xseq;
    __syncthreads(); // the member's own waves are done with the layer: all waves start polling together
    if (!read) { return true; }
    constexpr int K = (HALF + 511) / 512;
    unsigned got[K];
    bool ok = false;
    for (int polls = 0; polls < kHpPollLimit; ++polls) {
        ok = true;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = tid + j * 512;
            const bool want = i < HALF;
            got[j] = __float_as_uint(hpLoadF(xb + (want ? i : 0)));
            ok = ok && (!want || (got[j] & 0x80000000u) == sign);
        }
        ok = __all(ok);
        if (ok) { break; }
        __builtin_amdgcn_s_sleep(2);
    }
    if (!ok && (tid & 63) == 0) { *c.abort_lds = 1; atomicExch(c.err, 95); }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = tid + j * 512;
        if (i < HALF) {
            const int ch = other * (CPAD / 2) + i / P, p = i % P;
            tout[ch * CS + (p / W + 1) * PW + (p % W) + 1] = __uint_as_float(got[j] & 0x7FFFFFFFu);
        }
    }
    __syncthreads();
    return *c.abort_lds == 0;
}

// the layer sequence of one wave of a member: oc-tile `ot` x the NT pixel tiles from `tile0` (CORNER: the last of them is the corner tile)
template <int H, int W, int CIN0_PAD, int CPAD, int NT, bool CORNER>
__device__ __forceinline__ bool pairRun(const float* __restrict__ params, const TowerArgs& ta, float* __restrict__ T0, float* __restrict__ T1, int lane, int tid, int ot,
                                        int tile0, HelpCtx& c)
{
    constexpr int P = H * W;
    const PixSet<NT> px = makePixSet<H, W, NT>(lane, tile0);
    float aS[CIN0_PAD / 4], aA[CPAD / 4], aB[CPAD / 4];
    bool have = false;
    if (ta.has_stem) {
        const float* nw = ta.nlayers > 1 ? params + ta.w_off[1] : nullptr;
        tower_layer<H, W, CIN0_PAD / 4, NT, CPAD / 4, CORNER, false, true>(T0, nullptr, T1, nullptr, params + ta.w_off[0], params + ta.b_off[0], ta.C, ta.OT, lane, ot, px, false,
                                                                           aS, nw, aA, hpPart<CPAD, P>(c, ot), hpSign(c));
        have = nw != nullptr;
        if (!hpExchange<H, W, CPAD>(c, T1, tid, c.member == 0 || ta.nlayers > 1)) { return false; }
    }
    float *x = T1, *tmp = T0;
#pragma unroll 1
    for (int l = ta.has_stem; l < ta.nlayers; ++l) {
        const bool second = ((l - ta.has_stem) & 1) != 0, last = l + 1 == ta.nlayers;
        tower_layer<H, W, CPAD / 4, NT, CPAD / 4, CORNER, false, true>(second ? tmp : x, second ? x : nullptr, second ? x : tmp, nullptr, params + ta.w_off[l], params + ta.b_off[l],
                                                                       ta.C, ta.OT, lane, ot, px, have, aA, last ? nullptr : params + ta.w_off[l + 1], aB, hpPart<CPAD, P>(c, ot),
                                                                       hpSign(c));
#pragma unroll
        for (int cg = 0; cg < CPAD / 4; ++cg) { aA[cg] = aB[cg]; }
        have = !last;
        if (!hpExchange<H, W, CPAD>(c, second ? x : tmp, tid, c.member == 0 || !last)) { return false; }
    }
    return true;
}

// The split chain of pixel tile 2 (towerBodyPair), first wave: taps [0, kPairCut) of every layer, no epilogue — the accumulator goes to the slot of oc-tile half
// `half` of the member.  The wave waits for nobody but the exchanges.
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __forceinline__ bool pairRunHead(const float* __restrict__ params, const TowerArgs& ta, float* __restrict__ T0, float* __restrict__ T1, int lane, int tid, int ot,
                                            int half, HelpCtx& c)
{
    const PixSet<1> px = makePixSet<H, W, 1>(lane, 2);
    float aS[CIN0_PAD / 4], aA[CPAD / 4], aB[CPAD / 4];
    bool have = false;
    f32x4 acc;
    if (ta.has_stem) {
        const float* nw = ta.nlayers > 1 ? params + ta.w_off[1] : nullptr;
        tower_layer<H, W, CIN0_PAD / 4, 1, CPAD / 4, false, false, true, 0, kPairCut, false, false>(T0, nullptr, T1, nullptr, params + ta.w_off[0], params + ta.b_off[0], ta.C, ta.OT,
                                                                                                    lane, ot, px, false, aS, nw, aA, nullptr, 0u, &acc);
        hpHandOut(c, half, lane, acc, 1u);
        have = nw != nullptr;
        if (!hpExchange<H, W, CPAD>(c, T1, tid, c.member == 0 || ta.nlayers > 1)) { return false; }
    }
    float *x = T1, *tmp = T0;
#pragma unroll 1
    for (int l = ta.has_stem; l < ta.nlayers; ++l) {
        const bool second = ((l - ta.has_stem) & 1) != 0, last = l + 1 == ta.nlayers;
        tower_layer<H, W, CPAD / 4, 1, CPAD / 4, false, false, true, 0, kPairCut, false, false>(second ? tmp : x, second ? x : nullptr, second ? x : tmp, nullptr, params + ta.w_off[l],
                                                                                                params + ta.b_off[l], ta.C, ta.OT, lane, ot, px, have, aA,
                                                                                                last ? nullptr : params + ta.w_off[l + 1], aB, nullptr, 0u, &acc);
        hpHandOut(c, half, lane, acc, unsigned(l) + 1u);
#pragma unroll
        for (int cg = 0; cg < CPAD / 4; ++cg) { aA[cg] = aB[cg]; }
        have = !last;
        if (!hpExchange<H, W, CPAD>(c, second ? x : tmp, tid, c.member == 0 || !last)) { return false; }
    }
    return true;
}

// ... second wave: the corner tile's chain of the layer as before, then taps [kPairCut, 9) of pixel tile 2 on the first wave's accumulator, in the same k order,
// and that tile's epilogue.  The fragments of tap kPairCut are fetched during the corner chain's last tap (the layer function's look-ahead, pointed at this layer's
// own weights), so the wait for the accumulator hides their round trip.  A wait that times out leaves the tile undone: the abort flag is up, and the exchange
// behind the layer returns false.
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __forceinline__ bool pairRunCornerTail(const float* __restrict__ params, const TowerArgs& ta, float* __restrict__ T0, float* __restrict__ T1, int lane, int tid, int ot,
                                                  int half, HelpCtx& c)
{
    constexpr int P = H * W;
    const PixSet<1> pxc = makePixSet<H, W, 1>(lane, 5), pxt = makePixSet<H, W, 1>(lane, 2);
    float nS[CIN0_PAD / 4], cutS[CIN0_PAD / 4], nA[CPAD / 4], cutA[CPAD / 4]; // (nS, nA: never read — the corner chain starts without fragments, the rest fetches none ahead)
    f32x4 acc;
    if (ta.has_stem) {
        const float* wl = params + ta.w_off[0];
        tower_layer<H, W, CIN0_PAD / 4, 1, CIN0_PAD / 4, true, false, true>(T0, nullptr, T1, nullptr, wl, params + ta.b_off[0], ta.C, ta.OT, lane, ot, pxc, false, nS,
                                                                            wl + size_t(kPairCut) * ta.OT * (CIN0_PAD / 4) * 64, cutS, hpPart<CPAD, P>(c, ot), hpSign(c));
        if (hpHandIn(c, half, lane, acc, 1u)) {
            tower_layer<H, W, CIN0_PAD / 4, 1, CPAD / 4, false, false, true, kPairCut, 9, true, true>(T0, nullptr, T1, nullptr, wl, params + ta.b_off[0], ta.C, ta.OT, lane, ot, pxt, true,
                                                                                                      cutS, nullptr, nA, hpPart<CPAD, P>(c, ot), hpSign(c), &acc);
        }
        if (!hpExchange<H, W, CPAD>(c, T1, tid, c.member == 0 || ta.nlayers > 1)) { return false; }
    }
    float *x = T1, *tmp = T0;
#pragma unroll 1
    for (int l = ta.has_stem; l < ta.nlayers; ++l) {
        const bool second = ((l - ta.has_stem) & 1) != 0, last = l + 1 == ta.nlayers;
        const float* wl = params + ta.w_off[l];
        tower_layer<H, W, CPAD / 4, 1, CPAD / 4, true, false, true>(second ? tmp : x, second ? x : nullptr, second ? x : tmp, nullptr, wl, params + ta.b_off[l], ta.C, ta.OT, lane, ot,
                                                                    pxc, false, nA, wl + size_t(kPairCut) * ta.OT * (CPAD / 4) * 64, cutA, hpPart<CPAD, P>(c, ot), hpSign(c));
        if (hpHandIn(c, half, lane, acc, unsigned(l) + 1u)) {
            tower_layer<H, W, CPAD / 4, 1, CPAD / 4, false, false, true, kPairCut, 9, true, true>(second ? tmp : x, second ? x : nullptr, second ? x : tmp, nullptr, wl,
                                                                                                  params + ta.b_off[l], ta.C, ta.OT, lane, ot, pxt, true, cutA, nullptr, nA,
                                                                                                  hpPart<CPAD, P>(c, ot), hpSign(c), &acc);
        }
        if (!hpExchange<H, W, CPAD>(c, second ? x : tmp, tid, c.member == 0 || !last)) { return false; }
    }
    return true;
}

// shapes the pair tower covers: 4 oc-tiles (two per member), 6 pixel tiles the last of which is the corner tile (9x9)
template <int H, int W, int CPAD>
constexpr bool pairTowerShape() { return CPAD == 64 && TileMap<H, W>::PT == 6 && TileMap<H, W>::kCorner; }

// The tower of one simulation on a pair of workgroups: each member unpacks the leaf's planes (`bits`: cin0 x ceil(P / 32) words) into its own LDS tile, computes
// its two oc-tiles of every layer and swaps them with the other member; the owner ends with the complete output x in its tile T1 (returned), the helper with all
// but the owner's half of the last layer.  nullptr: aborted.
// Waves w and w + 4 share a SIMD.  SIMD s works on oc-tile 2 m + s / 2: the wave of the lower half takes two full pixel tiles (0, 1 or 3, 4), its partner one
// (the first six taps of tile 2; or the corner tile 5 and then the last three taps of tile 2 — the split chain of the header comment) with the higher priority,
// like the wave with fewer accumulator chains of the solo tower (net_body.h towerBody): at most 400 MFMAs per SIMD and layer instead of 784.
// c.slot: kHpSlotFloats floats of LDS outside the tiles.
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __forceinline__ float* towerBodyPair(const unsigned* __restrict__ bits, const float* __restrict__ params, const TowerArgs& ta, int tid, float* __restrict__ tiles,
                                                HelpCtx& c)
{
    static_assert(pairTowerShape<H, W, CPAD>(), "pair tower: two oc-tiles per member, pixel tiles {0, 1}, {2}, {3, 4}, {corner}");
    constexpr int P = H * W, PW = W + 2, CS = planeStride(H, W), W32 = (P + 31) / 32;
    constexpr int CMAX = CIN0_PAD > CPAD ? CIN0_PAD : CPAD;
    const int lane = tid & 63, wave = tid >> 6;
    float* T0 = tiles;
    float* T1 = tiles + CMAX * CS;
    for (int i = tid; i < kTowerTiles * CMAX * CS / 4; i += 512) { reinterpret_cast<float4*>(tiles)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    if (tid < 2) { ((HpLdsWord*)c.slot)[kHpSlotAcc + tid] = 0u; } // the sequence words of the hand-over: a tower's layers count from 1
    __syncthreads();
    float* Tin = ta.has_stem ? T0 : T1;
    for (int i = tid; i < ta.cin0 * P; i += 512) {
        const int ch = i / P, p = i - ch * P;
        Tin[ch * CS + (p / W + 1) * PW + (p % W) + 1] = ((bits[ch * W32 + (p >> 5)] >> (p & 31)) & 1u) ? 1.0f : 0.0f;
    }
    __syncthreads();
    const int simd = wave & 3, ot = 2 * c.member + (simd >> 1), grp = simd & 1;
    bool ok;
    if (wave < 4) {
        ok = pairRun<H, W, CIN0_PAD, CPAD, 2, false>(params, ta, T0, T1, lane, tid, ot, 3 * grp, c);
    } else {
        __builtin_amdgcn_s_setprio(2);
        if (grp == 0) { ok = pairRunHead<H, W, CIN0_PAD, CPAD>(params, ta, T0, T1, lane, tid, ot, simd >> 1, c); }
        else { ok = pairRunCornerTail<H, W, CIN0_PAD, CPAD>(params, ta, T0, T1, lane, tid, ot, simd >> 1, c); }
        __builtin_amdgcn_s_setprio(0);
    }
    return ok ? T1 : nullptr;
}

// ---- quad tower: four members (0 = the owner, 1-3 = the holders of the game's helper slots), member m computes oc-tile m of every layer for all pixel tiles
// with the same layer function as the pair, so the activations are bit-identical to the pair's and the solo tower's.  The exchange buffers, hpPart and hpSign are
// the pair's: part `ot` of buffer (xseq & 1) holds oc-tile ot whoever wrote it, and every exchange writes all four parts in either mode, so a game may change
// between pair and quad towers from one simulation to the next while its exchange count runs on (a word of the exchange before last in the same buffer carries the
// other phase).
// Buffer reuse with four members: member A writes its part of buffer b for exchange x during layer x and overwrites it for exchange x + 2 during layer x + 2, which
// it starts only after it has read exchange x + 1 completely.  Every other member B wrote its part of exchange x + 1 during its layer x + 1, which B started behind
// the barrier that ends its read of exchange x: A's write for x + 2 comes after every B has finished reading x.  The read a helper skips after the last layer
// (exchange x_l) is made up for by its wait for the next command: the owner sends it after it has read all of x_l, whose parts every helper wrote after it
// had finished reading x_l - 1 — the buffer the next tower's first layer overwrites; nobody but the owner reads x_l, and the owner has.
template <int H, int W, int CPAD>
__device__ __forceinline__ bool hpExchangeQuad(HelpCtx& c, float* __restrict__ tout, int tid, bool read)
{
    constexpr int P = H * W, PW = W + 2, CS = planeStride(H, W), OWN = CPAD / 4 * P, OTHERS = 3 * OWN;
    const unsigned sign = hpSign(c);
    const float* xb = reinterpret_cast<const float*>(c.hb + kHpXbuf) + size_t(c.xseq & 1) * CPAD * P;
    const int own0 = c.member * OWN; // the words [own0, own0 + OWN) of the buffer are this member's own
    ++c.xseq;
    __syncthreads(); // the member's own waves are done with the layer: all waves start polling together
    if (!read) { return true; }
    constexpr int K = (OTHERS + 511) / 512;
    unsigned got[K];
    bool ok = false;
    for (int polls = 0; polls < kHpPollLimit; ++polls) {
        ok = true;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = tid + j * 512;
            const bool want = i < OTHERS;
            const int src = want ? i + (i >= own0 ? OWN : 0) : (own0 == 0 ? OWN : 0);
            got[j] = __float_as_uint(hpLoadF(xb + src));
            ok = ok && (!want || (got[j] & 0x80000000u) == sign);
        }
        ok = __all(ok);
        if (ok) { break; }
        __builtin_amdgcn_s_sleep(2);
    }
    if (!ok && (tid & 63) == 0) { *c.abort_lds = 1; atomicExch(c.err, kHpErrQuad); }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = tid + j * 512;
        if (i < OTHERS) {
            const int src = i + (i >= own0 ? OWN : 0), ch = src / P, p = src % P;
            tout[ch * CS + (p / W + 1) * PW + (p % W) + 1] = __uint_as_float(got[j] & 0x7FFFFFFFu);
        }
    }
    __syncthreads();
    return *c.abort_lds == 0;
}

// the layer sequence of one wave of a quad member: oc-tile c.member x pixel tile `tile` (HAS_TILE = false: a wave without a tile, which only takes part in the exchanges)
template <int H, int W, int CIN0_PAD, int CPAD, bool HAS_TILE, bool CORNER>
__device__ __forceinline__ bool quadRun(const float* __restrict__ params, const TowerArgs& ta, float* __restrict__ T0, float* __restrict__ T1, int lane, int tid, int tile, HelpCtx& c)
{
    constexpr int P = H * W;
    const int ot = c.member;
    const PixSet<1> px = makePixSet<H, W, 1>(lane, HAS_TILE ? tile : 0);
    float aS[CIN0_PAD / 4], aA[CPAD / 4], aB[CPAD / 4];
    bool have = false;
    if (ta.has_stem) {
        const float* nw = ta.nlayers > 1 ? params + ta.w_off[1] : nullptr;
        if constexpr (HAS_TILE) {
            tower_layer<H, W, CIN0_PAD / 4, 1, CPAD / 4, CORNER, false, true>(T0, nullptr, T1, nullptr, params + ta.w_off[0], params + ta.b_off[0], ta.C, ta.OT, lane, ot, px, false,
                                                                              aS, nw, aA, hpPart<CPAD, P>(c, ot), hpSign(c));
        }
        have = nw != nullptr;
        if (!hpExchangeQuad<H, W, CPAD>(c, T1, tid, c.member == 0 || ta.nlayers > 1)) { return false; }
    }
    float *x = T1, *tmp = T0;
#pragma unroll 1
    for (int l = ta.has_stem; l < ta.nlayers; ++l) {
        const bool second = ((l - ta.has_stem) & 1) != 0, last = l + 1 == ta.nlayers;
        if constexpr (HAS_TILE) {
            tower_layer<H, W, CPAD / 4, 1, CPAD / 4, CORNER, false, true>(second ? tmp : x, second ? x : nullptr, second ? x : tmp, nullptr, params + ta.w_off[l], params + ta.b_off[l],
                                                                          ta.C, ta.OT, lane, ot, px, have, aA, last ? nullptr : params + ta.w_off[l + 1], aB, hpPart<CPAD, P>(c, ot),
                                                                          hpSign(c));
#pragma unroll
            for (int cg = 0; cg < CPAD / 4; ++cg) { aA[cg] = aB[cg]; }
        }
        have = !last;
        if (!hpExchangeQuad<H, W, CPAD>(c, second ? x : tmp, tid, c.member == 0 || !last)) { return false; }
    }
    return true;
}

// The tower of one simulation on four workgroups: like towerBodyPair, with one oc-tile per member.  Waves w and w + 4 share a SIMD; SIMD 0 works on pixel tiles
// 0 and 1, SIMD 1 on 2 and 3, one wave each (two single chains fill a SIMD's pipe: a dependent MFMA issues every 57 cycles, the pipe takes one every 32), SIMD 2
// on tile 4 and SIMD 3 on the corner tile: at most 2 x 144 = 288 MFMAs per SIMD and layer instead of the pair's 432.  The waves of a SIMD have the same number of
// chains, so none gets a priority; waves 6 and 7 have no tile and take part in the exchanges only.
template <int H, int W, int CIN0_PAD, int CPAD>
__device__ __forceinline__ float* towerBodyQuad(const unsigned* __restrict__ bits, const float* __restrict__ params, const TowerArgs& ta, int tid, float* __restrict__ tiles,
                                                HelpCtx& c)
{
    static_assert(pairTowerShape<H, W, CPAD>(), "quad tower: one oc-tile per member, pixel tiles {0, 1}, {2, 3}, {4}, {corner}");
    constexpr int P = H * W, PW = W + 2, CS = planeStride(H, W), W32 = (P + 31) / 32;
    constexpr int CMAX = CIN0_PAD > CPAD ? CIN0_PAD : CPAD;
    const int lane = tid & 63, wave = tid >> 6;
    float* T0 = tiles;
    float* T1 = tiles + CMAX * CS;
    for (int i = tid; i < kTowerTiles * CMAX * CS / 4; i += 512) { reinterpret_cast<float4*>(tiles)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __syncthreads();
    float* Tin = ta.has_stem ? T0 : T1;
    for (int i = tid; i < ta.cin0 * P; i += 512) {
        const int ch = i / P, p = i - ch * P;
        Tin[ch * CS + (p / W + 1) * PW + (p % W) + 1] = ((bits[ch * W32 + (p >> 5)] >> (p & 31)) & 1u) ? 1.0f : 0.0f;
    }
    __syncthreads();
    bool ok;
    if (wave == 3) { ok = quadRun<H, W, CIN0_PAD, CPAD, true, true>(params, ta, T0, T1, lane, tid, 5, c); }
    else if (wave < 3) { ok = quadRun<H, W, CIN0_PAD, CPAD, true, false>(params, ta, T0, T1, lane, tid, 2 * wave, c); }
    else if (wave < 6) { ok = quadRun<H, W, CIN0_PAD, CPAD, true, false>(params, ta, T0, T1, lane, tid, 2 * (wave - 4) + 1, c); }
    else { ok = quadRun<H, W, CIN0_PAD, CPAD, false, false>(params, ta, T0, T1, lane, tid, 0, c); }
    return ok ? T1 : nullptr;
}

} // namespace mz
