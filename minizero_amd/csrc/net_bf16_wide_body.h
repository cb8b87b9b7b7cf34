// The opt-in bf16x3 tower (`mz_nn_precision=bf16x3`) for 128 and 256 hidden channels (9x9) and for 64 hidden channels on 11x11 / 15x15 boards: the arithmetic of net_bf16_body.h — every f32 value v carried as
// hi = bf16(v), lo = bf16(v - hi), a product as three v_mfma_f32_16x16x32_bf16 (hi * lo, lo * hi, hi * hi) into one f32 accumulator, bias + skip + ReLU in
// f32, the stem's 0 / 1 planes as hi alone — on the data flow of the one-tile f32 tower (net_wide_body.h): the 64-channel body's four LDS buffers (x and t,
// each as hi and lo) would be 128 KB at 128 channels and 256 KB at 256.
//   * ONE tile in LDS: the current layer's input as a hi and a lo buffer, channel-innermost as in net_bf16_body.h with C / 8 chunks per position
//     (actByteW): 128 positions x C x 4 B = 64 KB at 128 channels, 128 KB at 256.  The 16 lanes a ds_read_b128 serves together read 16 positions of one
//     pixel tile, distinct mod 16 (TileMap), i.e. the 16 slots of 256-byte rows: no bank conflict.
//   * a layer = all MFMAs -> workgroup barrier -> the epilogue writes hi / lo IN PLACE over the tile.  Wave w of the 8 owns the C / 128 oc-tiles from
//     w * C / 128 and ALL pixel tiles (12 accumulator tiles at 256 channels), so every output belongs to the same lane in every layer: the block input x
//     goes as f32 to the workgroup's two blocks in global memory (L2-resident; SimArgs::act / act2 in the simulation kernel) in a per-lane order
//     (one coalesced dwordx4 per accumulator tile), where the lane that wrote it finds the skip values of the block's second conv.
//   * the last layer leaves f32: padded planes [C][CS] over the tile for the heads of the simulation kernel, or NCHW in global memory.
//   * A fragments ([tap][oc-tile][k-block][hi, lo][lane] x 8, bf16_split.h) travel D steps ahead of their MFMAs in a register ring, the next layer's first D
//     steps are fetched before the barrier; B fragments one step ahead in a pinned order (net_bf16_body.h).  The tap loop is a real loop (a 256-channel
//     layer unrolled would be 2600 MFMAs of code).
//   * 64 channels (11x11, 15x15: boards whose four buffers of net_bf16_body.h would not leave the simulation kernel its blocks) are 4 oc-tiles for 8 waves:
//     wave w owns oc-tile w & 3 and one of TWO PIXEL GROUPS (w >> 2), the split of the f32 one-tile tower (net_wide_body.h WideGeo: WO = 4, WP = 2) — 11x11:
//     4 + 4 pixel tiles; 15x15: 8 + 7, the last one the corner tile (225 = 14 * 16 + 1).  An output still belongs to the same lane in every layer.  With
//     KB = 2 k-blocks per tap the ring's D = 4 steps are two taps: the tap loop goes round the ring once per pair of taps, and tap 8 is taken alone.
// gfx950, -ffp-contract=off.
#pragma once
#include "net_bf16_body.h"
#include <type_traits>

namespace mz {

// Explicit address spaces: inside the simulation kernel the tower is a function of its own, whose pointer arguments are generic — their loads would be FLAT
// loads, which count on both wait counters, and every wait for a B operand from the LDS would wait for all the weight fragments in flight (net_body.h XPtr).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char LdsByte;
typedef __attribute__((address_space(3))) const u32x4 LdsCU32x4;
typedef __attribute__((address_space(3))) bf16x4 LdsBf16x4;
typedef __attribute__((address_space(3))) float LdsFloat;
typedef __attribute__((address_space(1))) const u32x4 GlbCU32x4;
typedef __attribute__((address_space(1))) f32x4 GlbF32x4;
typedef __attribute__((address_space(1))) const f32x4 GlbCF32x4;

template <int H, int W, int C>
struct Bf16WideGeo {
    using TM = TileMap<H, W>;
    static constexpr int BW = W, P = H * W, PW = W + 2, NPOS = (H + 2) * (W + 2), NPOS16 = (NPOS + 16) / 16 * 16; // at least one spare position (the dump slot)
    static constexpr int CH = C / 8, KB = C / 32, OT = C / 16;
    static constexpr int WO = OT < 8 ? OT : 8, WP = 8 / WO; // waves side by side over the oc-tiles / pixel groups (128, 256 channels: 8 / 1; 64 channels: 4 / 2)
    static constexpr int NOT = OT / WO;        // oc-tiles per wave
    static constexpr int PT = TM::PT;
    static constexpr int groupTiles(int wp) { return PT / WP + (wp < PT % WP ? 1 : 0); } // pixel tiles of group wp: consecutive ones, the corner tile in the last group
    static constexpr int NT = groupTiles(0);   // pixel tiles per wave, at most (WP == 1: all of them)
    static constexpr bool kCorner = TM::kCorner;
    static constexpr int D = NOT >= 2 ? 2 : 4; // steps the A fragments travel ahead (two oc-tiles per wave: 16 registers per step)
    static constexpr int kBufBytes = NPOS16 * C * 2; // one buffer (hi or lo)
    static constexpr int kDump = NPOS16 - 1;
    static constexpr int CS = (NPOS + 1 + 3) & ~3;   // plane stride of the last layer's f32 planes (one spare float: the dump slot)
    static constexpr int kTileBytes = 2 * kBufBytes > C * CS * 4 ? 2 * kBufBytes : C * CS * 4;
    // x in global memory: accumulator tile (i, j) of wave w as one float4 per lane; the wave's pixel tiles below NTH in the first block, the others in the second
    static constexpr int NTH = (NT + 1) / 2;
    static_assert((C == 64 || C % 128 == 0) && NOT * NT <= 12, "one-tile bf16 tower: 64, 128 or 256 hidden channels, at most 12 accumulator tiles per wave");
    static_assert(WP == 1 || (WP == 2 && groupTiles(1) >= 2), "one or two pixel groups, each with two halves of B fragments");
    static_assert(KB % D == 0 || 2 * KB == D, "the ring's slot of a step is its k-block's, or (two taps per round) its tap's parity and its k-block's");
    static_assert(8 * NOT * NTH * 64 * 4 <= C * P, "the per-lane order of x must fit a [C][P] block");
    static_assert(kTileBytes <= 160 * 1024, "the tile must fit the LDS");
};
template <int CH>
__device__ __forceinline__ int actByteW(int pos, int chunk) { return (((pos >> 4) * CH + chunk) * 16 + (pos & 15)) * 16; }

// One conv3x3 layer (KB k-blocks per tap: C / 32, or 1 for the stem, which has no lo input) for the NOT oc-tiles from ot0 and the wave's NT pixel tiles (px; all
// of them, or those of its pixel group; CORNER: the last one is the corner tile).
//   gskip / gkeep: this wave's part of x in global memory (see above), read as the skip values / written for a later layer; nullptr: neither
//   out_f32: last layer of the simulation kernel, f32 padded planes over the tile; gout: last layer of the stand-alone launch, f32 NCHW
//   next_wf: the fragments of the layer that follows (C / 32 k-blocks per tap): its first D steps are left in the ring
template <class G, int NT, bool CORNER, int KB, bool HAS_LO>
__device__ __forceinline__ void wideLayerBf16(LdsByte* tile, GlbF32x4* gskip0, GlbF32x4* gskip1, GlbF32x4* gkeep0, GlbF32x4* gkeep1, bool out_f32, float* __restrict__ gout,
                                              GlbCU32x4* wf, GlbCU32x4* next_wf, GlbCF32x4* bias, int lane, int ot0,
                                              const PixSetBf16<NT>& px, bool have_first, u32x4 (&ring)[G::D][G::NOT][2])
{
    constexpr int NOT = G::NOT, D = G::D, OT = G::OT, PW = G::PW, CH = G::CH, KBN = G::KB, NTH = G::NTH;
    static_assert(KB == 1 || KB == KBN, "stem or tower layer");
    static_assert(NT <= G::NT && NT - NTH <= NTH, "the wave's part of x: NTH tiles in each block");
    const int kg = lane >> 4;
    const LdsByte* in_hi = tile;
    const LdsByte* in_lo = tile + G::kBufBytes;
    f32x4 acc[NOT][NT];
#pragma unroll
    for (int i = 0; i < NOT; ++i) {
#pragma unroll
        for (int j = 0; j < NT; ++j) { acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
    }
    float biasv[NOT][4];
#pragma unroll
    for (int i = 0; i < NOT; ++i) {
        const f32x4 b4 = bias[4 * (ot0 + i) + kg];
        biasv[i][0] = b4[0]; biasv[i][1] = b4[1]; biasv[i][2] = b4[2]; biasv[i][3] = b4[3];
    }
    GlbCU32x4* wme = wf + size_t(ot0) * KB * 128 + lane;          // (tap t, k-block kb) of oc-tile ot0 + i: wme[((t * OT + i) * KB + kb) * 128]
    GlbCU32x4* nme = next_wf ? next_wf + size_t(ot0) * KBN * 128 + lane : nullptr;
    auto loadA = [&](u32x4 (&slot)[NOT][2], GlbCU32x4* p, int kb_stride) { // p: the step's fragments of oc-tile ot0
#pragma unroll
        for (int i = 0; i < NOT; ++i) { slot[i][0] = p[size_t(i) * kb_stride * 128]; slot[i][1] = p[size_t(i) * kb_stride * 128 + 64]; }
    };
    if (!have_first) {
#pragma unroll
        for (int s = 0; s < D; ++s) { loadA(ring[s], KB == 1 ? wme + size_t(s) * OT * 128 : wme + s * 128, KB); }
    }
    // B fragments half a step ahead of their MFMAs, in a pinned order (net_bf16_body.h): a step's pixel tiles are taken in two halves, so that two halves
    // of B fragments are in registers, not two steps' (48 registers less; at 256 channels the kernel spilled).  (The corner tile's reads outside its four taps
    // are all-zero padding; they are issued all the same — the loop body stays uniform — and only its MFMAs are left out.)
    constexpr int NH0 = (NT + 1) / 2, NH1 = NT - NH0;
    static_assert(NH1 >= 1, "two halves");
    auto bload = [&](auto half, int tapoff, int kb, u32x4 (&bh)[NH0], u32x4 (&bl)[NH0]) {
        constexpr int J0 = decltype(half)::value ? NH0 : 0, N = decltype(half)::value ? NH1 : NH0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int off = actByteW<CH>(px.src[J0 + j] + tapoff, kb * 4 + kg);
            bh[j] = *(LdsCU32x4*)(in_hi + off);
            if constexpr (HAS_LO) { bl[j] = *(LdsCU32x4*)(in_lo + off); }
        }
    };
    u32x4 b_hi[NH0], b_lo[NH0];
    // the MFMAs of half a step; product-major: consecutive MFMAs write different accumulators (three on one accumulator back to back wait for each other)
    auto mfmas = [&](auto half, auto inside, const u32x4 (&a)[NOT][2]) {
        constexpr int J0 = decltype(half)::value ? NH0 : 0;
        constexpr int N = !decltype(half)::value ? NH0 : (CORNER && !decltype(inside)::value) ? NH1 - 1 : NH1; // all-zero B operand of the corner tile: nothing to add
        if constexpr (HAS_LO) {
#pragma unroll
            for (int i = 0; i < NOT; ++i) {
#pragma unroll
                for (int j = 0; j < N; ++j) { acc[i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[i][0]), __builtin_bit_cast(bf16x8, b_lo[j]), acc[i][J0 + j], 0, 0, 0); }
            }
        }
#pragma unroll
        for (int i = 0; i < NOT; ++i) {
#pragma unroll
            for (int j = 0; j < N; ++j) { acc[i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[i][1]), __builtin_bit_cast(bf16x8, b_hi[j]), acc[i][J0 + j], 0, 0, 0); }
        }
#pragma unroll
        for (int i = 0; i < NOT; ++i) {
#pragma unroll
            for (int j = 0; j < N; ++j) { acc[i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[i][0]), __builtin_bit_cast(bf16x8, b_hi[j]), acc[i][J0 + j], 0, 0, 0); }
        }
    };
    auto takeB = [&](const u32x4 (&nh)[NH0], const u32x4 (&nl)[NH0]) {
#pragma unroll
        for (int j = 0; j < NH0; ++j) { b_hi[j] = nh[j]; if constexpr (HAS_LO) { b_lo[j] = nl[j]; } }
    };
    // one step: on entry b holds its first half; `fetch` puts the step's fragments into `a` and issues the ring's next load; (ntapoff, nkb): the step that follows
    auto step = [&](auto inside, int tapoff, int kb, int ntapoff, int nkb, auto&& fetch) {
        u32x4 n_hi[NH0], n_lo[NH0], a[NOT][2];
        bload(std::true_type{}, tapoff, kb, n_hi, n_lo);
        fetch(a);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(std::false_type{}, inside, a);
        __builtin_amdgcn_sched_barrier(0);
        takeB(n_hi, n_lo);
        bload(std::false_type{}, ntapoff, nkb, n_hi, n_lo);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(std::true_type{}, inside, a);
        __builtin_amdgcn_sched_barrier(0);
        takeB(n_hi, n_lo);
    };
    bload(std::false_type{}, 0, 0, b_hi, b_lo);
    if constexpr (KB == 1) { // the stem: nine steps, unrolled
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int sn = s < 8 ? s + 1 : 8; // (the last step fetches its own B fragments again: harmless)
            auto fetch = [&](u32x4 (&a)[NOT][2]) {
#pragma unroll
                for (int i = 0; i < NOT; ++i) { a[i][0] = ring[s % D][i][0]; a[i][1] = ring[s % D][i][1]; }
                if (s + D < 9) { loadA(ring[s % D], wme + size_t(s + D) * OT * 128, KB); }  // this slot's fragments are in `a` now
                else if (nme) { loadA(ring[s % D], nme + (size_t((s + D - 9) / KBN) * OT * KBN + (s + D - 9) % KBN) * 128, KBN); } // the next layer's step s + D - 9 (its tap, its k-block)
            };
            if (cornerTapInside(s)) { step(std::true_type{}, (s / 3) * PW + s % 3, 0, (sn / 3) * PW + sn % 3, 0, fetch); }
            else { step(std::false_type{}, (s / 3) * PW + s % 3, 0, (sn / 3) * PW + sn % 3, 0, fetch); }
        }
        if (nme) { // the ring holds the next layer's step i in slot (9 + i) % D: rotate it to slot i
            u32x4 tmp[D][NOT][2];
#pragma unroll
            for (int i = 0; i < D; ++i) {
#pragma unroll
                for (int k = 0; k < NOT; ++k) { tmp[i][k][0] = ring[(9 + i) % D][k][0]; tmp[i][k][1] = ring[(9 + i) % D][k][1]; }
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
#pragma unroll
                for (int k = 0; k < NOT; ++k) { ring[i][k][0] = tmp[i][k][0]; ring[i][k][1] = tmp[i][k][1]; }
            }
        }
    } else if constexpr (KB % D != 0) {
        // Fewer k-blocks than ring slots (64 channels: KB = 2, D = 4): the ring holds TWO taps.  Step (t, kb) is in slot (t & 1) * KB + kb, which then takes
        // step (t + 2, kb) — of this layer, of the next one (its tap t + 2 - 9), or, without one, this tap's own again (harmless).  The loop takes the taps in
        // pairs, so that a slot is a constant, and tap 8 alone; behind it the next layer's step i is in slot (9 * KB + i) % D, as behind the stem.
        static_assert(2 * KB == D && NOT == 1, "two taps per round of the ring");
        auto tapSteps = [&](auto odd, int t) {
            constexpr int S0 = decltype(odd)::value ? KB : 0;
            const int tn = t < 8 ? t + 1 : 8;
            const int tapoff = (t / 3) * PW + (t % 3), ntapoff = (tn / 3) * PW + (tn % 3);
            GlbCU32x4* ahead = t + 2 < 9 ? wme + size_t(t + 2) * OT * KB * 128 : (nme ? nme + size_t(t + 2 - 9) * OT * KB * 128 : wme + size_t(t) * OT * KB * 128);
            auto steps = [&](auto inside) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    auto fetch = [&](u32x4 (&a)[NOT][2]) {
                        a[0][0] = ring[S0 + kb][0][0]; a[0][1] = ring[S0 + kb][0][1];
                        loadA(ring[S0 + kb], ahead + kb * 128, KB);
                    };
                    if (kb + 1 < KB) { step(inside, tapoff, kb, tapoff, kb + 1, fetch); } else { step(inside, tapoff, kb, ntapoff, 0, fetch); }
                }
            };
            if (!CORNER || cornerTapInside(t)) { steps(std::true_type{}); } else { steps(std::false_type{}); }
        };
#pragma unroll 1
        for (int t = 0; t < 8; t += 2) {
            tapSteps(std::false_type{}, t);
            tapSteps(std::true_type{}, t + 1);
        }
        tapSteps(std::false_type{}, 8);
        if (nme) {
            u32x4 tmp[D][2];
#pragma unroll
            for (int i = 0; i < D; ++i) { tmp[i][0] = ring[(9 * KB + i) % D][0][0]; tmp[i][1] = ring[(9 * KB + i) % D][0][1]; }
#pragma unroll
            for (int i = 0; i < D; ++i) { ring[i][0][0] = tmp[i][0]; ring[i][0][1] = tmp[i][1]; }
        }
    } else {
        // one tap: its KB steps; step kb's fragments are in ring slot kb % D, which then takes step kb + D — of this tap, of the next one, or (behind tap 8)
        // of the next layer; the layer's last tap without a next layer fetches its own fragments again (harmless, and the loop body stays uniform)
        auto tapSteps = [&](auto inside, int tapoff, int ntapoff, GlbCU32x4* cur, GlbCU32x4* nxt) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                auto fetch = [&](u32x4 (&a)[NOT][2]) {
#pragma unroll
                    for (int i = 0; i < NOT; ++i) { a[i][0] = ring[kb % D][i][0]; a[i][1] = ring[kb % D][i][1]; }
                    if (kb + D < KB) { loadA(ring[kb % D], cur + (kb + D) * 128, KB); } else { loadA(ring[kb % D], nxt + (kb + D - KB) * 128, KB); }
                };
                if (kb + 1 < KB) { step(inside, tapoff, kb, tapoff, kb + 1, fetch); } else { step(inside, tapoff, kb, ntapoff, 0, fetch); }
            }
        };
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int tn = t < 8 ? t + 1 : 8;
            GlbCU32x4* cur = wme + size_t(t) * OT * KB * 128;
            GlbCU32x4* nxt = t < 8 ? wme + size_t(t + 1) * OT * KB * 128 : (nme ? nme : cur);
            const int tapoff = (t / 3) * PW + (t % 3), ntapoff = (tn / 3) * PW + (tn % 3);
            if (!CORNER || cornerTapInside(t)) { tapSteps(std::true_type{}, tapoff, ntapoff, cur, nxt); }
            else { tapSteps(std::false_type{}, tapoff, ntapoff, cur, nxt); }
        }
    }
    // the skip values: in the registers before the barrier
    f32x4 sk[NOT][NT];
    if (gskip0) {
#pragma unroll
        for (int i = 0; i < NOT; ++i) {
#pragma unroll
            for (int j = 0; j < NT; ++j) { sk[i][j] = j < NTH ? gskip0[(i * NTH + j) * 64 + lane] : gskip1[(i * NTH + j - NTH) * 64 + lane]; }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NOT; ++i) {
#pragma unroll
            for (int j = 0; j < NT; ++j) { sk[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
        }
    }
    __syncthreads(); // every wave has read its last B operand: the tile may be overwritten
    // epilogue: + bias (+ skip), ReLU; D layout of the 16x16 MFMA: lane (n = lane & 15, kg) holds output channels 16 * ot + 4 * kg + r at pixel n
#pragma unroll
    for (int i = 0; i < NOT; ++i) {
        const int ocb = 16 * (ot0 + i) + 4 * kg;
        const int chunk = ocb >> 3, half = (ocb >> 2) & 1;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const f32x4 skv = sk[i][j];
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = acc[i][j][r] + biasv[i][r];
                x = x + skv[r]; // without a skip: + 0 only turns -0 into +0, which the ReLU does anyway
                v[r] = x > 0.0f ? x : 0.0f;
            }
            if (gkeep0) {
                const f32x4 v4 = f32x4{v[0], v[1], v[2], v[3]};
                if (j < NTH) { gkeep0[(i * NTH + j) * 64 + lane] = v4; } else { gkeep1[(i * NTH + j - NTH) * 64 + lane] = v4; }
            }
            const int q = px.q[j];
            if (gout) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { if (q >= 0) { __builtin_nontemporal_store(v[r], &gout[(ocb + r) * G::P + q]); } }
            } else if (out_f32) {
                const int d = q < 0 ? G::NPOS : (q / G::BW + 1) * PW + (q % G::BW) + 1;
#pragma unroll
                for (int r = 0; r < 4; ++r) { ((LdsFloat*)tile)[(ocb + r) * G::CS + d] = v[r]; }
            } else {
                bf16x4 hi, lo;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    hi[r] = static_cast<__bf16>(v[r]);
                    lo[r] = static_cast<__bf16>(v[r] - static_cast<float>(hi[r]));
                }
                const int off = actByteW<CH>(px.dst[j], chunk) + half * 8;
                *(LdsBf16x4*)(tile + off) = hi;
                *(LdsBf16x4*)(tile + G::kBufBytes + off) = lo;
            }
        }
    }
}

// All layers for the NOT oc-tiles from ot0 and the NT pixel tiles from tile0 (CORNER: the last of them is the corner tile) on wave `wave`
template <class G, int H, int W, int NT, bool CORNER>
__device__ __forceinline__ void towerRunBf16Wide(LdsByte* lt, const uint4* __restrict__ wfrag, const float* __restrict__ params, const TowerArgsBf16& ta, float* __restrict__ gx,
                                                 float* __restrict__ gt, bool out_f32, float* __restrict__ gout, int lane, int wave, int ot0, int tile0)
{
    constexpr int PW = G::PW;
    PixSetBf16<NT> px;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        px.q[j] = kTileMap<H, W>.q[(tile0 + j) * 16 + (lane & 15)];
        const int q = px.q[j] < 0 ? 0 : px.q[j];
        px.src[j] = (q / W) * PW + (q % W);
        px.dst[j] = px.q[j] < 0 ? G::kDump : (q / W + 1) * PW + (q % W) + 1;
    }
    GlbF32x4* k0 = (GlbF32x4*)gx + size_t(wave) * G::NOT * G::NTH * 64; // the wave's part of x
    GlbF32x4* k1 = (GlbF32x4*)gt + size_t(wave) * G::NOT * G::NTH * 64;
    GlbCU32x4* wfr = (GlbCU32x4*)wfrag;
    GlbCF32x4* par4 = (GlbCF32x4*)params; // (bias offsets are multiples of 4 floats: the blob's arrays are 16-byte aligned)
    u32x4 ring[G::D][G::NOT][2];
    // stem: planes -> x (kept for the first block's skip)
    wideLayerBf16<G, NT, CORNER, 1, false>(lt, nullptr, nullptr, k0, k1, false, nullptr, wfr + ta.w_off[0], wfr + ta.w_off[1], par4 + ta.b_off[0] / 4, lane, ot0, px, false, ring);
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l < ta.nlayers; ++l) { // residual blocks: t = relu(conv1(x)); x = relu(conv2(t) + x)
        const bool second = ((l - 1) & 1) != 0, last = l + 1 == ta.nlayers, keep = second && !last;
        wideLayerBf16<G, NT, CORNER, G::KB, true>(lt, second ? k0 : nullptr, second ? k1 : nullptr, keep ? k0 : nullptr, keep ? k1 : nullptr, last && out_f32, last ? gout : nullptr,
                                                  wfr + ta.w_off[l], last ? nullptr : wfr + ta.w_off[l + 1], par4 + ta.b_off[l] / 4, lane, ot0, px, true, ring);
        __syncthreads();
    }
}

// The body for sample `b`, run by all 512 threads of a workgroup: input = bit-packed planes (cin0 <= 32 channels).  `tile` = Bf16WideGeo::kTileBytes of LDS;
// gx, gt = this workgroup's two blocks of C x P floats in global memory.  out != nullptr: the last activations as f32 NCHW to out + b * C * P; else they stay
// in the tile as f32 padded planes (channel stride Bf16WideGeo::CS, row stride W + 2), whose pointer is returned.
template <int H, int W, int C>
__device__ __forceinline__ float* towerBodyBf16Wide(const unsigned* __restrict__ in_bits, const uint4* __restrict__ wfrag, const float* __restrict__ params,
                                                    const TowerArgsBf16& ta, float* __restrict__ gx, float* __restrict__ gt, float* __restrict__ out, int b, int tid, char* tile)
{
    using G = Bf16WideGeo<H, W, C>;
    constexpr int P = G::P, PW = G::PW, W32 = (P + 31) / 32;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    LdsByte* lt = (LdsByte*)tile;
    for (int i = tid; i < 2 * G::kBufBytes / 16; i += 512) { ((__attribute__((address_space(3))) u32x4*)lt)[i] = u32x4{0, 0, 0, 0}; }
    __syncthreads();
    {
        const unsigned* bits = in_bits + size_t(b) * ta.cin0 * W32;
        for (int i = tid; i < ta.cin0 * P; i += 512) {
            const int c = i / P, p = i - c * P;
            if ((bits[c * W32 + (p >> 5)] >> (p & 31)) & 1u) {
                const int pos = (p / W + 1) * PW + (p % W) + 1;
                *(__attribute__((address_space(3))) unsigned short*)(lt + actByteW<G::CH>(pos, c >> 3) + (c & 7) * 2) = 0x3F80; // bf16 1.0 (hi only: the planes are 0 / 1)
            }
        }
    }
    __syncthreads();
    float* gout = out ? out + size_t(b) * C * P : nullptr;
    if constexpr (G::WP == 1) { // wave w: the NOT oc-tiles from w * NOT, all pixel tiles
        towerRunBf16Wide<G, H, W, G::NT, G::kCorner>(lt, wfrag, params, ta, gx, gt, !out, gout, lane, wave, wave * G::NOT, 0);
    } else { // wave w: oc-tile w % WO, pixel group w / WO (the same number of barriers on either side)
        const int ot0 = (wave % G::WO) * G::NOT;
        if (wave < G::WO) { towerRunBf16Wide<G, H, W, G::groupTiles(0), false>(lt, wfrag, params, ta, gx, gt, !out, gout, lane, wave, ot0, 0); }
        else { towerRunBf16Wide<G, H, W, G::groupTiles(1), G::kCorner>(lt, wfrag, params, ta, gx, gt, !out, gout, lane, wave, ot0, G::groupTiles(0)); }
    }
    return reinterpret_cast<float*>(tile);
}

} // namespace mz
