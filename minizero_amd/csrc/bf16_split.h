// Host side of the split-bf16 operands of the opt-in bf16x3 towers (net_bf16_body.h, net_bf16_wide_body.h): the rounding that turns an f32 weight into
// hi = bf16(v), lo = bf16(v - hi), and where a weight's two halves lie in a layer's A fragments.  No HIP in here: tests/csrc/bf16_split_check.cpp
// compiles it with g++ and the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mz {

// f32 -> bf16, round to nearest, ties to even (what the device's float -> __bf16 conversion does); inf stays inf, a nan stays a (quiet) nan
inline uint16_t bf16Rne(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) { return static_cast<uint16_t>((u >> 16) | ((u & 0x007FFFFFu) ? 0x0040u : 0u)); } // inf / nan: truncate
    u += 0x7FFFu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
}
inline float bf16ToFloat(uint16_t h)
{
    const uint32_t u = static_cast<uint32_t>(h) << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// v ~ hi + lo with 16 mantissa bits together: |v - (hi + lo)| <= 2^-16 |v| while lo stays a normal number
inline void bf16Split(float v, uint16_t* hi, uint16_t* lo)
{
    *hi = bf16Rne(v);
    *lo = bf16Rne(v - bf16ToFloat(*hi));
}

// A layer's fragments: [tap][oc-tile][k-block][hi, lo][lane][8] bf16, OT = ceil(cout / 16) oc-tiles, KB = ceil(cin / 32) k-blocks per tap; lane = 16 * kg + m
// holds W'[oc = 16 * ot + m][c = 32 * kb + 8 * kg + j][tap] in its element j — one dwordx4 load per lane is the A operand of one v_mfma_f32_16x16x32_bf16.
inline size_t bf16FragElems(int OT, int KB) { return size_t(9) * OT * KB * 2 * 64 * 8; }
// index (in bf16 elements) of the hi (hl = 0) or lo (hl = 1) half of W'[oc][c][tap]
inline size_t bf16FragIndex(int OT, int KB, int tap, int oc, int c, int hl)
{
    const int ot = oc >> 4, m = oc & 15, kb = c >> 5, kg = (c >> 3) & 3, j = c & 7;
    return ((((size_t(tap) * OT + ot) * KB + kb) * 2 + hl) * 64 + 16 * kg + m) * 8 + j;
}

} // namespace mz
