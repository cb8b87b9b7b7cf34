// Stand-alone check of minizero_amd/csrc/bf16_split.h (built by tests/test_bf16_split.py with -fsanitize=address,undefined): the rounding of the split-bf16
// operands and the place of every weight in a layer's A fragments.  Prints one line per failed check; exit status = the number of failed checks.
#include "bf16_split.h"
#include <cmath>
#include <cstdio>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) { ++g_fail; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static float fromBits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main()
{
    using namespace mz;
    // round to nearest, ties to even: 0x....8000 is the tie
    CHECK(bf16Rne(fromBits(0x3F808000u)) == 0x3F80, "tie above an even mantissa rounds down");
    CHECK(bf16Rne(fromBits(0x3F818000u)) == 0x3F82, "tie above an odd mantissa rounds up");
    CHECK(bf16Rne(fromBits(0x3F808001u)) == 0x3F81, "above the tie rounds up");
    CHECK(bf16Rne(fromBits(0x3F807FFFu)) == 0x3F80, "below the tie rounds down");
    CHECK(bf16Rne(fromBits(0xBF818000u)) == 0xBF82, "ties to even for negative values");
    CHECK(bf16Rne(fromBits(0x3FFF8000u)) == 0x4000, "a tie that carries into the exponent");
    CHECK(bf16Rne(fromBits(0x7F7FFFFFu)) == 0x7F80, "FLT_MAX rounds to inf");
    // +-0, denormals, inf / nan
    CHECK(bf16Rne(0.0f) == 0x0000 && bf16Rne(-0.0f) == 0x8000, "+-0 keep their sign");
    CHECK(bf16Rne(fromBits(0x00010000u)) == 0x0001 && bf16Rne(fromBits(0x80400000u)) == 0x8040, "denormals that fit pass through");
    CHECK(bf16Rne(fromBits(0x00000001u)) == 0x0000 && bf16Rne(fromBits(0x00018000u)) == 0x0002, "denormals round like every other value");
    CHECK(bf16Rne(fromBits(0x7F800000u)) == 0x7F80 && bf16Rne(fromBits(0xFF800000u)) == 0xFF80, "inf passes through");
    CHECK((bf16Rne(fromBits(0x7FC00000u)) & 0x7FFF) > 0x7F80 && (bf16Rne(fromBits(0x7F800001u)) & 0x7FFF) > 0x7F80 && (bf16Rne(fromBits(0xFFFFFFFFu)) & 0x7FFF) > 0x7F80,
          "a nan stays a nan");
    for (uint32_t h = 0; h < 0x10000u; ++h) {
        const float f = bf16ToFloat(static_cast<uint16_t>(h));
        if (f == f) { CHECK(bf16Rne(f) == h, "bf16 value %04x does not survive the round trip", h); }
    }
    // |v - (hi + lo)| <= 2^-16 |v| over a fixed sample: a counter-based generator over sign, exponents -40 .. 40 and all 23 mantissa bits, and the network's range
    uint64_t s = 0x9E3779B97F4A7C15ull;
    double worst = 0.0;
    for (int i = 0; i < 2000000; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t mant = static_cast<uint32_t>(s >> 41), sign = static_cast<uint32_t>(s >> 40) & 1u;
        const int e = (i & 1) ? 127 - 8 + static_cast<int>((s >> 20) % 9) : 127 - 40 + static_cast<int>((s >> 20) % 81);
        const float v = fromBits((sign << 31) | (static_cast<uint32_t>(e) << 23) | mant);
        uint16_t hi, lo;
        bf16Split(v, &hi, &lo);
        const double err = std::fabs(double(v) - (double(bf16ToFloat(hi)) + double(bf16ToFloat(lo))));
        const double rel = err / std::fabs(double(v));
        worst = rel > worst ? rel : worst;
        if (rel > std::ldexp(1.0, -16)) { CHECK(false, "v = %a: hi + lo off by %.3g |v|", v, rel); break; }
    }
    printf("split: worst |v - (hi + lo)| / |v| = 2^%.2f\n", std::log2(worst));
    // the fragment index: a bijection onto [0, 9 * C * C * 2) for the tower layers of 64, 128 and 256 channels (and onto the stem's fragments: 32 padded inputs)
    const int shapes[][2] = {{64, 64}, {128, 128}, {256, 256}, {32, 64}, {32, 256}}; // (input channels, output channels)
    for (const auto& sh : shapes) {
        const int cin = sh[0], cout = sh[1], OT = cout / 16, KB = cin / 32;
        const size_t n = bf16FragElems(OT, KB);
        CHECK(n == size_t(9) * cin * cout * 2, "%d -> %d: %zu elements", cin, cout, n);
        std::vector<unsigned char> seen(n, 0);
        bool ok = true;
        for (int t = 0; t < 9 && ok; ++t)
            for (int oc = 0; oc < cout && ok; ++oc)
                for (int c = 0; c < cin && ok; ++c)
                    for (int hl = 0; hl < 2; ++hl) {
                        const size_t i = bf16FragIndex(OT, KB, t, oc, c, hl);
                        if (i >= n || seen[i]) { ok = false; CHECK(false, "%d -> %d: (%d, %d, %d, %d) -> %zu is out of range or taken", cin, cout, t, oc, c, hl, i); break; }
                        seen[i] = 1;
                    }
        size_t count = 0;
        for (unsigned char b : seen) { count += b; }
        CHECK(count == n, "%d -> %d: %zu of %zu elements reached", cin, cout, count, n);
    }
    // 64 channels: the offsets of the builder this header was taken out of (Net::packBf16 before the one-tile tower: nested loops tap, oc-tile, k-block, hi / lo,
    // lane, element — recorded from that loop)
    struct { int t, oc, c, hl; size_t at; } lit[] = {{0, 0, 0, 0, 0}, {0, 1, 0, 0, 8}, {0, 0, 0, 1, 512}, {0, 0, 9, 1, 641}, {1, 16, 32, 0, 11264}, {3, 5, 31, 1, 25519},
                                                     {4, 37, 50, 0, 38186}, {8, 63, 63, 1, 73727}};
    for (const auto& l : lit) { CHECK(bf16FragIndex(4, 2, l.t, l.oc, l.c, l.hl) == l.at, "64 channels: (%d, %d, %d, %d) -> %zu, the builder had %zu", l.t, l.oc, l.c, l.hl, bf16FragIndex(4, 2, l.t, l.oc, l.c, l.hl), l.at); }
    // one lane's dwordx4 is 8 consecutive input channels of one output channel
    for (int j = 1; j < 8; ++j) { CHECK(bf16FragIndex(16, 8, 5, 200, 96 + j, 1) == bf16FragIndex(16, 8, 5, 200, 96, 1) + j, "a lane's elements are consecutive"); }
    printf(g_fail ? "%d checks failed\n" : "bf16_split: ok\n", g_fail);
    return g_fail;
}
