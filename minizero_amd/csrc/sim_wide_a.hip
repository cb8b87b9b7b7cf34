// instances of the wide simulation kernel, part 0 (sim_wide.inc) + the host side of all parts
#define MZ_SIM_WIDE_PART 0
#define MZ_SIM_WIDE_CASES(X) X(f32, 9, 9, 32, 128, 2) X(f32, 9, 9, 32, 32, 2) X(f32, 7, 7, 32, 128, 1) X(f32, 13, 13, 32, 64, 3)
#include "sim_wide.inc"

namespace mz {

#define MZ_SIM_WIDE_DECL(n) MZ_SIM_WIDE_SIG(n);
MZ_SIM_WIDE_PARTS(MZ_SIM_WIDE_DECL)
#undef MZ_SIM_WIDE_DECL

static bool simWideAny(int H, int W, int c0q, int C, int cpl, int prec, const SimArgs* d_args, int games, const uint8_t* d_rot, int sim0, int nsims, int host_start, int lf, size_t lds,
                       hipStream_t s, size_t* tile_bytes, int* rc, int* spec_words = nullptr)
{
#define MZ_SIM_WIDE_TRY(n) || MZ_SIM_WIDE_FN(n)(H, W, c0q, C, cpl, prec, d_args, games, d_rot, sim0, nsims, host_start, lf, lds, s, tile_bytes, rc, spec_words)
    return false MZ_SIM_WIDE_PARTS(MZ_SIM_WIDE_TRY);
#undef MZ_SIM_WIDE_TRY
}

// The LDS plan of sim_kernel_wide for a search of n simulations on a board of board_n x board_n points: false = no instance, or the mandatory blocks do not fit.
// *lf = the optional blocks that fit, in the order of what they buy (superko table, the leaf's block beside the heads, path speculation); *lds = the bytes to ask for
// env_kind: GameKind (the kernels take its rules argument, game_kind.h rulesArg).  The instance is the one of the network's precision: the bf16x3 kernels' tile
// is another size (9x9 x 256: 128 KB against the f32 tile's 124), so the same search may keep fewer optional blocks, or have no plan where the f32 tower has one.
bool Net::simWidePlan(int board_n, int env_kind, int num_simulation, const HeadParams& hp, int channels, int W32, size_t leaf_bytes, size_t scratch_bytes, int* lf, size_t* lds,
                      size_t* tile_bytes_out) const
{
    TowerArgs ta;
    int c0q = 0;
    if (desc_.type != 0 || !makeWideArgs(repr_, true, &ta, &c0q)) { return false; }
    const int H = desc_.hidden_channel_height, W = desc_.hidden_channel_width, C = desc_.num_hidden_channels;
    if (H != board_n || W != board_n) { return false; }
    const int cpl = rulesArg(env_kind, board_n);
    size_t tile_bytes = 0;
    int rc = MZ_OK, spec_words = kSpecWords;
    if (precision_ == 1 && !bf16Supported()) { return false; }
    if (!simWideAny(H, W, c0q, C, cpl, precision_, nullptr, 0, nullptr, 0, 0, 0, 0, 0, nullptr, &tile_bytes, &rc, &spec_words)) { return false; }
    const size_t rcp_n = size_t(num_simulation) + 5, max_depth = size_t(num_simulation) + 3, A = desc_.action_size;
    const size_t heads = (size_t(hp.PC) * hp.P + hp.P + hp.VH + hp.A + 16) * sizeof(float);
    size_t need = tile_bytes + rcp_n * sizeof(double) + (2 * max_depth + 2 + ((simXchgWords(int(A), channels, W32) + 1) & ~size_t(1))) * sizeof(float) + heads + 16;
    const size_t cap = size_t(160) * 1024;
    if (need > cap || scratch_bytes > tile_bytes) { return false; }
    int f = 0;
    const size_t seen = size_t(kGoSeenCap) * sizeof(uint64_t);
    if (cpl > 0 && need + seen <= cap) { f |= 2; need += seen; } // (the superko table and the leaf's block are Go's)
    // (the walk's speculation before the leaf's block: it is what keeps the slowest game of a launch short — 9x9 x 256 without it: select + leaf 26 us on average,
    //  98 us in the deepest game, and a launch lasts as long as its slowest game)
    const size_t spec = rcp_n * (sizeof(double) + sizeof(float)) + size_t(spec_words) * sizeof(int) + 8;
    if (need + spec <= cap) { f |= 1; need += spec; }
    const bool beside = hp.VH <= 256 && (hp.PC + 1) * hp.P <= 384 && hp.A <= 384; // waves 6 and 7 have no share of the heads (sim_az_body.h)
    const size_t leaf = (leaf_bytes + 7) & ~size_t(7);
    if (beside && (f & 2) && need + leaf <= cap) { f |= 4; need += leaf; }
    if (lf) { *lf = f; }
    if (lds) { *lds = need; }
    if (tile_bytes_out) { *tile_bytes_out = tile_bytes; }
    return true;
}

int Net::simLaunchWide(const SimArgs& a, const GoDevView& gv, int max_depth, const uint8_t* d_rot, int sim0, int nsims, bool host_start, int lf, size_t lds, bool* launched)
{
    *launched = false;
    int rc = uploadSimArgs(a);
    if (rc) { return rc; }
    int c0q = 16 * repr_[0].cq;
    const int H = desc_.hidden_channel_height, W = desc_.hidden_channel_width, C = desc_.num_hidden_channels;
    if (simWideAny(H, W, c0q, C, rulesArg(gv.kind, gv.n), precision_, reinterpret_cast<const SimArgs*>(sim_args_.p), gv.games, d_rot, sim0, nsims, host_start ? 1 : 0, lf, lds, stream_, nullptr, &rc)) {
        *launched = rc == MZ_OK;
    }
    return rc;
}

} // namespace mz
