// gfx950 kernel of the tree read-out (tree_read.h).  One wave64 per game, built like pool.hip (-ffp-contract=off; nothing is computed here anyway: the values are
// copied).  Plain loads and stores, no atomics; every loop is bounded by the capacity and by num_children, and a wave never waits for another.
#include "tree_read.h"
#include <cstring>

namespace mz {

namespace {

// what lanes of this wave stored is what its next loads see
__device__ __forceinline__ void treeWaveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// entry e of the queue: the fields, and in `src` where the node's children start (all the queue needs of the node once it is written)
__device__ __forceinline__ void treeWriteEntry(int* gi, float* gf, int* src, int E, int e, const NodeRec& r, float logit, float noise, float value, int parent,
                                               int ordinal, int depth)
{
    gi[kTrParent * E + e] = parent;
    gi[kTrOrdinal * E + e] = ordinal;
    gi[kTrAction * E + e] = r.action;
    gi[kTrPlayer * E + e] = r.players & 0xFF;
    gi[kTrNumChildren * E + e] = r.num_children;
    gi[kTrDepth * E + e] = depth;
    gf[kTrCount * E + e] = r.count;
    gf[kTrMean * E + e] = r.mean;
    gf[kTrPolicy * E + e] = r.policy;
    gf[kTrLogit * E + e] = logit;
    gf[kTrNoise * E + e] = noise;
    gf[kTrValue * E + e] = value;
    gf[kTrReward * E + e] = r.reward;
    src[e] = r.first_child;
}

constexpr int kTreeStrides = 4; // strides of 64 children whose loads are in flight together (a 19x19 parent: 362 children, two turns)

// The queue is walked in batches: after one wave sync the lanes fetch (first child, number of children, depth) of up to 64 entries in one round trip; the
// entries of the batch are then served from registers, and what they append is only looked at by the next batch.  Per parent the records and cold fields of up
// to 256 children are requested before any of them is looked at, so an entry costs about one memory round trip instead of one per dependent load.
__global__ __launch_bounds__(64) void tree_read_kernel(PoolView pv, TreeReadView tv, const uint8_t* __restrict__ game_mask)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (game_mask && !game_mask[g]) { return; }
    const size_t base = size_t(g) * pv.cap;
    const int E = tv.cap;
    int* gi = tv.ints + size_t(g) * kTreeInts * E;
    float* gf = tv.floats + size_t(g) * kTreeFloats * E;
    int* src = tv.src + size_t(g) * E;
    bool over = E < 1;
    if (lane == 0 && !over) { treeWriteEntry(gi, gf, src, E, 0, pv.rec[base], pv.logit[base], pv.noise[base], pv.value[base], -1, 0, 0); }
    int head = 0, tail = 1, deepest = 0;
    while (!over && head < tail) { // head grows by at least one per turn and tail <= E: at most E turns
        treeWaveSync();            // the entries below `tail` were written by lanes of this wave
        const int batch = tail - head < 64 ? tail - head : 64;
        int my_fc = 0, my_nc = 0, my_depth = 0;
        if (lane < batch) {
            my_fc = src[head + lane];
            my_nc = gi[kTrNumChildren * E + head + lane];
            my_depth = gi[kTrDepth * E + head + lane];
        }
        for (int b = 0; b < batch && !over; ++b) {
            const int fc = __shfl(my_fc, b), nc = __shfl(my_nc, b), depth = __shfl(my_depth, b);
            if (nc <= 0) { continue; }
            if (fc < 1 || fc > pv.cap - nc) { over = true; break; } // a record this pool cannot hold: nothing past the game's nodes is read
            const size_t kids = base + fc;
            for (int i0 = 0; i0 < nc && !over; i0 += 64 * kTreeStrides) {
                NodeRec r[kTreeStrides];
                float lg[kTreeStrides], ns[kTreeStrides], vl[kTreeStrides];
                unsigned long long m[kTreeStrides];
                int total = 0;
#pragma unroll
                for (int k = 0; k < kTreeStrides; ++k) {
                    const int i = i0 + 64 * k + lane;
                    r[k] = NodeRec{};
                    lg[k] = ns[k] = vl[k] = 0.0f;
                    if (i < nc) { r[k] = pv.rec[kids + i]; lg[k] = pv.logit[kids + i]; ns[k] = pv.noise[kids + i]; vl[k] = pv.value[kids + i]; }
                }
#pragma unroll
                for (int k = 0; k < kTreeStrides; ++k) {
                    m[k] = __ballot(i0 + 64 * k + lane < nc && r[k].count > 0.0f); // MCTSNode::displayInTreeLog (ref mcts.h:27)
                    total += __popcll(m[k]);
                }
                if (total == 0) { continue; }
                if (total > E - tail) { over = true; break; }
#pragma unroll
                for (int k = 0; k < kTreeStrides; ++k) {
                    const int i = i0 + 64 * k + lane;
                    const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m[k] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m[k]), 0u)); // kept lanes below me
                    if ((m[k] >> lane) & 1ull) { treeWriteEntry(gi, gf, src, E, tail + rank, r[k], lg[k], ns[k], vl[k], head + b, i, depth + 1); }
                    tail += __popcll(m[k]);
                }
                deepest = depth + 1 > deepest ? depth + 1 : deepest;
            }
        }
        head += batch;
    }
    if (lane == 0) {
        int* info = tv.info + size_t(g) * 4;
        info[0] = over ? -1 : tail;
        info[1] = pv.num_nodes[g];
        info[2] = deepest;
        info[3] = 0;
        if (over) { *tv.err = MZ_ERR_CAPACITY; } // the pool's error flag; every wave that stores here stores the same word
    }
}

} // namespace

class TreeReaderImpl final : public TreeReader {
public:
    int init(int device, hipStream_t stream, const Pool& pool, int entries_per_game) override;
    int read(Pool& pool, int game, TreeSnapshot* out) override;

private:
    TreeReadView v_{};
    int device_ = 0, games_ = 0;
    hipStream_t stream_ = nullptr;
    DevBuf<int> ints_, src_, info_;
    DevBuf<float> floats_;
    DevBuf<uint8_t> d_mask_;
    PinBuf<uint8_t> h_mask_;
    PinBuf<int> h_ints_;     // one game's block + its info words
    PinBuf<float> h_floats_;
};

TreeReader* createTreeReader() { return new TreeReaderImpl(); }

#define RALLOC(buf, k) \
    if (!(buf).alloc(k)) { setError("tree: allocation of %zu elements failed (%s)", size_t(k), #buf); return MZ_ERR_DEVICE; }

int TreeReaderImpl::init(int device, hipStream_t stream, const Pool& pool, int entries_per_game)
{
    if (entries_per_game < 1) { setError("tree: bad capacity %d", entries_per_game); return MZ_ERR_ARG; }
    device_ = device;
    stream_ = stream;
    MZ_HIP(hipSetDevice(device));
    games_ = pool.v_.games;
    const size_t G = games_, E = entries_per_game;
    RALLOC(ints_, G * kTreeInts * E); RALLOC(floats_, G * kTreeFloats * E); RALLOC(src_, G * E); RALLOC(info_, G * 4);
    RALLOC(d_mask_, G); RALLOC(h_mask_, G); RALLOC(h_ints_, kTreeInts * E + 4); RALLOC(h_floats_, kTreeFloats * E);
    MZ_HIP(hipMemset(info_.p, 0, G * 4 * sizeof(int)));
    v_.cap = entries_per_game;
    v_.ints = ints_.p; v_.floats = floats_.p; v_.src = src_.p; v_.info = info_.p;
    return MZ_OK;
}

int TreeReaderImpl::read(Pool& pool, int game, TreeSnapshot* out)
{
    if (game < 0 || game >= games_ || !out) { setError("tree: game %d out of range", game); return MZ_ERR_ARG; }
    MZ_HIP(hipSetDevice(device_));
    MZ_HIP(hipStreamSynchronize(stream_)); // the pinned mask and staging of the previous read-out are free
    const size_t E = v_.cap;
    memset(h_mask_.p, 0, games_);
    h_mask_.p[game] = 1;
    MZ_HIP(hipMemcpyAsync(d_mask_.p, h_mask_.p, games_, hipMemcpyHostToDevice, stream_));
    v_.err = pool.errFlag();
    hipLaunchKernelGGL(tree_read_kernel, dim3(games_), dim3(64), 0, stream_, pool.v_, v_, d_mask_.p);
    MZ_HIP(hipGetLastError());
    MZ_HIP(hipMemcpyAsync(h_ints_.p, v_.ints + size_t(game) * kTreeInts * E, kTreeInts * E * sizeof(int), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipMemcpyAsync(h_ints_.p + kTreeInts * E, v_.info + size_t(game) * 4, 4 * sizeof(int), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipMemcpyAsync(h_floats_.p, v_.floats + size_t(game) * kTreeFloats * E, kTreeFloats * E * sizeof(float), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipStreamSynchronize(stream_));
    const int* info = h_ints_.p + kTreeInts * E;
    out->num_nodes = info[1];
    out->deepest = info[2];
    if (info[0] < 0) {
        out->entries = 0;
        (void)pool.checkError(); // takes the flag down again: the search itself is intact
        setError("tree: game %d has more visited nodes than the %d entries of the read-out", game, v_.cap);
        return MZ_ERR_CAPACITY;
    }
    const int n = info[0];
    out->entries = n;
    out->ints.resize(size_t(kTreeInts) * n);
    out->floats.resize(size_t(kTreeFloats) * n);
    for (int r = 0; r < kTreeInts; ++r) { memcpy(out->ints.data() + size_t(r) * n, h_ints_.p + r * E, n * sizeof(int)); }
    for (int r = 0; r < kTreeFloats; ++r) { memcpy(out->floats.data() + size_t(r) * n, h_floats_.p + r * E, n * sizeof(float)); }
    return MZ_OK;
}

} // namespace mz
