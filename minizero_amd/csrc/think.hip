// gfx950 kernels of the batched think (think.h).  One wave64 per game for the ordered parts (selection under virtual loss; expand + backup in batch order), one
// wave64 per (game, walk) for the parts that are independent per query (leaf position + planes, candidate list).  Built like pool.hip: -ffp-contract=off, the
// reference's formulas as written.  The leaf and candidate bodies are go_body.h's own, reached through views whose per-game arrays are offset so that the body's
// index `g` lands on the (game, walk) entry: the bodies and their existing instantiations stay as they are.
#include "think_body.h"
#include "go_body.h"
#include "net.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace mz {

namespace {

__global__ __launch_bounds__(64) void think_select_kernel(PoolView pv, ThinkView tv, int* __restrict__ err) { thinkSelectBody(pv, tv, blockIdx.x, threadIdx.x, err); }

// the views of (game g, walk q - g * B): what the bodies index by game and is kept per walk moves by q - g entries
__device__ __forceinline__ PoolView walkPool(PoolView pv, const ThinkView& tv, int g, int q)
{
    const ptrdiff_t d = q - g;
    pv.path_len = tv.path_len + d;
    pv.path = tv.path + d * pv.max_depth;
    pv.path_action = tv.path_action + d * pv.max_depth;
    pv.host_path_len = nullptr;
    pv.host_path_action = nullptr;
    return pv;
}

template <int CPL>
__global__ __launch_bounds__(64) void think_leaf_kernel(GoDevView v, PoolView pv, ThinkView tv)
{
    extern __shared__ uint64_t smem[];
    const int q = blockIdx.x, g = q / tv.B;
    if (tv.query[q] == 0) { return; }
    const ptrdiff_t d = q - g;
    v.feat = tv.feat + d * v.channels * v.W32;
    v.legal = tv.legal + d * v.LW;
    v.leaf_player = tv.leaf_player + d;
    v.terminal = tv.terminal + d;
    v.eval = tv.eval + d;
    leafBody<CPL>(v, walkPool(pv, tv, g, q), tv.rot[q], tv.slot[q], g, threadIdx.x, smem);
}

// the candidate body reads nothing that is kept per game: the (game, walk) index is its `g`
__global__ __launch_bounds__(64) void think_cand_kernel(GoDevView v, ThinkView tv, const float* __restrict__ policy, const float* __restrict__ logit,
                                                        const float* __restrict__ value, int* __restrict__ err)
{
    extern __shared__ uint64_t smem[];
    const int q = blockIdx.x;
    if (tv.query[q] == 0) { return; }
    v.legal = tv.legal; v.leaf_player = tv.leaf_player; v.terminal = tv.terminal; v.eval = tv.eval;
    azCandBody(v, policy, logit, value, tv.rot[q], tv.cand_count, tv.cand_action, tv.cand_policy, tv.cand_logit, tv.cand_player, tv.value, tv.reward, err, q,
               threadIdx.x, smem);
}

// mz_think_symmetries=8: the planes of query q under rotation r = blockIdx.y + 1, gathered from the planes the leaf kernel wrote under rotation 0 (row q of
// block 0) into row r * Q + q.  Every plane of every game of the table is a per-point bitmap — stones, history, to move, all on-board points — and the leaf
// bodies build the planes of rotation r as plane bit p <- position inv[r][p] (go_body.h), so one gather over the packed words gives their bits: lane l takes
// point p = 64 i + l of word i, the ballot over the lanes is the word, lane ch keeps plane ch's and stores its two halves (the last word of a plane may have
// one half only, and its bits past P stay 0, as the leaf bodies leave them).  inv[r][p] < P, so the word read is one of the row's W32.
__global__ __launch_bounds__(64) void think_sym_planes_kernel(GoDevView v, ThinkView tv, int Q)
{
    const int q = blockIdx.x, r = blockIdx.y + 1, lane = threadIdx.x;
    if (tv.query[q] == 0) { return; }
    const int P = v.P, W32 = v.W32, C = v.channels;
    const size_t row = size_t(C) * W32;
    const uint32_t* __restrict__ in = tv.feat + size_t(q) * row;
    uint32_t* __restrict__ out = tv.feat + (size_t(r) * Q + q) * row;
    const uint16_t* __restrict__ map = v.inv + size_t(r) * P;
    for (int i = 0; 64 * i < P; ++i) {
        const int p = 64 * i + lane;
        const int s = p < P ? map[p] : 0;
        uint64_t mine = 0;
        for (int ch = 0; ch < C; ++ch) {
            const uint64_t bal = __ballot(p < P && ((in[ch * W32 + (s >> 5)] >> (s & 31)) & 1));
            if (lane == ch) { mine = bal; }
        }
        if (lane < C) {
            if (2 * i < W32) { out[lane * W32 + 2 * i] = static_cast<uint32_t>(mine); }
            if (2 * i + 1 < W32) { out[lane * W32 + 2 * i + 1] = static_cast<uint32_t>(mine >> 32); }
        }
    }
}

// mz_think_symmetries=8: policy, logit and value of query q in the board's own frame.  Row r * Q + q holds the network's outputs on the planes of rotation r;
// action a's entry there is fwd[r][a] (getRotateAction; the pass maps to itself).  The sum is the contract: f32, r = 0, 1, .., 7 in that order
// from the r = 0 term, one rounding per addition (the unit is built with -ffp-contract=off), then times 0.125f.  Lanes over the actions: a < A and
// fwd[r][a] < A, so no access leaves a row.
__global__ __launch_bounds__(64) void think_sym_reduce_kernel(GoDevView v, ThinkView tv, int Q, const float* __restrict__ policy, const float* __restrict__ logit,
                                                              const float* __restrict__ value, float* __restrict__ policy_out, float* __restrict__ logit_out,
                                                              float* __restrict__ value_out)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    if (tv.query[q] == 0) { return; }
    const int A = v.A;
    for (int a = lane; a < A; a += 64) {
        const int f0 = v.fwd[a];
        float p = policy[size_t(q) * A + f0], l = logit[size_t(q) * A + f0];
#pragma unroll
        for (int r = 1; r < 8; ++r) {
            const size_t at = (size_t(r) * Q + q) * A + v.fwd[size_t(r) * A + a];
            p = p + policy[at];
            l = l + logit[at];
        }
        policy_out[size_t(q) * A + a] = p * 0.125f;
        logit_out[size_t(q) * A + a] = l * 0.125f;
    }
    if (lane == 0) {
        float s = value[q];
#pragma unroll
        for (int r = 1; r < 8; ++r) { s = s + value[size_t(r) * Q + q]; }
        value_out[q] = s * 0.125f;
    }
}

// afterNNEvaluation per query in batch order (zero_actor.cpp:149-156): expand + backup, then the leaf's virtual loss comes off every node of the path — that
// also clears what the duplicates of this query added (a path to a node is unique)
__global__ __launch_bounds__(64) void think_expand_backup_kernel(PoolView pv, ThinkView tv, int* __restrict__ err)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const size_t base = size_t(g) * pv.cap;
    float* vls = tv.vl + base;
    const int bs = tv.status[g * 4 + 1];
    int last = -1;
    for (int b = 0; b < bs && b < tv.B; ++b) {
        const int q = g * tv.B + b;
        if (tv.query[q] == 0) { continue; }
        const ptrdiff_t d = q - g;
        thinkWaveSync(); // what the query before this one wrote
        expandBackupBody(walkPool(pv, tv, g, q), tv.cand_count + d, tv.cand_action + d * pv.A, tv.cand_policy + d * pv.A, tv.cand_logit + d * pv.A, tv.cand_player + d,
                         tv.value + d, tv.reward + d, tv.slot[q], err, g, lane, nullptr);
        const int len = tv.path_len[q];
        const int* path = tv.path + size_t(q) * pv.max_depth;
        const float lv = len > 0 ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(vls[path[len - 1]]))) : 0.0f; // getVirtualLoss() of the leaf (:154), read before any of it comes off
        for (int k = lane; k < len; k += 64) { vls[path[k]] -= lv; }
        last = q;
    }
    thinkWaveSync();
    if (lane == 0) {
        const int count = static_cast<int>(pv.rec[base].count);
        tv.status[g * 4 + 0] = count;
        // the query that completed the search: handleSearchDone() ran while its path still carried one virtual loss (:96 before :154) — the host puts it back for the decision
        int child = -1;
        if (last >= 0 && count == tv.n + 1) { child = tv.path_len[last] >= 2 ? tv.path[size_t(last) * pv.max_depth + 1] - pv.rec[base].first_child : -1; }
        tv.status[g * 4 + 3] = (last >= 0 && count == tv.n + 1) ? child : -2;
    }
}

__global__ __launch_bounds__(64) void think_reroot_kernel(PoolView pv, GoDevView gv, float* __restrict__ vl, const int* __restrict__ args, int* newidx, int* work, int work_cap,
                                                          int* __restrict__ status, int* __restrict__ err)
{
    thinkRerootBody(pv, gv, vl, args, newidx, work, work_cap, status, blockIdx.x, threadIdx.x, err);
}

} // namespace

class ThinkDeviceImpl final : public ThinkDevice {
public:
    int init(int device, hipStream_t stream, const Pool& pool, const GoDevView& gv, int B, const mz_search_cfg& cfg, bool reuse, int symmetries) override;
    int clearAsync() override;
    uint8_t* hostRot() override { return h_rot_.p; }
    int stepAsync(Pool& pool, const GoDevView& gv, Net& net) override;
    const int* hostStatus() const override { return h_status_.p; }
    int* hostReroot() override { return h_reroot_.p; }
    int reroot(Pool& pool, const GoDevView& gv) override;
    const int* hostRerootStatus() const override { return h_reroot_.p + size_t(games_) * 2; }

private:
    ThinkView v_{};
    int device_ = 0, games_ = 0, sym_ = 1;
    hipStream_t stream_ = nullptr;
    DevBuf<float> vl_, bias_tab_, eval_, cand_f_, out_; // out_: the heads' outputs per (game, walk): policy, logit [Q][A], value [Q] (mz_think_symmetries=8: [8 Q][A], [8 Q])
    DevBuf<float> avg_;                                 // mz_think_symmetries=8 only: the averages the candidate kernel reads, laid out as out_ is with the key at 1
    DevBuf<double> sqrt_tab_;
    DevBuf<int> walk_i_, status_, leaf_i_, cand_i_;
    DevBuf<uint8_t> d_rot_;
    PinBuf<uint8_t> h_rot_;
    PinBuf<int> h_status_;
    DevBuf<uint32_t> feat_;
    DevBuf<uint64_t> legal_;
    // mz_think_reuse_tree only: the new index per node, the worklist of expanded kept nodes, (action, player) + status per game
    DevBuf<int> newidx_, work_, d_reroot_;
    PinBuf<int> h_reroot_;
    int work_cap_ = 0;
};

ThinkDevice* createThinkDevice() { return new ThinkDeviceImpl(); }

#define TALLOC(buf, k) \
    if (!(buf).alloc(k)) { setError("think: allocation of %zu elements failed (%s)", size_t(k), #buf); return MZ_ERR_DEVICE; }

int ThinkDeviceImpl::init(int device, hipStream_t stream, const Pool& pool, const GoDevView& gv, int B, const mz_search_cfg& cfg, bool reuse, int symmetries)
{
    if (B < 2 || B > kThinkMaxBatch) { setError("think: batch size %d out of range", B); return MZ_ERR_ARG; }
    if (symmetries != 1 && symmetries != 8) { setError("think: mz_think_symmetries=%d (1 or 8)", symmetries); return MZ_ERR_ARG; }
    if (symmetries == 8 && gv.channels > 64) { setError("think: mz_think_symmetries=8 gathers at most 64 planes, the game has %d", gv.channels); return MZ_ERR_ARG; }
    sym_ = symmetries;
    device_ = device;
    stream_ = stream;
    MZ_HIP(hipSetDevice(device));
    const PoolView& pv = pool.v_;
    const size_t G = pv.games, Q = G * B, MD = pv.max_depth, A = pv.A;
    games_ = pv.games;
    ThinkView& t = v_;
    t.B = B; t.n = cfg.num_simulation; t.tab_n = cfg.num_simulation + B + 2;
    TALLOC(vl_, G * pv.cap); TALLOC(walk_i_, 2 * Q * MD + 3 * Q); TALLOC(status_, 4 * G); TALLOC(h_status_, 4 * G);
    TALLOC(d_rot_, Q); TALLOC(h_rot_, Q);
    TALLOC(bias_tab_, t.tab_n); TALLOC(sqrt_tab_, t.tab_n);
    const size_t S = sym_; // blocks of the feature buffer and of the heads' outputs: [S][games][B]
    TALLOC(feat_, S * Q * gv.channels * gv.W32); TALLOC(legal_, Q * gv.LW); TALLOC(leaf_i_, 2 * Q); TALLOC(eval_, Q);
    TALLOC(cand_i_, 2 * Q + Q * A); TALLOC(cand_f_, 2 * Q + 2 * Q * A); TALLOC(out_, S * (2 * Q * A + Q));
    if (sym_ == 8) { TALLOC(avg_, 2 * Q * A + Q); }
    t.vl = vl_.p;
    t.path = walk_i_.p; t.path_action = walk_i_.p + Q * MD; t.path_len = walk_i_.p + 2 * Q * MD; t.query = t.path_len + Q; t.slot = t.query + Q;
    t.rot = d_rot_.p;
    t.status = status_.p;
    t.feat = feat_.p; t.legal = legal_.p; t.leaf_player = leaf_i_.p; t.terminal = leaf_i_.p + Q; t.eval = eval_.p;
    t.cand_count = cand_i_.p; t.cand_player = cand_i_.p + Q; t.cand_action = cand_i_.p + 2 * Q;
    t.value = cand_f_.p; t.reward = cand_f_.p + Q; t.cand_policy = cand_f_.p + 2 * Q; t.cand_logit = cand_f_.p + 2 * Q + Q * A;
    // PUCT tables as Pool::init builds them (ref mcts.cpp:57-58), for N up to n + B
    std::vector<float> bias(t.tab_n);
    std::vector<double> sq(t.tab_n);
    for (int N = 0; N < t.tab_n; ++N) {
        const float ratio = (1 + N + cfg.puct_base) / cfg.puct_base;
        bias[N] = cfg.puct_init + ::log(static_cast<double>(ratio));
        sq[N] = ::sqrt(static_cast<double>(N));
    }
    MZ_HIP(hipMemcpy(bias_tab_.p, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
    MZ_HIP(hipMemcpy(sqrt_tab_.p, sq.data(), sq.size() * sizeof(double), hipMemcpyHostToDevice));
    t.bias_tab = bias_tab_.p;
    t.sqrt_tab = sqrt_tab_.p;
    MZ_HIP(hipMemset(walk_i_.p, 0, walk_i_.n * sizeof(int)));
    MZ_HIP(hipMemset(status_.p, 0, status_.n * sizeof(int)));
    MZ_HIP(hipMemset(feat_.p, 0, feat_.n * sizeof(uint32_t))); // the forward runs over every (game, walk) entry: the ones no query ever wrote hold empty planes
    MZ_HIP(hipMemset(d_rot_.p, 0, Q)); // (mz_think_symmetries=8 never uploads the draws: every leaf and candidate list under rotation 0)
    memset(h_rot_.p, 0, Q);
    memset(h_status_.p, 0, 4 * G * sizeof(int));
    if (reuse) {
        work_cap_ = cfg.num_simulation + 2; // a search expands at most n + 1 nodes
        TALLOC(newidx_, G * pv.cap); TALLOC(work_, G * work_cap_); TALLOC(d_reroot_, 4 * G); TALLOC(h_reroot_, 4 * G);
        MZ_HIP(hipMemset(d_reroot_.p, 0, d_reroot_.n * sizeof(int)));
        for (size_t g = 0; g < G; ++g) { h_reroot_.p[g * 2] = -2; h_reroot_.p[g * 2 + 1] = 0; h_reroot_.p[(G + g) * 2] = 0; h_reroot_.p[(G + g) * 2 + 1] = 1; }
    }
    return clearAsync();
}

int ThinkDeviceImpl::reroot(Pool& pool, const GoDevView& gv)
{
    if (!h_reroot_.p) { setError("think: the re-root was not set up (mz_think_reuse_tree=false)"); return MZ_ERR_STATE; }
    MZ_HIP(hipSetDevice(device_));
    const size_t G = games_;
    MZ_HIP(hipMemcpyAsync(d_reroot_.p, h_reroot_.p, G * 2 * sizeof(int), hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(think_reroot_kernel, dim3(games_), dim3(64), 0, stream_, pool.v_, gv, vl_.p, d_reroot_.p, newidx_.p, work_.p, work_cap_, d_reroot_.p + G * 2,
                       pool.errFlag());
    MZ_HIP(hipGetLastError());
    MZ_HIP(hipMemcpyAsync(h_reroot_.p + G * 2, d_reroot_.p + G * 2, G * 2 * sizeof(int), hipMemcpyDeviceToHost, stream_));
    MZ_HIP(hipStreamSynchronize(stream_));
    for (size_t g = 0; g < G; ++g) { h_reroot_.p[g * 2] = -2; }
    return pool.checkError();
}

int ThinkDeviceImpl::clearAsync()
{
    MZ_HIP(hipMemsetAsync(vl_.p, 0, vl_.n * sizeof(float), stream_));
    return MZ_OK;
}

int ThinkDeviceImpl::stepAsync(Pool& pool, const GoDevView& gv, Net& net)
{
    const PoolView& pv = pool.v_;
    const int Q = games_ * v_.B;
    const size_t R = size_t(sym_) * Q; // rows of the forward
    float *d_policy = out_.p, *d_logit = out_.p + R * pv.A, *d_value = out_.p + 2 * R * pv.A;
    if (sym_ == 1) { MZ_HIP(hipMemcpyAsync(d_rot_.p, h_rot_.p, Q, hipMemcpyHostToDevice, stream_)); }
    hipLaunchKernelGGL(think_select_kernel, dim3(games_), dim3(64), 0, stream_, pv, v_, pool.errFlag());
    MZ_HIP(hipGetLastError());
    const size_t leaf_smem = gv.kind == kGo ? goLeafSmemBytes(gv, pv.max_depth) : 0;
    if (!forRulesArg(rulesArg(gv.kind, gv.n), [&](auto cpl) { hipLaunchKernelGGL(think_leaf_kernel<cpl()>, dim3(Q), dim3(64), leaf_smem, stream_, gv, pv, v_); })) {
        setError("think: board too large");
        return MZ_ERR_ARG;
    }
    MZ_HIP(hipGetLastError());
    if (sym_ == 8) {
        hipLaunchKernelGGL(think_sym_planes_kernel, dim3(Q, 7), dim3(64), 0, stream_, gv, v_, Q);
        MZ_HIP(hipGetLastError());
    }
    int rc = net.forwardAZ(reinterpret_cast<const float*>(v_.feat), static_cast<int>(R), d_policy, d_logit, d_value, true);
    if (rc) { return rc; }
    if (sym_ == 8) { // the averages take the place of the heads' outputs: laid out [Q][A], [Q][A], [Q]
        float *a_policy = avg_.p, *a_logit = avg_.p + size_t(Q) * pv.A, *a_value = avg_.p + 2 * size_t(Q) * pv.A;
        hipLaunchKernelGGL(think_sym_reduce_kernel, dim3(Q), dim3(64), 0, stream_, gv, v_, Q, d_policy, d_logit, d_value, a_policy, a_logit, a_value);
        MZ_HIP(hipGetLastError());
        d_policy = a_policy; d_logit = a_logit; d_value = a_value;
    }
    hipLaunchKernelGGL(think_cand_kernel, dim3(Q), dim3(64), azCandSmemBytes(gv.A), stream_, gv, v_, d_policy, d_logit, d_value, pool.errFlag());
    MZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(think_expand_backup_kernel, dim3(games_), dim3(64), 0, stream_, pv, v_, pool.errFlag());
    MZ_HIP(hipGetLastError());
    MZ_HIP(hipMemcpyAsync(h_status_.p, status_.p, size_t(games_) * 4 * sizeof(int), hipMemcpyDeviceToHost, stream_));
    return MZ_OK;
}

} // namespace mz
