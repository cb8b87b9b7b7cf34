// Device body of the batched think's selection (think.h): the walks of one step of game `g`, run by ONE wave64 one after the other under virtual loss.
// The formulas are the reference's with the virtual loss in (mcts.cpp:40-61,181-217, mcts.h:46), written as the reference writes them — real IEEE divisions, the
// log() / sqrt() of the PUCT bias from host-built tables indexed by N (which counts virtual losses and so reaches n + B), the init-Q sum an ordered f32 sum over
// the children in storage order, ties by mcts.cpp:191.  No visited-prefix shortcut and no speculation: a child with only virtual loss has a q of its own (-1), so
// the children that need a look are all of them.
#pragma once
#include "pool_body.h"
#include "think.h"

namespace mz {

// q of a child that count + virtual loss != 0 (ref mcts.cpp:40-53 without value rescaling: board games do not rescale)
__device__ __forceinline__ float thinkMean(const PoolView& v, const NodeRec& c, float vl, int cplayer)
{
    float value = c.reward + v.gamma * c.mean;
    value = (cplayer == v.flipping_player) ? -value : value;
    return (value * c.count - vl) / (c.count + vl);
}

__device__ __forceinline__ void thinkWaveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// err: the pool's error flag (a walk deeper than the path arrays or an N past the tables: MZ_ERR_CAPACITY)
__device__ __forceinline__ void thinkSelectBody(const PoolView& v, const ThinkView& t, int g, int lane, int* err)
{
    NodeRec* recs = v.rec + size_t(g) * v.cap;
    float* vls = t.vl + size_t(g) * v.cap;
    const int B = t.B, MD = v.max_depth;
    const int count0 = static_cast<int>(recs[0].count);
    const int left = t.n + 1 - count0;
    const int bs = left < 0 ? 0 : (left < B ? left : B);
    int nq = 0;
    for (int b = 0; b < B; ++b) {
        const size_t q = size_t(g) * B + b;
        if (b >= bs) { // not walked in this step: nothing of an earlier step may look like a query
            if (lane == 0) { t.query[q] = 0; t.path_len[q] = 0; }
            continue;
        }
        thinkWaveSync(); // the virtual loss the walk before this one left behind
        int* path = t.path + q * MD;
        int* pact = t.path_action + q * MD;
        NodeRec cur = loadRec(recs);
        float cur_vl = vls[0];
        int node = 0, depth = 1;
        if (lane == 0) { path[0] = 0; pact[0] = cur.action; vls[0] = cur_vl + 1.0f; } // addVirtualLoss (zero_actor.cpp:145) as the walk passes: every value read below is the one from before this walk
        bool bad = false;
        while (cur.num_children != 0) {
            if (depth >= MD) { bad = true; break; }
            const int nc = cur.num_children, fc = cur.first_child, cplayer = (cur.players >> 8) & 0xFF;
            const int N = static_cast<int>((cur.count + cur_vl) - 1); // total_simulation (mcts.cpp:185)
            if (N < 0 || N >= t.tab_n || fc < 0 || fc + nc > v.cap) { bad = true; break; }
            const float bias = t.bias_tab[N];
            const double sqrtN = t.sqrt_tab[N];
            // ---- init Q (mcts.cpp:200-217): ordered sum over the children with count + virtual loss != 0 ----
            float sum_of_win = 0.0f, sum = 0.0f;
            for (int cb = 0; cb < nc; cb += 64) {
                const int i = cb + lane;
                float qv = 0.0f;
                bool vis = false;
                if (i < nc) {
                    const NodeRec c = loadRec(recs + fc + i);
                    const float cvl = vls[fc + i];
                    vis = (c.count + cvl) != 0.0f;
                    if (vis) { qv = thinkMean(v, c, cvl, cplayer); }
                }
                unsigned long long m = __ballot(vis);
                while (m) { const int j = __builtin_ctzll(m); m &= m - 1; sum_of_win += laneF(qv, j); sum += 1; }
            }
            const float init_q = (sum_of_win - 1) / (sum + 1);
            // ---- PUCT score + arg-max (mcts.cpp:55-61,181-198) ----
            float bs_ = -FLT_MAX, bp = -FLT_MAX;
            int bi = INT_MAX;
            for (int cb = 0; cb < nc; cb += 64) {
                const int i = cb + lane;
                if (i < nc) {
                    const NodeRec c = loadRec(recs + fc + i);
                    const float cvl = vls[fc + i];
                    const float cw = c.count + cvl;
                    const float bpol = bias * c.policy;
                    const float value_u = static_cast<float>((static_cast<double>(bpol) * sqrtN) / static_cast<double>(1 + cw));
                    const float value_q = (cw == 0.0f) ? init_q : thinkMean(v, c, cvl, cplayer);
                    const float score = value_u + value_q;
                    if (better(score, c.policy, i, bs_, bp, bi)) { bs_ = score; bp = c.policy; bi = i; }
                }
            }
            float rs = bs_, rp = bp;
            int ri = bi;
            dppBest<0x111, 0xF>(rs, rp, ri);
            dppBest<0x112, 0xF>(rs, rp, ri);
            dppBest<0x114, 0xF>(rs, rp, ri);
            dppBest<0x118, 0xF>(rs, rp, ri);
            dppBest<0x142, 0xA>(rs, rp, ri);
            dppBest<0x143, 0xC>(rs, rp, ri);
            ri = laneI(ri, 63);
            if (ri < 0 || ri >= nc) { bad = true; break; }
            // the winner's record and virtual loss, read again by every lane at one address: the next level's header
            node = fc + ri;
            cur = loadRec(recs + node);
            cur_vl = vls[node];
            if (lane == 0) { path[depth] = node; pact[depth] = cur.action; vls[node] = cur_vl + 1.0f; }
            ++depth;
        }
        if (bad && lane == 0) { atomicExch(err, MZ_ERR_CAPACITY); }
        // the walk is a query iff its leaf carried no virtual loss before it (zero_actor.cpp:142)
        const bool is_query = !bad && cur_vl == 0.0f;
        if (lane == 0) {
            t.path_len[q] = bad ? 0 : depth;
            t.query[q] = is_query ? 1 : 0;
            t.slot[q] = is_query ? count0 + nq : 0; // a query adds one visit to the root: the slots of a search's queries are 0 .. n, as in lock-step
        }
        nq += is_query ? 1 : 0;
    }
    if (lane == 0) {
        t.status[g * 4 + 1] = bs;
        t.status[g * 4 + 2] = nq;
    }
}

} // namespace mz
