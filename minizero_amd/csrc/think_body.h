// Device body of the batched think's selection (think.h): the walks of one step of game `g`, run by ONE wave64 one after the other under virtual loss.
// The formulas are the reference's with the virtual loss in (mcts.cpp:40-61,181-217, mcts.h:46), written as the reference writes them — real IEEE divisions, the
// log() / sqrt() of the PUCT bias from host-built tables indexed by N (which counts virtual losses and so reaches n + B), the init-Q sum an ordered f32 sum over
// the children in storage order, ties by mcts.cpp:191.  No visited-prefix shortcut and no speculation: a child with only virtual loss has a q of its own (-1), so
// the children that need a look are all of them.
#pragma once
#include "pool_body.h"
#include "think.h"
#include "go_dev.h"

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

// Re-root of game `g` after a move (mz_think_reuse_tree; think.h): ONE wave64.  args[g] = (action, player): action < -1 leaves the game alone, -1 clears
// its tree, any other keeps the subtree of the root's child with that action if that child is expanded, and clears otherwise.  The pool allocates by bump, so
// a parent precedes its block of children and the kept nodes, moved to the front of the game's range in ascending old index, keep their blocks contiguous and
// their child order: a node's new index is <= its old one, and the move needs no second copy of the pool.  Nothing is computed: every value is copied.
//   work    [work_cap] the expanded kept nodes whose blocks are still to be marked (a kept tree of c visits has at most c of them)
//   newidx  [cap] 1 = kept while marking, then the node's new index (-1: dropped)
//   status  [2] the kept root's count (0: cleared), the game's number of nodes
// A visited node also owns a position slot of the device rules (go_dev.h: `hslot`, the slot a leaf's position is built from its parent's; a search hands out
// slots 0 .. n in query order).  The next search hands out slots c .. n for a root kept with c visits, so the kept nodes' slots — at most c: a visit of the
// subtree's root makes at most one node visited — are renumbered 0 .. in ascending old order and their positions moved down the same way (new <= old again;
// the kept root was queried before anything below it, so it gets slot 0, where reset_search's root upload puts the same position).
// Every index read from a record is checked against the game's node count before it is used; a tree that fails a check is cleared and the pool's error flag set.
__device__ __forceinline__ void thinkCopySlot(const GoDevView& gv, size_t src, size_t dst, int lane)
{
    for (int w = lane; w < 2 * gv.W; w += 64) { gv.stones[dst * 2 * gv.W + w] = gv.stones[src * 2 * gv.W + w]; }
    for (int p = lane; p < gv.Ppad; p += 64) { gv.lab[dst * gv.Ppad + p] = gv.lab[src * gv.Ppad + p]; }
    if (lane == 0) {
        gv.hash[dst] = gv.hash[src];
        gv.meta[dst * 2] = gv.meta[src * 2];
        gv.meta[dst * 2 + 1] = gv.meta[src * 2 + 1];
    }
}

__device__ __forceinline__ void thinkRerootBody(const PoolView& v, const GoDevView& gv, float* __restrict__ vl, const int* __restrict__ args, int* newidx_all,
                                                int* work_all, int work_cap, int* __restrict__ status, int g, int lane, int* err)
{
    const int action = __builtin_amdgcn_readfirstlane(args[g * 2]), player = __builtin_amdgcn_readfirstlane(args[g * 2 + 1]);
    if (action < -1) { return; }
    const size_t base = size_t(g) * v.cap;
    NodeRec* recs = v.rec + base;
    float* vls = vl + base;
    int* newidx = newidx_all + base;
    int* work = work_all + size_t(g) * work_cap;
    int N = __builtin_amdgcn_readfirstlane(v.num_nodes[g]);
    N = N < 1 ? 1 : (N > v.cap ? v.cap : N);
    const NodeRec root = loadRec(recs);
    bool bad = false;
    const int S = gv.slots;
    if (S < 1 || S > v.cap) { bad = true; } // (the slot map below lives in newidx)
    // ---- 1. the child with the action: keep or clear ----
    int child = -1;
    NodeRec cr{};
    if (action >= 0 && root.num_children > 0) {
        const int nc = root.num_children, fc = root.first_child;
        if (fc < 1 || fc > N - nc) { bad = true; }
        for (int cb = 0; cb < nc && !bad && child < 0; cb += 64) {
            const int i = cb + lane;
            const unsigned long long m = __ballot(i < nc && recs[fc + (i < nc ? i : 0)].action == action);
            if (m) { child = fc + cb + __builtin_ctzll(m); }
        }
        if (child >= 0) {
            cr = loadRec(recs + child);
            if (cr.num_children > 0 && (cr.first_child <= child || cr.first_child > N - cr.num_children)) { bad = true; }
        }
    }
    bool keep = !bad && child >= 0 && cr.num_children > 0;
    int M = 1;
    if (keep) {
        // ---- 2. mark the subtree: the whole block of every expanded kept node ----
        for (int i = lane; i < N; i += 64) { newidx[i] = 0; }
        thinkWaveSync();
        if (lane == 0) { newidx[child] = 1; work[0] = child; }
        int head = 0, tail = 1;
        while (head < tail && !bad) { // head grows by one per turn, tail <= work_cap
            thinkWaveSync();
            const int e = __builtin_amdgcn_readfirstlane(work[head]);
            ++head;
            const NodeRec er = loadRec(recs + e);
            const int nc = er.num_children, fc = er.first_child;
            if (nc <= 0 || fc <= e || fc > N - nc) { bad = true; break; }
            for (int cb = 0; cb < nc; cb += 64) {
                const int i = cb + lane;
                bool exp = false;
                if (i < nc) {
                    newidx[fc + i] = 1;
                    exp = recs[fc + i].num_children > 0;
                }
                const unsigned long long m = __ballot(exp);
                const int cnt = __popcll(m);
                if (cnt > work_cap - tail) { bad = true; break; }
                const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
                if (exp) { work[tail + rank] = fc + i; }
                tail += cnt;
            }
        }
        keep = !bad;
    }
    if (keep) {
        // ---- 3. pass one: the new index of every kept node, ascending ----
        thinkWaveSync();
        int run = 0;
        for (int cb = 0; cb < N; cb += 64) {
            const int i = cb + lane;
            const bool k = i < N && newidx[i] != 0;
            const unsigned long long m = __ballot(k);
            const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
            if (i < N) { newidx[i] = k ? run + rank : -1; }
            run += __popcll(m);
        }
        M = run;
        thinkWaveSync();
        // ---- 4. pass two: move the records and the cold arrays, first_child remapped.  A chunk's stores land at or below its own indices, never in a later
        // chunk's; inside the chunk every lane has its values in registers before any lane stores ----
        for (int cb = 0; cb < N; cb += 64) {
            const int i = cb + lane;
            const int j = i < N ? newidx[i] : -1;
            NodeRec r{};
            float lg = 0.0f, ns = 0.0f, va = 0.0f;
            int hs = -1;
            if (j >= 0) {
                r = loadRec(recs + i);
                lg = v.logit[base + i]; ns = v.noise[base + i]; va = v.value[base + i]; hs = v.hslot[base + i];
                if (r.num_children > 0 && r.first_child > i && r.first_child < N) { r.first_child = newidx[r.first_child]; } // (its block is kept and lies ahead of it: checked while marking)
            }
            thinkWaveSync();
            if (j >= 0) {
                if (j == 0) { r.action = -1; r.players = (r.players & ~0xFF) | (player & 0xFF); } // what ZeroActor::resetSearch writes (ref zero_actor.cpp:33)
                reinterpret_cast<float4*>(recs + j)[0] = make_float4(r.count, r.mean, r.policy, r.reward);
                reinterpret_cast<int4*>(recs + j)[1] = make_int4(r.first_child, r.num_children, r.action, r.players);
                v.logit[base + j] = lg; v.noise[base + j] = ns; v.value[base + j] = va; v.hslot[base + j] = hs;
            }
            thinkWaveSync();
        }
        // ---- 5. the position slots of the kept nodes: renumbered in ascending old order, the positions moved down (newidx is free again: the slot map) ----
        int* smap = newidx;
        for (int i = lane; i < S; i += 64) { smap[i] = 0; }
        thinkWaveSync();
        for (int i = lane; i < M; i += 64) {
            const int hs = v.hslot[base + i];
            if (hs >= 0 && hs < S) { smap[hs] = 1; }
        }
        thinkWaveSync();
        const size_t sb = size_t(g) * S;
        int used = 0;
        for (int cb = 0; cb < S; cb += 64) {
            const int sl = cb + lane;
            const bool k = sl < S && smap[sl] != 0;
            unsigned long long m = __ballot(k);
            const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
            if (sl < S) { smap[sl] = k ? used + rank : -1; }
            while (m) { // a copy reads a slot above every slot written so far or the one the copy before it read: program order per lane is enough
                const int src = cb + __builtin_ctzll(m);
                m &= m - 1;
                if (used != src) { thinkCopySlot(gv, sb + src, sb + used, lane); }
                ++used;
            }
        }
        thinkWaveSync();
        for (int i = lane; i < M; i += 64) {
            const int hs = v.hslot[base + i];
            if (hs >= 0 && hs < S) { v.hslot[base + i] = smap[hs]; }
        }
        thinkWaveSync();
        if (v.hslot[base] != 0) { bad = true; } // the kept root's position is the root upload's
    } else if (lane == 0) { // reset_kernel's root (pool.hip)
        NodeRec n;
        n.count = 0; n.mean = 0; n.policy = 0; n.reward = 0;
        n.first_child = -1; n.num_children = 0; n.action = -1;
        n.players = player;
        recs[0] = n;
        v.logit[base] = 0; v.noise[base] = 0; v.value[base] = 0; v.hslot[base] = -1;
        v.bound_size[g] = 0;
        v.bound_lo[g] = 0; v.bound_hi[g] = 0;
    }
    for (int i = lane; i < N; i += 64) { vls[i] = 0.0f; } // between two searches no virtual loss is outstanding: cleared, not moved
    if (lane == 0) {
        v.num_nodes[g] = M;
        v.path_len[g] = 0;
        status[g * 2 + 0] = keep ? static_cast<int>(cr.count) : 0;
        status[g * 2 + 1] = M;
        if (bad) { atomicExch(err, MZ_ERR_CAPACITY); }
    }
}

} // namespace mz
