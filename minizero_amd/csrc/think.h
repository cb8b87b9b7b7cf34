// Batched think (actor_mcts_think_batch_size = B > 1 under mz_manual_step): one STEP of a game's search is B selections under virtual loss, one forward over
// the leaves that are queries, then expand + backup per query in batch order (ref actor/zero_actor.cpp:129-157, mcts.h:33-47, mcts.cpp:40-61,181-217).
// A step of every game of a lane is five launches on the lane's stream and one small read-back; no workgroup waits for another.
//   think_select_kernel          one wave per game, its walks one after the other: the order is the semantics
//   think_leaf_kernel<CPL>       one wave per (game, walk): leafBody<CPL> of go_body.h for the queries
//   (Net::forwardAZ over games * B samples)
//   think_cand_kernel            one wave per (game, walk): azCandBody for the queries
//   think_expand_backup_kernel   one wave per game: expandBackupBody per query in batch order, the virtual loss of the query's path removed after each
//   think_reroot_kernel          (mz_think_reuse_tree) one wave per game after a move: the subtree of the move played is compacted to the front of the
//                                game's node range and becomes the tree of the next search (the kept nodes' position slots move down with them); any
//                                other game is left alone or cleared
// mz_think_symmetries=8 puts two more launches around the forward, which then runs over 8 * games * B samples:
//   think_sym_planes_kernel      one wave per (query, r = 1 .. 7): the bit-packed planes of the leaf (written under rotation 0) gathered through
//                                GoDevView::inv[r] into block r of the feature buffer, laid out [8][games][B] — block 0 is the buffer of the key at 1
//   think_sym_reduce_kernel      one wave per query: policy, logit and value of the eight rows read through GoDevView::fwd and summed in f32 in the
//                                order r = 0 .. 7, times 0.125f, into the row the candidate kernel reads (with rotation 0)
// The node records keep their layout: the virtual loss is an array of its own beside them, allocated here.
#pragma once
#include "go_dev.h"
#include "pool.h"

namespace mz {

class Net;
constexpr int kThinkMaxBatch = 64;

struct ThinkView {
    int B, n, tab_n;            // walks per step, actor_num_simulation, entries of the two tables
    float* vl;                  // [games][cap] virtual loss per node (mcts.h:59)
    int *path, *path_action;    // [games][B][max_depth]
    int *path_len, *query, *slot; // [games][B]: length of the walk, 1 = the walk is a query, the position slot of a query's leaf
    const uint8_t* rot;         // [games][B] feature rotation drawn for the walk
    int* status;                // [games][4]: root visits after the step, walks of the step, queries of the step, root child on the last query's path if it completed the search (else -1)
    const float* bias_tab;      // [tab_n] PUCT bias for N = 0 .. n + B (N counts virtual losses: the pool's tables end at n)
    const double* sqrt_tab;     // [tab_n]
    // per (game, walk) outputs of the leaves and candidate lists, laid out as GoDevView / the pool's staging lay them out per game
    uint32_t* feat;
    uint64_t* legal;
    int *leaf_player, *terminal;
    float* eval;
    int *cand_count, *cand_action, *cand_player;
    float *cand_policy, *cand_logit, *value, *reward;
};

// The device half behind an interface: the worker (host code, also built without any device code by the host-only test programs) reaches it through
// createThinkDevice(), which think.hip defines; where that unit is not linked the symbol is null and the worker refuses a batch size above 1.
class ThinkDevice {
public:
    virtual ~ThinkDevice() = default;
    // reuse: mz_think_reuse_tree — the scratch of the re-root (one int per node, a worklist of n + 2 entries per game) is allocated only then
    // symmetries: mz_think_symmetries, 1 or 8 — the feature buffer and the heads' outputs hold eight blocks only with 8
    virtual int init(int device, hipStream_t stream, const Pool& pool, const GoDevView& gv, int B, const mz_search_cfg& cfg, bool reuse, int symmetries = 1) = 0;
    virtual int clearAsync() = 0;                             // a new search: no virtual loss anywhere
    virtual uint8_t* hostRot() = 0;                           // [games][B], uploaded by stepAsync (with eight symmetries the draws are made and not used: every leaf is written under rotation 0)
    // one step of every game: select, leaves, forward, candidates, expand + backup, then the status words on their way to hostStatus()
    virtual int stepAsync(Pool& pool, const GoDevView& gv, Net& net) = 0;
    virtual const int* hostStatus() const = 0;                // valid after the stream has been waited for
    // the re-root: hostReroot() is [games][2] = (action, player) per game — action -2 leaves the game alone (reroot() puts that back everywhere), -1 clears
    // its tree, an action id keeps the subtree of the root's child with it, if that child is expanded, and clears otherwise.  reroot() runs the kernel on
    // the stream and waits; hostRerootStatus() is then [games][2] = (count of the kept root, 0 = cleared; nodes of the game)
    virtual int* hostReroot() = 0;
    virtual int reroot(Pool& pool, const GoDevView& gv) = 0;
    virtual const int* hostRerootStatus() const = 0;
};
ThinkDevice* createThinkDevice() __attribute__((weak));

} // namespace mz
