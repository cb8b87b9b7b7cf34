// Read-out of the visited search tree (Tree::toString's view of it, ref actor/tree.h:79-110): the nodes the reference would print — the root and every node
// with count > 0 (MCTSNode::displayInTreeLog, ref mcts.h:27) — compacted breadth-first into arrays of their own, one wave64 per game (tree_read.hip).
// The output is a queue: entry 0 is the root, `head` walks the entries, the kept children of an entry are appended behind `tail` in child order.  So the children
// of one parent are contiguous and ascending in `ordinal`, and the whole order is a function of the tree alone.
// Capacity: a search of n + 1 simulations visits at most n + 1 nodes besides the root, so n + 2 entries hold every tree a worker can build.
// Nothing here runs while a search kernel of the same pool is in flight: the launch is queued on the pool's stream, behind whatever the last cycle launched.
#pragma once
#include "pool.h"

namespace mz {

constexpr int kTreeInts = 6, kTreeFloats = 7;
// rows of the two per-game blocks
enum { kTrParent = 0, kTrOrdinal, kTrAction, kTrPlayer, kTrNumChildren, kTrDepth };
enum { kTrCount = 0, kTrMean, kTrPolicy, kTrLogit, kTrNoise, kTrValue, kTrReward };

struct TreeReadView {
    int cap;       // entries per game
    int* ints;     // [games][kTreeInts][cap]: parent (entry index, -1 for the root), ordinal (index among the parent's children), action, player, num_children, depth
    float* floats; // [games][kTreeFloats][cap]: count, mean, policy, logit, noise, value, reward — copied, never recomputed
    int* src;      // [games][cap]: where the children of every entry start in the pool (with num_children and depth above: the queue itself)
    int* info;     // [games][4]: entries written (-1: more than cap), num_nodes of the pool, deepest depth, unused
    int* err;      // the pool's error flag: MZ_ERR_CAPACITY where a game has more visited nodes than cap
};

// one game's read-out on the host: ints[row * entries + e], floats[row * entries + e]
struct TreeSnapshot {
    int entries = 0, num_nodes = 0, deepest = 0;
    std::vector<int> ints;
    std::vector<float> floats;
    const int* irow(int r) const { return ints.data() + size_t(r) * entries; }
    const float* frow(int r) const { return floats.data() + size_t(r) * entries; }
};

// The device half behind an interface, as think.h does it: the worker reaches it through createTreeReader(), which tree_read.hip defines; where that unit is
// not linked (the host-only test programs) the symbol is null and the worker refuses the read-out by name.
class TreeReader {
public:
    virtual ~TreeReader() = default;
    virtual int init(int device, hipStream_t stream, const Pool& pool, int entries_per_game) = 0;
    // the read-out of one game (the kernel runs with a mask that names it); waits for the stream
    virtual int read(Pool& pool, int game, TreeSnapshot* out) = 0;
};
TreeReader* createTreeReader() __attribute__((weak));

} // namespace mz
