"""What the reference shows of a searched tree, written from its text, over the trees of tests/search_model.py and tests/think_model.py:

render(tree, env_string)   Tree::toString (actor/tree.h:79-110) with the node text of MCTSNode::toString (actor/mcts.cpp:63-75): std::fixed, precision 4
entries(tree)              the breadth-first list of the displayed nodes (MCTSNode::displayInTreeLog, actor/mcts.h:27: count > 0; the root always) that the
                           read-out kernel is specified to produce: entry 0 the root, the kept children of an entry appended in child order
Margins                    records, per search, how close its selections came to going the other way (the selection margin of a row)

This file imports neither the oracle nor the product."""
import math
import re

import numpy as np

import search_model as S
import think_model as TM

INTS = ("parent", "ordinal", "action", "player", "num_children", "depth")
FLOATS = ("count", "mean", "policy", "logit", "noise", "value", "reward")


def _tol():
    """the bound tests/test_gpu_net.py holds the f32 network to the oracle with.  That file has no name for it (and existing test files stay as they are), so
    it is read from the sentence of its docstring that states it"""
    import test_gpu_net
    return float(re.search(r"we assert (\S+) against the oracle", test_gpu_net.__doc__).group(1))


TOL = _tol()


def node_text(t, i, digits=4):
    """MCTSNode::toString (mcts.cpp:63-75)"""
    f = "%." + str(digits) + "f"
    vals = (t.policy[i], t.logit[i], t.noise[i], t.value[i], t.reward[i], t.mean[i], t.count[i])
    return "p = %s, p_logit = %s, p_noise = %s, v = %s, r = %s, mean = %s, count = %s" % tuple(f % float(v) for v in vals)


def node_text_of(tr, e):
    """the same text over entry e of a read-out (a dict of arrays): what the device's strings must hold, '%.4f' of the read-out's own values"""
    return "p = %.4f, p_logit = %.4f, p_noise = %.4f, v = %.4f, r = %.4f, mean = %.4f, count = %.4f" % tuple(
        float(tr[k][e]) for k in ("policy", "logit", "noise", "value", "reward", "mean", "count"))


def player_char(p):
    return {0: "N", 1: "B", 2: "W"}.get(p, "?")  # playerToChar (environment/base/base_env.cpp:5-13)


def render(t, env_string, paren_by="expanded", show_unvisited=False, digits=4):
    """Tree::toString(env_string) (tree.h:79-87) and getTreeInfo_r (:89-110).  The keyword arguments switch on the wrong readings that
    tests/test_tree_model.py tells from the text: parentheses decided by the displayed children instead of the expanded ones (:93-98 counts !isLeaf()),
    children that displayInTreeLog() hides printed (:102), another precision (mcts.cpp:66)"""
    assert env_string and env_string[-1] == ")"

    def shown(c):
        return show_unvisited or t.count[c] > 0

    def info(node):
        if paren_by == "expanded":
            k = sum(1 for c in t.kids(node) if t.nkids[c] != 0)
        else:
            k = sum(1 for c in t.kids(node) if shown(c))
        out = []
        for c in t.kids(node):
            if not shown(c):
                continue
            s = "%s[%d]C[%s]%s" % (player_char(t.player[c]), t.action[c], node_text(t, c, digits), info(c))
            out.append("(" + s + ")" if k > 1 else s)
        return "".join(out)

    return env_string[:-1] + "C[" + node_text(t, 0, digits) + "]" + info(0) + ")"


def entries(t):
    """the read-out as a dict of numpy arrays (the keys of minizero_amd.Worker.tree)"""
    queue, rows = [0], [(-1, 0, 0)]  # (parent entry, ordinal, depth)
    head = 0
    while head < len(queue):
        node = queue[head]
        for i, c in enumerate(t.kids(node)):
            if t.count[c] > 0:
                queue.append(c)
                rows.append((head, i, rows[head][2] + 1))
        head += 1
    out = dict(parent=[r[0] for r in rows], ordinal=[r[1] for r in rows], depth=[r[2] for r in rows], action=[t.action[n] for n in queue],
               player=[t.player[n] for n in queue], num_children=[t.nkids[n] for n in queue])
    out = {k: np.array(v, np.int32) for k, v in out.items()}
    for k in FLOATS:
        out[k] = np.array([getattr(t, k)[n] for n in queue], np.float32)
    return out


class Margins:
    """Around Tree.select_child (and ThinkTree's): while the context is open every selection is recorded.

    score   the smallest gap between the best and the second-best PUCT score over all selections, the unvisited children (count == 0) that carry the same
            virtual loss counted as ONE contender, the best of them.
    Why one: such children share their q (init_q without a virtual loss, -1 with one) and the divisor of u, so their scores differ through the prior alone,
    and the best of them is the one with the highest prior — the first of them in child order, the children being stored sorted by prior.  Which of two such
    siblings is taken is therefore a question of the child order, and the child order is compared exactly (ordinal, action): a difference there fails a test
    instead of hiding in a tolerance.  (With total_simulation == 0 every child is such a child and sqrt(0) makes all scores equal: nothing to record.  On a
    9x9 board the priors of neighbouring children lie 1e-6 apart; no weight seed separates 82 of them by the bound below, and under a virtual loss every
    second walk of a step chooses among them.)
    A row is usable on the GPU if score >= score_bound(cfg): a condition on the inputs, not a tolerance on a result."""

    def __init__(self):
        self.score, self.selections, self.scored = math.inf, 0, 0

    def __enter__(self):
        self._orig = {cls: cls.select_child for cls in (S.Tree, TM.ThinkTree)}
        me = self

        def wrap(orig):
            def select_child(t, node):
                best = orig(t, node)
                n_node = t.count_vl(node) if hasattr(t, "vl") else t.count[node]
                total = int(np.float32(n_node - np.float32(1)))
                kids = list(t.kids(node))
                me.selections += 1
                if len(kids) < 2:
                    return best
                q0 = t.init_q(node)
                best_of = {}  # contender -> its best score: a visited child is its own contender, the unvisited ones are one per virtual loss
                for c in kids:
                    key = ("visited", c) if t.count[c] != 0 else ("unvisited", float(t.vl[c]) if hasattr(t, "vl") else 0.0)
                    best_of[key] = max(best_of.get(key, -math.inf), float(t.puct_score(c, total, q0)))
                s = sorted(best_of.values(), reverse=True)
                if len(s) >= 2:
                    me.score = min(me.score, s[0] - s[1])
                    me.scored += 1
                return best
            return select_child

        for cls, orig in self._orig.items():
            cls.select_child = wrap(orig)
        return self

    def __exit__(self, *exc):
        for cls, orig in self._orig.items():
            cls.select_child = orig
        return False


def score_bound(cfg):
    """A score moves by at most TOL through q and by bias * sqrt(N) * TOL through the prior (bias <= puct_init + 1 for every N a test reaches, N <= n); 16 is
    headroom over the sum of the two, for each of the two scores compared"""
    return 16.0 * (cfg.actor_mcts_puct_init + 1.0) * math.sqrt(cfg.actor_num_simulation) * TOL
