"""Tree reuse between the moves of a game (mz_think_reuse_tree=true) on top of tests/think_model.py, which is imported, not edited.  The reference has no
such option (ZeroActor::resetSearch clears the tree, zero_actor.cpp:29-34), so this file is the definition the product is held to:

act(action, player)   one ply.  If the root has a child with that action and the child is expanded (nkids > 0), the child becomes the root: it keeps count,
                      mean, value, reward, policy, logit, noise, its children and everything below them; its action becomes -1, with the player of the move
                      just played (what ZeroActor::resetSearch writes, zero_actor.cpp:33); every node outside the subtree is gone; no virtual loss is left.
                      In any other case (no tree yet, no such child, the child unexpanded: count 0 or a terminal leaf) the tree is a fresh one.
clear()               mz_worker_reset_game, reset_actors, a weight change, env_set_turn: a fresh tree
reset_search()        a kept tree is searched on: the search is done at count == n + 1 (isSearchDone unchanged), so a root kept with c visits runs
                      n + 1 - c simulations, its first step is an ordinary step of min(B, n + 1 - c) walks, and a rotation is drawn per walk that is made

The subtree is copied by ascending old index: the tree allocates by bump, a parent precedes its block of children, so blocks stay contiguous and the child
order stays.  Capacity: a kept root with c visits has at most c expanded nodes below and including it and the search expands at most n + 1 - c more, so the
tree never holds more than 1 + (n + 1) * A nodes (A: the largest number of children of a node).

READINGS names the wrong readings that tests/test_think_reuse_model.py tells from the model by a changed record, tree field or counter.  Like its siblings
this file imports neither the oracle nor the product."""
import copy

import numpy as np

import search_model as S
import think_model as TM

f32 = np.float32

READINGS = ("n_new_simulations",        # every search runs n + 1 simulations on top of what was kept
            "root_keeps_action",        # the new root keeps the action of the move instead of -1
            "unexpanded_child_kept",    # a child without children (count 0 or a terminal leaf) becomes the root instead of a fresh tree
            "one_ply_only",             # only the first act after a search re-roots: the opponent's act clears
            "vl_survives",              # the virtual loss handleSearchDone() saw on the last query's path is carried into the kept tree
            "draws_for_skipped_walks")  # rotations are drawn as if the search had made all n + 1 walks

FIELDS = ("action", "player", "count", "mean", "policy", "logit", "noise", "value", "reward", "first", "nkids", "hidden", "vl")


def fresh_tree(cfg, root_player):
    t = TM.ThinkTree(cfg)
    t.reset(root_player)
    return t


def subtree(t, child, player, keep_action=False, vl=None):
    """the tree below `child` as a tree of its own, nodes in ascending old index"""
    keep, work = {child}, [child]
    while work:
        node = work.pop()
        for c in t.kids(node):  # the whole block of an expanded node is kept; only the expanded ones have anything below them
            keep.add(c)
            if t.nkids[c] > 0:
                work.append(c)
    order = sorted(keep)
    assert order[0] == child, "a parent precedes its children"
    new = {old: i for i, old in enumerate(order)}
    out = TM.ThinkTree(t.cfg)
    for k in FIELDS:
        src = vl if (k == "vl" and vl is not None) else getattr(t, k)
        setattr(out, k, [src[old] for old in order])
    out.first = [new[t.first[old]] if t.nkids[old] > 0 else 0 for old in order]
    if vl is None:
        out.vl = [f32(0)] * len(order)
    if not keep_action:
        out.action[0] = -1
    out.player[0] = player
    out.bound = {}
    return out


class _Search(TM.Search):
    """think_model.Search over a tree that may already hold visits; it remembers the virtual loss handleSearchDone() saw (for the reading that carries it on)"""

    def __init__(self, cfg, env, net, B, draw, tree):
        super().__init__(cfg, env, net, B, draw)
        if tree is not None:
            self.t = tree
        self.vl_at_decision = None

    def decide(self):
        self.vl_at_decision = list(self.t.vl)
        super().decide()


class ReuseSearch:
    """One game of a worker with mz_think_reuse_tree: `tree` is what the worker holds for the game between the calls (None: no tree yet)."""

    def __init__(self, cfg, env, net, B, draw_rotation=None, reuse=True, reading=None):
        assert reading is None or reading in READINGS, reading
        assert B >= 1 and not cfg.actor_use_gumbel
        self.cfg, self.env, self.net, self.B, self.draw, self.reuse, self.reading = cfg, env, net, B, draw_rotation, reuse, reading
        self.tree, self.is_kept, self.s, self.kept_root = None, False, None, 0
        self.acts_since_search = 0
        self.reroots = self.kept = self.kept_visits = 0  # acts with the option on, those that kept a subtree, the visits of the roots kept
        self.steps = self.walks = self.queries = 0

    # ---- what the caller does between two searches ----
    def _reroot(self, action, player):
        """-> (the tree after the move (action, player), whether it is a kept subtree)"""
        t = self.tree
        fresh = fresh_tree(self.cfg, player)
        if not self.reuse or t is None:
            return fresh, False
        if self.reading == "one_ply_only" and self.acts_since_search > 0:
            return fresh, False
        child = next((c for c in t.kids(0) if t.action[c] == action), None)
        if child is None:
            return fresh, False
        if t.nkids[child] == 0 and self.reading != "unexpanded_child_kept":
            return fresh, False
        vl = self.s.vl_at_decision if (self.reading == "vl_survives" and self.s is not None and self.acts_since_search == 0) else None
        return subtree(t, child, player, keep_action=self.reading == "root_keeps_action", vl=vl), True

    def reroot(self, action, player):
        return self._reroot(action, player)[0]

    def act(self, action, player):
        self.env.act(action, player)
        if self.reuse:
            self.tree, self.is_kept = self._reroot(action, player)
            self.reroots += 1
            if self.is_kept:
                self.kept += 1
                self.kept_visits += int(self.tree.count[0])
        else:
            self.tree, self.is_kept = fresh_tree(self.cfg, player), False
        self.acts_since_search += 1

    def clear(self):
        self.tree, self.is_kept = None, False

    # ---- the search ----
    def reset_search(self):
        cfg = self.cfg
        kept = self.tree if (self.reuse and self.is_kept) else None
        c = int(kept.count[0]) if kept is not None else 0
        self.kept_root = c
        if self.reading == "n_new_simulations" and c > 0:
            cfg = copy.copy(cfg)
            cfg.actor_num_simulation = self.cfg.actor_num_simulation + c
        self.s = _Search(cfg, self.env, self.net, self.B, self.draw, kept)
        self.tree, self.is_kept = self.s.t, False
        self.acts_since_search = 0
        if self.reading == "draws_for_skipped_walks" and self.draw is not None:
            for _ in range(c):
                self.draw()
        return self.s

    def done(self):
        return self.s.done()

    def step(self):
        before = (self.s.steps, self.s.walks, self.s.queries)
        self.s.step()
        self.steps += self.s.steps - before[0]; self.walks += self.s.walks - before[1]; self.queries += self.s.queries - before[2]

    def think(self, max_steps=None):
        """ZeroActor::think: reset the search, step until it is done (or the limit strikes after max_steps steps), decide"""
        self.reset_search()
        while not self.s.done() and (max_steps is None or self.s.steps < max_steps):
            self.step()
        if self.s.decision is None:
            self.s.decide()
        return self.s.decision

    def stats(self):
        return (self.reroots, self.kept, self.kept_visits)


def most_visited_reply(rs):
    """the opponent answers with the most visited child of the root kept after our move (the grandchild of the search is kept); None: no kept tree"""
    t = rs.tree
    if t is None or t.nkids[0] == 0 or all(t.count[c] == 0 for c in t.kids(0)):
        return None
    c = t.select_by_max_count()
    return t.action[c], t.player[c]


def unvisited_reply(rs):
    """the opponent answers with the last child of the kept root that has no visit (the tree is cleared); None: there is none"""
    t = rs.tree
    if t is None or t.nkids[0] == 0:
        return None
    cs = [c for c in t.kids(0) if t.count[c] == 0]
    return (t.action[cs[-1]], t.player[cs[-1]]) if cs else None


def play(cfg, env, net, moves, B, draw_rotation=None, reuse=True, reading=None, opponent=None, max_steps=None, resign_enabled=True, log=None):
    """think_model.play with the tree carried over: the records of the first `moves` searched moves.  opponent(rs) -> (action, player) or None: a reply played
    through act after every searched move, so that every search is the same side's.  `log`, a list, receives per searched move a dict: decision, trees (a
    deep copy of the tree after the search, after our act and after the reply), think (steps, walks, queries so far), reuse (stats so far), root (the
    visits the search started with)"""
    rs = ReuseSearch(cfg, env, net, B, draw_rotation, reuse, reading)
    out = []
    for _ in range(moves):
        if env.terminal():
            break
        d = rs.think(max_steps)
        entry = dict(decision=d, root=rs.kept_root, trees=[copy.deepcopy(rs.tree)], reply=None)
        resign = resign_enabled and d["resign"]
        out.append(dict(action=d["action"], P=d["P"], V=d["V"], R=None, resign=resign))
        if not resign:
            rs.act(d["action"], d["player"])
            out[-1]["R"] = "%g" % float(env.reward())
            entry["trees"].append(copy.deepcopy(rs.tree))
            reply = opponent(rs) if (opponent is not None and not env.terminal()) else None
            if reply is not None:
                rs.act(*reply)
                entry["reply"] = reply
                entry["trees"].append(copy.deepcopy(rs.tree))
        entry["think"], entry["reuse"], entry["nodes"] = (rs.steps, rs.walks, rs.queries), rs.stats(), [len(t.action) for t in entry["trees"]]
        if log is not None:
            log.append(entry)
        if resign:
            break
    return out
