"""The batched think of the reference on top of tests/search_model.py, written from the reference's text: ZeroActor::step (actor/zero_actor.cpp:129-157) makes
actor_mcts_think_batch_size selections under virtual loss, evaluates them in one forward, then expands and backs up the queries in batch order.  The tree of
the search model is extended, not edited: ThinkTree adds the virtual loss of mcts.h:33-47 and the forms of getNormalizedMean / getNormalizedPUCTScore /
calculateInitQValue / selectChildByPUCTScore that see it (mcts.cpp:40-61,181-217).  As in search_model.py every float of the reference is a numpy float32 and
every promotion is spelled out; this file imports neither the oracle nor the product.

The environment handed in is that of search_model.py plus, for a search with random rotations, features(rot) and rotate_action(a, rot) (Env::getFeatures
and Env::getRotateAction, base_env.h:88,99).  The rotation draws (`randInt() % 8`, zero_actor.cpp:56) come from a callable, one call per draw.

READINGS names the wrong readings of the text that tests/test_think_model.py tells from the model by a changed record; a ThinkTree or a step() with one of
them switched on plays that reading instead of the reference."""
import numpy as np

from hand_cases import bias, u_term
import search_model as S

f32 = np.float32
FLT_MAX = S.FLT_MAX

READINGS = ("remove_one",            # removeVirtualLoss(1) instead of the leaf's virtual loss (zero_actor.cpp:154-155)
            "duplicates_are_queries",  # every walk is evaluated, expanded and backed up (:142 ignored)
            "no_draw_for_duplicates",  # the rotation is drawn for queries only (:56 runs before :142)
            "done_after_removal",      # handleSearchDone() once the virtual loss is off (:96 runs inside afterNNEvaluation, before :154)
            "n_without_vl",            # total_simulation = count - 1 (mcts.cpp:185 uses getCountWithVirtualLoss)
            "init_q_skips_count0")     # calculateInitQValue skips count == 0 (mcts.cpp:207 skips count + virtual loss == 0)


class ThinkTree(S.Tree):
    """S.Tree with MCTSNode::virtual_loss_"""

    def __init__(self, cfg, reading=None):
        assert reading is None or reading in READINGS, reading
        self.reading = reading
        super().__init__(cfg)

    def reset(self, root_player):
        super().reset(root_player)
        self.vl = [f32(0)]

    def expand(self, leaf, cands):
        super().expand(leaf, cands)
        self.vl.extend([f32(0)] * len(cands))

    def count_vl(self, i):
        return f32(self.count[i] + self.vl[i])  # getCountWithVirtualLoss (mcts.h:46)

    def normalized_mean(self, i):
        """getNormalizedMean (mcts.cpp:40-53): (value * count - virtual_loss) / (count + virtual_loss)"""
        v = f32(self.reward[i] + f32(f32(self.cfg.actor_mcts_reward_discount) * self.mean[i]))
        assert not self.cfg.actor_mcts_value_rescale, "the batched think of board games does not rescale"
        if self.player[i] == self.cfg.actor_mcts_value_flipping_player:
            v = f32(-v)
        with np.errstate(invalid="ignore"):
            return f32(f32(f32(v * self.count[i]) - self.vl[i]) / self.count_vl(i))

    def puct_score(self, i, total, init_q):
        """getNormalizedPUCTScore (mcts.cpp:55-61): u divides by 1 + count + virtual loss, q is init_q iff count + virtual loss == 0"""
        b = bias(total, self.cfg.actor_mcts_puct_base, self.cfg.actor_mcts_puct_init)
        u = u_term(b, self.policy[i], total, self.count_vl(i))
        q = init_q if self.count_vl(i) == 0 else self.normalized_mean(i)
        return f32(u + q)

    def init_q(self, node):
        """calculateInitQValue (mcts.cpp:200-217), the board-game build"""
        assert not self.cfg.atari_init_q
        sum_of_win, s = f32(0), f32(0)
        for c in self.kids(node):
            if (self.count[c] if self.reading == "init_q_skips_count0" else self.count_vl(c)) == 0:
                continue
            sum_of_win = f32(sum_of_win + self.normalized_mean(c))
            s = f32(s + f32(1))
        return f32(f32(sum_of_win - f32(1)) / f32(s + f32(1)))

    def select_child(self, node):
        """selectChildByPUCTScore (mcts.cpp:181-198): total_simulation = int(count + virtual loss - 1)"""
        total = int(f32((self.count[node] if self.reading == "n_without_vl" else self.count_vl(node)) - f32(1)))
        q0 = self.init_q(node)
        best, best_score, best_policy = None, -FLT_MAX, -FLT_MAX
        for c in self.kids(node):
            s = self.puct_score(c, total, q0)
            if s < best_score or (s == best_score and self.policy[c] <= best_policy):
                continue
            best, best_score, best_policy = c, s, self.policy[c]
        assert best is not None
        return best


class Search:
    """One ZeroActor's search of one position, step by step.  `trace` holds one entry per step: dict(paths, query, rot, left), the walks in order; `decision`
    is what handleSearchDone() saw: dict(selected, action, P, V, resign) or None."""

    def __init__(self, cfg, env, net, B, draw_rotation=None, root_noise=None, reading=None):
        assert B >= 1 and not cfg.actor_use_gumbel
        self.cfg, self.env, self.net, self.B, self.draw, self.noise, self.reading = cfg, env, net, B, draw_rotation, root_noise, reading
        self.t = ThinkTree(cfg, reading)
        self.t.reset(S.next_player(env.turn(), env.num_players()))  # resetSearch (zero_actor.cpp:29-34)
        self.trace, self.decision = [], None
        self.steps = self.walks = self.queries = 0

    def done(self):
        return self.t.num_simulation() == self.cfg.actor_num_simulation + 1  # isSearchDone

    def decide(self):
        """handleSearchDone (zero_actor.cpp:159-192) with actor_select_action_by_count, and what the caller reads next: isResign, the P and V strings"""
        t = self.t
        sel = t.select_by_max_count()
        self.decision = dict(selected=sel, action=t.action[sel], player=t.player[sel], P=t.distribution(), V=t.root_value_string(), resign=t.is_resign(sel))

    def step(self):
        """ZeroActor::step (zero_actor.cpp:129-157), the AlphaZero branch"""
        t, cfg = self.t, self.cfg
        left = cfg.actor_num_simulation + 1 - t.num_simulation()
        bs = min(self.B, left)
        assert bs > 0
        entry = dict(paths=[], query=[], rot=[], left=left)
        for _ in range(bs):
            path = t.select()  # beforeNNEvaluation: selection, then the rotation draw (:53-56)
            query = bool(t.vl[path[-1]] == 0) or self.reading == "duplicates_are_queries"
            rot = 0
            if self.draw is not None and (query or self.reading != "no_draw_for_duplicates"):
                rot = self.draw()
            entry["paths"].append(list(path)); entry["query"].append(query); entry["rot"].append(rot)
            for i in path:
                t.vl[i] = f32(t.vl[i] + f32(1))  # addVirtualLoss (:145)
        for path, query, rot in zip(entry["paths"], entry["query"], entry["rot"]):
            if not query:
                continue
            leaf = path[-1]
            e = self.env.clone()
            for i in path[1:]:
                e.act(t.action[i], t.player[i])
            if not e.terminal():
                p, l, v = self.net.forward(e.features(rot) if self.draw is not None else e.features())
                turn, legal = e.turn(), e.legal()
                at = (lambda a: e.rotate_action(a, rot)) if self.draw is not None else (lambda a: a)
                t.expand(leaf, S._sorted_candidates([(a, turn, f32(p[at(a)]), f32(l[at(a)])) for a in range(len(p)) if legal[a]]))
                t.backup(path, v, e.reward())
            else:
                t.backup(path, e.eval_score(), e.reward())
            if leaf == 0 and self.noise is not None:
                S.add_root_noise(cfg, t, self.noise)
            if self.done() and self.reading != "done_after_removal":
                self.decide()  # (:96) the virtual loss of this path is still on
            v = f32(1) if self.reading == "remove_one" else t.vl[leaf]
            for i in path:
                t.vl[i] = f32(t.vl[i] - v)  # removeVirtualLoss (:154-155)
            if self.done() and self.decision is None:
                self.decide()
        self.trace.append(entry)
        self.steps += 1; self.walks += bs; self.queries += sum(entry["query"])

    def think(self, max_steps=None):
        """ZeroActor::think (zero_actor.cpp:36-49); max_steps: the time limit strikes after that many steps, and handleSearchDone() runs on what is there"""
        while not self.done():
            if max_steps is not None and self.steps >= max_steps:
                break
            self.step()
        if self.decision is None:
            assert all(v == 0 for v in self.t.vl) or self.reading == "remove_one"
            self.decide()
        return self.decision


def play(cfg, env, net, moves, B, draw_rotation=None, first_noise=None, resign_enabled=True, reading=None, max_steps=None, searches=None):
    """S.play with the batched think: the records of the first `moves` moves; `searches`, a list, receives every Search"""
    out = []
    for k in range(moves):
        if env.terminal():
            break
        s = Search(cfg, env, net, B, draw_rotation, first_noise if k == 0 else None, reading)
        d = s.think(max_steps)
        if searches is not None:
            searches.append(s)
        resign = resign_enabled and d["resign"]
        out.append(dict(action=d["action"], P=d["P"], V=d["V"], R=None, resign=resign))
        if resign:
            break
        env.act(d["action"], d["player"])
        out[-1]["R"] = "%g" % float(env.reward())
    return out


def play_pool(cfg, envs, net, moves, B, draw_rotation=None, first_noise=None, resign_enabled=True, searches=None):
    """Several games of one worker on one RNG stream: a cycle is one step of every game whose search is not done, and a step's rotation draws are taken game
    by game, each game's walks in order.  All games search a move side by side; a game that has ended sits out.  -> the records, per game"""
    out = [[] for _ in envs]
    live = list(range(len(envs)))
    for k in range(moves):
        live = [g for g in live if not envs[g].terminal() and not (out[g] and out[g][-1]["resign"])]
        if not live:
            break
        ss = {g: Search(cfg, envs[g], net, B, draw_rotation, first_noise[g] if (k == 0 and first_noise is not None) else None) for g in live}
        while any(not s.done() for s in ss.values()):
            for g in live:
                if not ss[g].done():
                    ss[g].step()
        for g in live:
            d = ss[g].decision
            resign = resign_enabled and d["resign"]
            out[g].append(dict(action=d["action"], P=d["P"], V=d["V"], R=None, resign=resign))
            if not resign:
                envs[g].act(d["action"], d["player"])
                out[g][-1]["R"] = "%g" % float(envs[g].reward())
        if searches is not None:
            searches.append(ss)
    return out
