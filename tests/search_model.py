"""A plain, slow model of the reference's search, written from the reference's text: actor/mcts.cpp (tree, PUCT, backup, value bound, max count, resign),
actor/gumbel_zero.cpp (the Gumbel root: sequential halving, the start child of a simulation, the completed-Q policy) and actor/zero_actor.cpp:51-98,159-245
(one simulation around a network call, candidates, Gumbel and Dirichlet noise at the root, the decision), player succession from
environment/base/base_env.cpp:27-42.  Every float of the reference is a numpy float32 here and every promotion to double
is spelled out; nothing is computed with a tolerance.  The environment and the network are handed in; this file imports neither the oracle nor the product.

std::sort: libstdc++ sorts a range of at most 16 elements by insertion, which is stable; a longer range goes through introsort, whose result is defined by
the comparator alone only if no two elements compare equal.  ref_sort gives the stable order and raises AmbiguousOrder for a longer range with a tie."""
import math
from functools import cmp_to_key

import numpy as np

from hand_cases import add, bias, u_term

f32 = np.float32
FLT_MAX = f32(np.finfo(np.float32).max)
BLACK, WHITE = 1, 2


class AmbiguousOrder(Exception):
    """a std::sort of more than 16 elements met two that its comparator calls equal: the reference's order is then libstdc++'s business, not the text's"""


class Cfg:
    """the keys of config/configuration.cpp:13-34,45 the search reads, with their defaults (the noise draws themselves are handed to search())"""

    def __init__(self, **kw):
        self.actor_num_simulation = 50
        self.actor_mcts_puct_base = 19652.0
        self.actor_mcts_puct_init = 1.25
        self.actor_mcts_reward_discount = 1.0
        self.actor_mcts_value_rescale = False
        self.actor_mcts_value_flipping_player = WHITE
        self.actor_use_gumbel = False
        self.actor_gumbel_sample_size = 16
        self.actor_gumbel_sigma_visit_c = 50.0
        self.actor_gumbel_sigma_scale_c = 1.0
        self.actor_use_dirichlet_noise = True  # only search() with a root_noise reads it
        self.actor_dirichlet_noise_epsilon = 0.25
        self.actor_resign_threshold = -0.9
        self.atari_init_q = False  # the reference decides this at compile time (#if ATARI, mcts.cpp:211)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def ref_sort(items, less, what):
    out = sorted(items, key=cmp_to_key(lambda a, b: -1 if less(a, b) else (1 if less(b, a) else 0)))
    if len(out) > 16:
        for a, b in zip(out, out[1:]):
            if not less(a, b):
                raise AmbiguousOrder(what)
    return out


class Tree:
    """MCTS of actor/mcts.cpp over parallel Python lists; node 0 is the root, the children of a node are consecutive"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.reset(WHITE)

    def reset(self, root_player):
        """MCTS::reset (mcts.cpp:77-82) and the root's action of ZeroActor::resetSearch (zero_actor.cpp:33)"""
        self.action, self.player = [-1], [root_player]
        self.count, self.mean = [f32(0)], [f32(0)]
        self.policy, self.logit, self.noise = [f32(0)], [f32(0)], [f32(0)]
        self.value, self.reward = [f32(0)], [f32(0)]
        self.first, self.nkids, self.hidden = [0], [0], [None]
        self.bound = {}

    def kids(self, i):
        return range(self.first[i], self.first[i] + self.nkids[i])

    def num_simulation(self):
        return int(self.count[0])  # mcts.h:100

    def add(self, i, v):
        self.count[i], self.mean[i] = add(self.count[i], self.mean[i], v)  # mcts.cpp:20-28, weight 1

    def _rescale(self, v):
        """mcts.cpp:45-48 / gumbel_zero.cpp:25-28: all float; the fmin / fmax go through double and clamp exactly"""
        lo, hi = f32(min(self.bound)), f32(max(self.bound))
        v = f32(f32(v - lo) / f32(hi - lo))
        return f32(min(1.0, max(-1.0, float(f32(f32(f32(2) * v) - f32(1))))))

    def normalized_mean(self, i):
        """getNormalizedMean (mcts.cpp:40-53) without virtual loss: the last line is (value * count - 0) / count, which is NOT always value"""
        v = f32(self.reward[i] + f32(f32(self.cfg.actor_mcts_reward_discount) * self.mean[i]))
        if self.cfg.actor_mcts_value_rescale:
            if len(self.bound) < 2:
                return f32(1)
            v = self._rescale(v)
        if self.player[i] == self.cfg.actor_mcts_value_flipping_player:
            v = f32(-v)
        with np.errstate(invalid="ignore"):
            return f32(f32(v * self.count[i]) / self.count[i])

    def puct_score(self, i, total, init_q):
        """getNormalizedPUCTScore (mcts.cpp:55-61)"""
        b = bias(total, self.cfg.actor_mcts_puct_base, self.cfg.actor_mcts_puct_init)
        u = u_term(b, self.policy[i], total, self.count[i])
        q = init_q if self.count[i] == 0 else self.normalized_mean(i)
        return f32(u + q)

    def init_q(self, node):
        """calculateInitQValue (mcts.cpp:200-217), both builds"""
        sum_of_win, s = f32(0), f32(0)
        for c in self.kids(node):
            if self.count[c] == 0:
                continue
            sum_of_win = f32(sum_of_win + self.normalized_mean(c))
            s = f32(s + f32(1))
        if self.cfg.atari_init_q:
            return f32(sum_of_win / s) if s > 0 else f32(1)
        return f32(f32(sum_of_win - f32(1)) / f32(s + f32(1)))

    def select_child(self, node):
        """selectChildByPUCTScore (mcts.cpp:181-198): a later child wins only with a higher score, or an equal score and a higher prior"""
        total = int(self.count[node]) - 1
        q0 = self.init_q(node)
        best, best_score, best_policy = None, -FLT_MAX, -FLT_MAX
        for c in self.kids(node):
            s = self.puct_score(c, total, q0)
            if s < best_score or (s == best_score and self.policy[c] <= best_policy):
                continue
            best, best_score, best_policy = c, s, self.policy[c]
        assert best is not None
        return best

    def select_from(self, node):
        """selectFromNode (mcts.cpp:139-149)"""
        path = [node]
        while self.nkids[node] > 0:
            node = self.select_child(node)
            path.append(node)
        return path

    def select(self):
        return self.select_from(0)  # mcts.h:94

    def expand(self, leaf, cands):
        """expand (mcts.cpp:151-164); cands = [(action id, player, policy, logit)] in their final order"""
        assert cands
        self.first[leaf], self.nkids[leaf] = len(self.action), len(cands)
        for a, pl, p, l in cands:
            self.action.append(int(a)); self.player.append(pl)
            self.count.append(f32(0)); self.mean.append(f32(0))
            self.policy.append(f32(p)); self.logit.append(f32(l)); self.noise.append(f32(0))
            self.value.append(f32(0)); self.reward.append(f32(0))
            self.first.append(0); self.nkids.append(0); self.hidden.append(None)

    def _q(self, i):
        return f32(self.reward[i] + f32(f32(self.cfg.actor_mcts_reward_discount) * self.mean[i]))

    def backup(self, path, value, reward=0.0):
        """backup (mcts.cpp:166-179) with updateTreeValueBound (mcts.cpp:219-228)"""
        g = f32(self.cfg.actor_mcts_reward_discount)
        up = f32(value)
        self.value[path[-1]], self.reward[path[-1]] = f32(value), f32(reward)
        for i in reversed(path):
            old = self._q(i)
            self.add(i, up)
            if self.cfg.actor_mcts_value_rescale:
                o, nw = float(old), float(self._q(i))
                if o in self.bound:
                    self.bound[o] -= 1
                    if self.bound[o] == 0:
                        del self.bound[o]
                self.bound[nw] = self.bound.get(nw, 0) + 1
            up = f32(self.reward[i] + f32(g * up))

    # ---- root decisions that draw no random number ----
    def select_by_max_count(self, node=0):
        """selectChildByMaxCount (mcts.cpp:91-104): the first child with the largest count"""
        best, mx = None, f32(0)
        for c in self.kids(node):
            if self.count[c] <= mx:
                continue
            best, mx = c, self.count[c]
        assert best is not None
        return best

    def distribution(self):
        """getSearchDistributionString (mcts.cpp:126-137) as {action id: printed count}"""
        return {self.action[c]: "%g" % float(self.count[c]) for c in self.kids(0) if self.count[c] != 0}

    def root_value_string(self):
        """the V tag: std::to_string(root mean) (zero_actor.h:51)"""
        return "%f" % float(self.mean[0])

    def is_resign(self, selected):
        """MCTS::isResign (mcts.cpp:84-89)"""
        thr = f32(self.cfg.actor_resign_threshold)
        return bool(f32(-self.normalized_mean(0)) < thr and self.normalized_mean(selected) < thr)


class GumbelRoot:
    """GumbelZero (actor/gumbel_zero.cpp); `log` lists every halving as (simulations finished, new sample size, new budget)"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.candidates, self.sample_size, self.budget, self.log = [], 0, 0, []

    def _score(self, t, c, mx):
        """logit + (c_visit + max count) * c_scale * q, float throughout (gumbel_zero.cpp:130,133)"""
        k = f32(f32(f32(self.cfg.actor_gumbel_sigma_visit_c) + mx) * f32(self.cfg.actor_gumbel_sigma_scale_c))
        return f32(t.logit[c] + f32(k * t.normalized_mean(c)))

    @staticmethod
    def _max_child_count(t):
        mx = f32(0)
        for c in t.kids(0):
            mx = max(mx, t.count[c])
        return mx

    def sort_by_score(self, t):
        """sortCandidatesByScore (gumbel_zero.cpp:121-137): the maximum runs over ALL root children; an unvisited candidate scores -FLT_MAX"""
        mx = self._max_child_count(t)
        score = {c: (self._score(t, c, mx) if t.count[c] > 0 else -FLT_MAX) for c in self.candidates}
        self.candidates = ref_sort(self.candidates, lambda a, b: score[a] > score[b], "candidate scores")

    def selection(self, t):
        """selection (gumbel_zero.cpp:74-88)"""
        if t.num_simulation() == 0:
            return t.select()
        self.candidates = ref_sort(self.candidates, lambda a, b: bool(t.count[a] < t.count[b] or (t.count[a] == t.count[b] and t.logit[a] > t.logit[b])),
                                   "candidate (count, logit)")
        return [0] + t.select_from(self.candidates[0])

    def sequential_halving(self, t):
        """sequentialHalving (gumbel_zero.cpp:90-119); log2 and the divisions are double, the budgets int"""
        n, m = self.cfg.actor_num_simulation, self.cfg.actor_gumbel_sample_size
        if t.num_simulation() == 1:
            self.candidates = ref_sort(list(t.kids(0)), lambda a, b: bool(t.logit[a] > t.logit[b]), "root logits")[:m]
            self.sample_size = m
            self.budget = int(max(1.0, math.floor(n / (math.log2(m) * self.sample_size))))
            return
        if any(not (t.count[c] >= self.budget) for c in self.candidates):
            return
        next_budget = int(math.floor(n / (math.log2(m) * self.sample_size / 2)))
        if next_budget > 0 and self.sample_size > 2:
            self.sample_size //= 2
            self.sort_by_score(t)
            self.candidates = self.candidates[:self.sample_size]
            self.budget = int(t.count[self.candidates[0]]) + next_budget
            self.log.append((t.num_simulation() - 1, self.sample_size, self.budget))

    def decide(self, t):
        """decideActionNode with actor_select_action_by_count (gumbel_zero.cpp:60-65)"""
        self.sort_by_score(t)
        return self.candidates[0]

    def policy(self, t):
        """getMCTSPolicy (gumbel_zero.cpp:9-58) as {action id: '%g' of exp}; the unordered_map's iteration order is not modelled"""
        n = self.cfg.actor_num_simulation
        pi_sum, q_sum = f32(0), f32(0)
        for c in t.kids(0):
            if t.count[c] == 0:
                continue
            v = t.normalized_mean(c)
            pi_sum = f32(pi_sum + t.policy[c])
            q_sum = f32(q_sum + f32(t.policy[c] * v))
        value_pi = t.value[0]
        if self.cfg.actor_mcts_value_rescale:
            value_pi = f32(1) if len(t.bound) < 2 else t._rescale(value_pi)
        if t.player[t.first[0]] == self.cfg.actor_mcts_value_flipping_player:
            value_pi = f32(-value_pi)
        # 1.0 / (1 + n) is double; n / pi_sum is int / float = float; the sum is float; double * float is double, stored to float (:32)
        with np.errstate(divide="ignore", invalid="ignore"):
            inner = f32(value_pi + f32(f32(f32(n) / pi_sum) * q_sum))
        non_visited = f32((1.0 / (1 + n)) * float(inner))
        mx = self._max_child_count(t)
        k = f32(f32(f32(self.cfg.actor_gumbel_sigma_visit_c) + mx) * f32(self.cfg.actor_gumbel_sigma_scale_c))
        scores, max_logit = {}, -FLT_MAX
        for c in t.kids(0):
            v = non_visited if t.count[c] == 0 else t.normalized_mean(c)
            s = f32(f32(t.logit[c] - t.noise[c]) + f32(k * v))
            if t.action[c] not in scores:  # unordered_map::insert keeps the first
                scores[t.action[c]] = s
            max_logit = max(max_logit, s)
        out = {}
        for a, s in scores.items():
            x = f32(s - max_logit)
            if x < -38:
                continue
            out[a] = "%g" % math.exp(float(x))  # exp(double), printed by an ostream of precision 6
        return out


def next_player(player, num_player=2):
    """getNextPlayer (environment/base/base_env.cpp:27-36); getPreviousPlayer (:38-42) is the same function for one and two players"""
    assert num_player in (1, 2)
    if num_player == 1:
        return player
    return WHITE if player == BLACK else BLACK


other = next_player  # the two-player case


def add_root_noise(cfg, t, root_noise):
    """addNoiseToNodeChildren (zero_actor.cpp:194-213) with the draws handed in, one per child in child order.  Dirichlet (:197-204): epsilon is a float, so
    1 - epsilon, both products and the sum are float, and the logits stay as they are; Gumbel (:205-211): the noise goes onto the logit"""
    assert len(root_noise) == t.nkids[0]
    if cfg.actor_use_dirichlet_noise:
        eps = f32(cfg.actor_dirichlet_noise_epsilon)
        for c, d in zip(t.kids(0), root_noise):
            t.noise[c] = f32(d)
            t.policy[c] = f32(f32(f32(f32(1) - eps) * t.policy[c]) + f32(eps * f32(d)))
    else:
        for c, g in zip(t.kids(0), root_noise):
            t.noise[c] = f32(g)
            t.logit[c] = f32(t.logit[c] + f32(g))


def _sorted_candidates(cands):
    """the sort both calculate...ActionPolicy functions end with (zero_actor.cpp:225-227, 241-243)"""
    return ref_sort(cands, lambda a, b: bool(a[2] > b[2]), "candidate policies")


def search(cfg, env, net, muzero=False, root_noise=None, halvings=None):
    """One move's search, n + 1 simulations of ZeroActor::beforeNNEvaluation / afterNNEvaluation (zero_actor.cpp:51-98) one at a time, then the decision
    (:159-192).  root_noise: the Dirichlet draws (with cfg.actor_use_dirichlet_noise) or else the Gumbel draws for the root's children in child order (see
    add_root_noise).  The environment says how many players take turns (num_players(), base_env.h:101).  Returns (tree, selected, gumbel root)."""
    players = env.num_players()
    t = Tree(cfg)
    t.reset(next_player(env.turn(), players))  # getPreviousPlayer (zero_actor.cpp:33)
    gz = GumbelRoot(cfg)
    selected = None
    while t.num_simulation() < cfg.actor_num_simulation + 1:
        path = gz.selection(t) if cfg.actor_use_gumbel else t.select()
        leaf = path[-1]
        if not muzero:
            e = env.clone()
            for i in path[1:]:
                e.act(t.action[i], t.player[i])
            if not e.terminal():
                p, l, v = net.forward(e.features())
                turn, legal = e.turn(), e.legal()
                t.expand(leaf, _sorted_candidates([(a, turn, f32(p[a]), f32(l[a])) for a in range(len(p)) if legal[a]]))
                t.backup(path, v, e.reward())
            else:
                t.backup(path, e.eval_score(), e.reward())
        else:
            if t.num_simulation() == 0:
                p, l, v, h = net.initial(env.features())
                r = 0.0
            else:
                p, l, v, r, h = net.recurrent(t.hidden[path[-2]], env.action_features(t.action[leaf], t.player[leaf]))
            turn = next_player(t.player[leaf], players)  # Action::nextPlayer (zero_actor.cpp:235, base_env.h:335, atari.h:40)
            legal = env.legal() if leaf == 0 else None
            t.expand(leaf, _sorted_candidates([(a, turn, f32(p[a]), f32(l[a])) for a in range(len(p)) if legal is None or legal[a]]))
            t.backup(path, v, r)
            t.hidden[leaf] = h
        if leaf == 0 and root_noise is not None:
            add_root_noise(cfg, t, root_noise)
        if t.num_simulation() == cfg.actor_num_simulation + 1:
            selected = gz.decide(t) if cfg.actor_use_gumbel else t.select_by_max_count()
        if cfg.actor_use_gumbel:
            gz.sequential_halving(t)
    if halvings is not None:
        halvings.append(list(gz.log))
    return t, selected, gz


def play(cfg, env, net, moves, muzero=False, first_noise=None, resign_enabled=True):
    """The first `moves` moves of one game from the position `env` holds: per search a dict of the action id, the P tag as a dictionary, the V tag, whether
    the actor resigns instead of playing (actor_group.cpp:116-134 with zero_actor.h:40,50-51) and, for a move that is played, the R tag: the reward the
    environment reports after the move, printed by an ostream of precision 6 (base_actor.cpp:22-28,64 with zero_actor.cpp:122-127).  Ends early at a
    resignation or a terminal position."""
    out = []
    for k in range(moves):
        if env.terminal():
            break
        t, sel, gz = search(cfg, env, net, muzero, first_noise if k == 0 else None)
        resign = resign_enabled and t.is_resign(sel)
        out.append(dict(action=t.action[sel], P=gz.policy(t) if cfg.actor_use_gumbel else t.distribution(), V=t.root_value_string(), R=None, resign=resign))
        if resign:
            break
        env.act(t.action[sel], t.player[sel])
        out[-1]["R"] = "%g" % float(env.reward())
    return out


def halving_schedule(n, m, children=None):
    """(first budget, [(simulations finished, sample size, budget)]) of a Gumbel root whose leaves all return 0: every candidate is then visited in turn"""
    cfg = Cfg(actor_num_simulation=n, actor_gumbel_sample_size=m, actor_use_gumbel=True)
    nc = m + 2 if children is None else children
    t, gz = Tree(cfg), GumbelRoot(cfg)
    t.reset(WHITE)
    first = None
    while t.num_simulation() < n + 1:
        path = gz.selection(t)
        k = nc if path[-1] == 0 else 1
        t.expand(path[-1], [(a, other(t.player[path[-1]]), f32(2.0 ** -(a + 1)), f32(-a)) for a in range(k)])
        t.backup(path, 0.0)
        gz.sequential_halving(t)
        if first is None:
            first = gz.budget
    return first, gz.log
