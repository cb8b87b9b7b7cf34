"""The batched think with mz_think_symmetries=8 on top of tests/think_model.py, which is imported, not edited.  The reference has no such option (a leaf is
evaluated once, under the rotation drawn for its walk, zero_actor.cpp:56), so this file is the definition the product is held to:

for every query of a step, with F_r = Env::getFeatures(r) of the leaf and (p_r, l_r, v_r) the network's policy, logits and value on F_r,
    P[a] = (((((((p_0[fwd_0[a]] + p_1[fwd_1[a]]) + p_2[fwd_2[a]]) + ...) + p_7[fwd_7[a]]) * 0.125,   fwd_r[a] = Env::getRotateAction(a, r)
in float32, one rounding per operation, in the order r = 0, 1, .., 7; the same for the logits L[a] and the value V.  The candidates are then made from P and
L in the board's own frame (rotation 0), V is the leaf's value, and everything else — selection under virtual loss, duplicates, terminal leaves, the backup,
the root noise, the decision — is think_model's.  One rotation is still drawn per walk where actor_use_random_rotation_features asks for one; the drawn
value is not used.

The search is think_model.Search itself, handed an environment and a network that do the averaging between them: SymEnv.features(rot) hands out the leaf's
eight views instead of one array (whatever `rot` was drawn) and SymEnv.rotate_action is the identity, since SymNet.forward answers in the board's frame.
The views come from the rule environments' own rotations: tests/rule_envs.py's models take the rotation in features(), tictactoe_rules.py has none and its
planes go through rotate_point, an environment with features(rot) and rotate_action(a, rot) of its own (test_think_model.RotEnv) is asked itself.

On an empty board the eight views are one, so P[a] and P[a'] of two actions that a symmetry maps onto each other are sums of the same eight numbers in two
orders, and often the same float: candidate lists of more than 16 entries with ties, whose order search_model.ref_sort leaves to libstdc++
(AmbiguousOrder).  std_sort(order_of) puts the real std::sort (tests/csrc/ref_sort.cpp behind a callable: policies -> order) in that place for as long as
the block runs; without it such a position raises as ever.

swap=True is the wrong reading the tests tell from the model: the policy read through the planes' table (inv) instead of fwd.  Like its siblings this file
imports neither the oracle nor the product."""
import contextlib

import numpy as np

import rule_envs
import search_model as S
from nogo_rules import REVERSED, rotate_point

f32 = np.float32
EIGHTH = f32(0.125)


def fwd_table(n, A, r):
    """fwd_r[a] = getRotateAction(a, r): a board point goes through the rotation, every action behind the board (the pass) maps to itself"""
    return np.array([rotate_point(r, a, n) if a < n * n else a for a in range(A)])


def inv_table(n, A, r):
    """the planes' table (plane point p shows board point inv_r[p]) stretched over the actions: what a swapped table would read the policy through"""
    return np.array([rotate_point(REVERSED[r], a, n) if a < n * n else a for a in range(A)])


class Views:
    """what SymEnv.features() hands to SymNet.forward(): the leaf, asked for its planes under each rotation"""

    def __init__(self, env):
        self.env = env


class SymEnv:
    def __init__(self, env, side, swap=False):
        self.env, self.side, self.swap = env, side, swap

    def clone(self): return SymEnv(self.env.clone(), self.side, self.swap)
    def act(self, a, player): return self.env.act(a, player)
    def num_players(self): return self.env.num_players()
    def turn(self): return self.env.turn()
    def legal(self): return self.env.legal()
    def terminal(self): return self.env.terminal()
    def eval_score(self): return self.env.eval_score()
    def reward(self): return self.env.reward()

    def features(self, rot=0): return Views(self)  # (the rotation drawn for the walk is not used)
    def rotate_action(self, a, rot): return a      # (SymNet answers in the board's own frame)

    def view(self, r):
        """Env::getFeatures(r) of the position"""
        e = self.env
        if isinstance(e, rule_envs.RuleEnv):
            if e.game == "tictactoe":  # (tictactoe.cpp:77: plane point p shows board point rotate(p, reversed r))
                src = np.array([rotate_point(REVERSED[r], p, 3) for p in range(9)])
                return np.ascontiguousarray(e.features().reshape(4, 9)[:, src]).reshape(-1)
            assert e.game in ("go", "othello", "gomoku", "nogo"), e.game
            f = e.model.features(r)
            assert f.dtype == np.float32 and f.ndim == 1
            return f
        return e.features(r)

    def table(self, A, r):
        if self.swap:
            return inv_table(self.side, A, r)
        if isinstance(self.env, rule_envs.RuleEnv):
            return fwd_table(self.side, A, r)
        return np.array([self.env.rotate_action(a, r) for a in range(A)])


class SymNet:
    """the network of think_model behind the averaging: forward(views) -> (P, L, V) in the board's frame"""

    def __init__(self, net):
        self.net = net
        self.rows = 0  # network rows computed

    def forward(self, views):
        assert isinstance(views, Views), "the averaging network is handed the views of a SymEnv"
        P = L = V = None
        for r in range(8):
            p, l, v = self.net.forward(views.env.view(r))
            self.rows += 1
            p, l, v = np.asarray(p, f32), np.asarray(l, f32), f32(v)
            at = views.env.table(len(p), r)
            if r == 0:
                P, L, V = p[at], l[at], v
            else:
                P, L, V = P + p[at], L + l[at], f32(V + v)
            assert P.dtype == np.float32 and L.dtype == np.float32
        return P * EIGHTH, L * EIGHTH, f32(V * EIGHTH)


@contextlib.contextmanager
def std_sort(order_of):
    """search_model._sorted_candidates by the real std::sort for the length of the block: order_of(policies as float32) -> the indices in sorted order
    (None: the block runs on ref_sort as it is).  The order of a range without ties is the comparator's either way."""
    if order_of is None:
        yield
        return
    keep = S._sorted_candidates
    S._sorted_candidates = lambda cands: [cands[i] for i in order_of(np.array([c[2] for c in cands], f32))]
    try:
        yield
    finally:
        S._sorted_candidates = keep
