"""Hand-computed search cases: what the formulas of the reference's MCTS give on tiny trees, worked out on paper and spelled here in numpy f32 / f64
operations (ref actor/mcts.cpp:20-28 running mean, :40-53 normalized mean, :55-61 PUCT score, :181-203 the arg-max and its tie rule, :205-217 init-Q in both
builds, :163-179 backup, :219-228 value-bound multiset).  Nothing here calls the oracle or the product to GET an expectation — the same cases are then run
against the oracle's tree (tests/test_oracle_search.py, CPU) and against the HIP node pool (tests/test_gpu_pool.py, GPU)."""
import math

import numpy as np

f32 = np.float32


def bias(N, base=19652.0, init=1.25):
    """float puct_bias = init + log((1 + N + base) / base): the ratio in f32, log in double (mcts.cpp:57)"""
    ratio = f32((f32(1) + f32(N) + f32(base)) / f32(base))
    return f32(f32(init) + math.log(float(ratio)))


def u_term(b, policy, N, count):
    """(puct_bias * policy * sqrt(N)) / (1 + count): float * float, then double sqrt promotes the product, then the division (mcts.cpp:58)"""
    return f32((float(f32(b * f32(policy))) * math.sqrt(float(N))) / float(1 + count))


def add(count, mean, v, w=1.0):
    """count += w; mean += w * (v - mean) / count (mcts.cpp:20-28)"""
    count = f32(count + f32(w))
    mean = f32(mean + f32(f32(f32(w) * f32(f32(v) - mean)) / count))
    return count, mean


def case_tie_rule(tree):
    """equal scores: the child with the higher prior wins; equal priors too: the FIRST one (`policy <= best_policy -> continue`, mcts.cpp:191)"""
    t = tree(dict(actor_num_simulation=8))
    t.reset(2)
    assert t.select() == [0]
    t.expand_backup([3, 4, 5], 1, [0.4, 0.4, 0.2], [0.0, 0.0, -0.7], 0.0)
    assert t.select() == [0, 1]  # N = 0: u = 0, init_q = (0 - 1) / (0 + 1) = -1 for all three


def case_flipping_player(tree):
    """a visited child whose action was played by the flipping player ('W' = 2) counts with its mean negated (mcts.cpp:50)"""
    t = tree(dict(actor_num_simulation=8))
    t.reset(1)                                        # the root's action belongs to player 1: its children are white's moves
    t.select()
    t.expand_backup([0, 1], 2, [0.55, 0.45], [0.0, 0.0], 0.0)
    assert t.select() == [0, 1]
    t.expand_backup([2], 1, [1.0], [0.0], 0.8)       # the visited child: mean 0.8, q = -0.8 for white
    # N = 1.  child 0: u = bias(1) * 0.55 * 1 / 2, q = -0.8.  child 1 unvisited: init_q = (-0.8 - 1) / 2 = -0.9, u = bias(1) * 0.45 / 1
    b = bias(1)
    s0 = f32(u_term(b, 0.55, 1, 1) + f32(-0.8))
    s1 = f32(u_term(b, 0.45, 1, 0) + f32(f32(f32(-0.8) - f32(1)) / f32(2)))
    assert s1 > s0                                    # -0.337... against -0.456...
    assert t.select() == [0, 2]


def case_rescale_discount_atari(tree):
    """value rescaling + discount + rewards + the ATARI init-Q on a four-step search; bounds of the multiset after every backup"""
    t = tree(dict(actor_num_simulation=8, actor_mcts_value_rescale=True, actor_mcts_reward_discount=0.5, atari_init_q=True))
    g = f32(0.5)
    t.reset(1)
    assert t.select() == [0]
    t.expand_backup([7, 8, 9], 1, [0.5, 0.3, 0.2], [0.0, 0.0, 0.0], 0.2, 0.0)
    c0, m0 = add(f32(0), f32(0), 0.2)                 # root: count 1, mean 0.2; multiset {0 + g * 0.2}
    assert t.bound() == (1, f32(g * m0), f32(g * m0))
    assert t.root() == (c0, m0)
    # step 1: N = 0 -> u = 0; ATARI init-Q with no visited child = 1 for every child: tie -> highest prior
    assert t.select() == [0, 1]
    t.expand_backup([1, 2], 1, [0.6, 0.4], [0.0, 0.0], 1.0, 2.0)
    c1, m1 = add(f32(0), f32(0), 1.0)                 # node 1: reward 2, mean 1 -> multiset gains 2 + g * 1 = 2.5
    up = f32(f32(2.0) + f32(g * f32(1.0)))            # value handed to the root: r + g * v = 2.5
    old_root = f32(g * m0)
    c0, m0 = add(c0, m0, up)                          # root: count 2, mean 0.2 + (2.5 - 0.2) / 2 = 1.35
    assert m0 == f32(f32(0.2) + f32(f32(up - f32(0.2)) / f32(2)))
    new_root = f32(g * m0)                            # 0.675 replaces 0.1
    assert old_root != new_root
    assert t.bound() == (2, new_root, f32(2.5))
    assert t.root() == (c0, m0)
    # step 2: N = 1.  child 0 (visited): value 2.5 -> (2.5 - lo) / (hi - lo) = 1 -> 2 * 1 - 1 = 1.  ATARI init-Q = mean of the visited = 1
    b = bias(1)
    s = [f32(u_term(b, 0.5, 1, 1) + f32(1)), f32(u_term(b, 0.3, 1, 0) + f32(1)), f32(u_term(b, 0.2, 1, 0) + f32(1))]
    assert int(np.argmax(s)) == 1                     # 1.3125 | 1.375 | 1.25
    assert t.select() == [0, 2]
    t.expand_backup([4], 1, [1.0], [0.0], -1.0, 0.0)
    up2 = f32(f32(0) + f32(g * f32(-1.0)))            # -0.5 (node 2: reward 0, mean -1 -> multiset gains -0.5)
    old_root = f32(g * m0)
    c0, m0 = add(c0, m0, up2)                         # root: count 3
    assert t.bound() == (3, f32(-0.5), f32(2.5))
    assert t.root() == (c0, m0)
    assert f32(g * m0) not in (f32(-0.5), f32(2.5)) and old_root != f32(g * m0)
    # step 3: N = 2.  child 0: q = 1 (its value is the upper bound); child 1: value -0.5 is the lower bound -> 2 * 0 - 1 = -1; init-Q = (1 - 1) / 2 = 0
    b = bias(2)
    s = [f32(u_term(b, 0.5, 2, 1) + f32(1)), f32(u_term(b, 0.3, 2, 1) + f32(-1)), f32(u_term(b, 0.2, 2, 0) + f32(0))]
    assert int(np.argmax(s)) == 0
    # ... and below node 1 (count 1 -> N = 0): u = 0, nothing visited -> init-Q 1 for both -> the higher prior, node 4
    assert t.select() == [0, 1, 4]


def case_rescale_needs_two_bounds(tree):
    """with fewer than two distinct values in the multiset a visited child's normalized mean is 1 (mcts.cpp:44)"""
    t = tree(dict(actor_num_simulation=8, actor_mcts_value_rescale=True))
    t.reset(1)
    t.select()
    t.expand_backup([0, 1], 1, [0.9, 0.1], [0.0, 0.0], 0.0)
    assert t.bound() == (1, f32(0), f32(0))
    assert t.select() == [0, 1]
    t.expand_backup([5], 1, [1.0], [0.0], 0.0)        # value 0 again: the multiset still holds ONE key (0, counted twice ... the root's old 0 left, its new 0 came)
    assert t.bound()[0] == 1
    # N = 1: child 0 visited, q = 1 (size < 2); child 1: init_q (board build) = (1 - 1) / 2 = 0
    b = bias(1)
    s0 = f32(u_term(b, 0.9, 1, 1) + f32(1))
    s1 = f32(u_term(b, 0.1, 1, 0) + f32(0))
    assert s0 > s1
    assert t.select()[:2] == [0, 1]


# ---- a Gumbel root: five children, actor_gumbel_sample_size = 4, actor_num_simulation = 12 (ref actor/gumbel_zero.cpp:74-137) ----
# Root logits 2, 1.5, 1, 0.5, 0: the candidates are nodes 1..4.  budget0 = max(1, floor(12 / (log2(4) * 4))) = 1, so simulations 1..4 start at nodes 1, 2, 3, 4
# (count ascending, logit descending).  Then every candidate has one visit: next budget = floor(12 / (2 * 4 / 2)) = 3, sample 4 -> 2, scores
# logit + (50 + 1) * q = 2 - 1.02 | 1.5 + 0 | 1 + 1.53 | 0.5 + 0: the candidates become [3, 2], the budget 1 + 3 = 4.  From then on the less visited of the two
# starts, node 2 (the higher logit) at equal counts: 2, 3, 2, 3, 2, 3 reaches 4 visits each after simulation 10; the next budget is floor(12 / (2 * 2 / 2)) = 6
# but a sample of 2 is never halved; simulations 11, 12 start at 2, 3.  At the decision the maximum count is 5: node 2 scores 1.5 + 55 * 0, node 3
# 1 + 55 * (0.03 / 5) = 1.33, so the candidates end as [2, 3] and action 11 is played.
GUMBEL_ROOT = dict(actions=[10, 11, 12, 13, 14], policy=[0.4, 0.25, 0.2, 0.1, 0.05], logit=[2.0, 1.5, 1.0, 0.5, 0.0], value=0.1)
GUMBEL_LEAF_VALUE = {1: -0.02, 2: 0.0, 3: 0.03, 4: 0.0}  # every deeper leaf returns 0
GUMBEL_STARTS = [1, 2, 3, 4, 2, 3, 2, 3, 2, 3, 2, 3]
GUMBEL_HALVINGS = [(4, 2, 4)]                             # (simulations finished, sample size, budget)
GUMBEL_FINAL_CANDIDATES = [2, 3]
# Below a start node the walk is plain PUCT.  Every inner node has two children with priors 0.7 / 0.3 and all their values are 0: at N = 0 the higher prior wins
# the tie; at N >= 1 the visited child has q = -0 or 0 and u = bias * 0.7 * sqrt(N) / (1 + count) (0.4375 | 0.4125 | 0.3789 for N = 1, 2, 3 with count = N),
# the other one init-Q (0 - 1) / 2 and u = bias * 0.3 * sqrt(N) (0.375 | 0.530 | 0.650): -0.125 | 0.030 | 0.150.  The first child always wins, so each visit of a
# candidate goes one node deeper along first children.  Nodes are numbered in order of expansion, two per simulation from node 6 on.
GUMBEL_PATHS = [[0, 1], [0, 2], [0, 3], [0, 4], [0, 2, 8], [0, 3, 10], [0, 2, 8, 14], [0, 3, 10, 16], [0, 2, 8, 14, 18], [0, 3, 10, 16, 20],
                [0, 2, 8, 14, 18, 22], [0, 3, 10, 16, 20, 24]]


def gumbel_script_expand(t, path):
    """the scripted network of the Gumbel case: what the leaf at the end of `path` is expanded with; the children's actions belong to players 1, 2, 1, ... by depth"""
    leaf, player = path[-1], 1 + (len(path) - 1) % 2
    if leaf == 0:
        t.expand_backup(GUMBEL_ROOT["actions"], player, GUMBEL_ROOT["policy"], GUMBEL_ROOT["logit"], GUMBEL_ROOT["value"])
    else:
        t.expand_backup([0, 1], player, [0.7, 0.3], [0.0, 0.0], GUMBEL_LEAF_VALUE.get(leaf, 0.0))


def case_gumbel_start_nodes(tree):
    """the PUCT walks below the start children of the scripted Gumbel root, and the root's running mean over its 13 values"""
    t = tree(dict(actor_num_simulation=12))
    t.reset(2)
    path = t.select()
    assert path == [0]
    gumbel_script_expand(t, path)
    c, m = add(f32(0), f32(0), GUMBEL_ROOT["value"])
    for start, expect in zip(GUMBEL_STARTS, GUMBEL_PATHS):
        path = t.select(start)
        assert path == expect, (start, path, expect)
        gumbel_script_expand(t, path)
        c, m = add(c, m, GUMBEL_LEAF_VALUE.get(path[-1], 0.0))
    assert t.root() == (c, m) and c == 13
    # N = 1 at node 2 before simulation 7, spelled out once: the visited first child against the unvisited second one
    b = bias(1)
    assert f32(u_term(b, 0.7, 1, 1) + f32(-0.0)) > f32(u_term(b, 0.3, 1, 0) + f32(f32(f32(-0.0) - f32(1)) / f32(2)))


# ---- a root for the completed-Q policy (gumbel_zero.cpp:9-58): n = 3, children 7, 3, 5, 1 with logits 1, 0.5, 0, -45 and priors 0.5, 0.25, 0.125, 0.125 ----
# Child 0 is visited twice (values 0.25, then 0.75 one node deeper: mean 0.5), child 1 once (0.25); the root's own value is 0.5 and its mean ends as
# 0.5 -> 0.375 -> 0.5 -> 0.4375.  pi_sum = 0.75, q_sum = 0.5 * 0.5 + 0.25 * 0.25 = 0.3125, n / pi_sum = 4, value of an unvisited child = 1 / 4 * (0.5 + 4 * 0.3125)
# = 0.4375.  Maximum count 2: scores logit + 52 * q = 27 | 13.5 | 22.75 | -22.25, minus the maximum 0 | -13.5 | -4.25 | -49.25: the last is below -38 and dropped.
POLICY_ROOT = dict(actions=[7, 3, 5, 1], policy=[0.5, 0.25, 0.125, 0.125], logit=[1.0, 0.5, 0.0, -45.0], value=0.5)
POLICY_EXPECT = {7: "1", 3: "1.37096e-06", 5: "0.0142642"}  # exp(0), exp(-13.5) = 1.3709590...e-06, exp(-4.25) = 0.0142642339...
POLICY_V = "0.437500"


def build_policy_root(t):
    t.reset(2)
    assert t.select() == [0]
    t.expand_backup(POLICY_ROOT["actions"], 1, POLICY_ROOT["policy"], POLICY_ROOT["logit"], POLICY_ROOT["value"])
    assert t.select(1) == [0, 1]
    t.expand_backup([4], 2, [1.0], [0.0], 0.25)
    assert t.select(1) == [0, 1, 5]
    t.expand_backup([6], 1, [1.0], [0.0], 0.75)
    assert t.select(2) == [0, 2]
    t.expand_backup([4], 2, [1.0], [0.0], 0.25)


def case_policy_root(tree):
    """the tree under the completed-Q policy case: paths from the start children and the root's mean, all exact in binary"""
    t = tree(dict(actor_num_simulation=3))
    build_policy_root(t)
    assert t.root() == (f32(4), f32(0.4375))
    # plain PUCT from the root at N = 3: child 0 (q 0.5, u = bias * 0.5 * sqrt(3) / 3 = 0.361) beats child 1 (q 0.25, u = 0.271) and the unvisited ones
    # (init-Q = (0.75 - 1) / 3 = -0.083, u = 0.271); below it the only children
    assert t.select() == [0, 1, 5, 6]


# ---- max count with a tie, and the resign test (mcts.cpp:84-104): every value is -0.75, children 0 and 1 end with two visits each, child 2 with none ----
# selectChildByMaxCount takes the FIRST of the two; P = "20:2,21:2"; the root's action belongs to white, so its win rate is -(-0.75) and -win rate = -0.75; the
# selected child's is -0.75: both below a threshold of -0.5 (resign), not below the default -0.9.  (-0.75 * 5) / 5 and (-0.75 * 2) / 2 are exact.
RESIGN_ROOT = dict(actions=[20, 21, 22], policy=[0.5, 0.3, 0.2], logit=[0.0, 0.0, 0.0], value=-0.75)
RESIGN_EXPECT = dict(selected=1, P={20: "2", 21: "2"}, V="-0.750000")


def build_resign_root(t):
    t.reset(2)
    t.select()
    t.expand_backup(RESIGN_ROOT["actions"], 1, RESIGN_ROOT["policy"], RESIGN_ROOT["logit"], RESIGN_ROOT["value"])
    for start, expect in ((1, [0, 1]), (2, [0, 2]), (2, [0, 2, 5]), (1, [0, 1, 4])):
        assert t.select(start) == expect
        t.expand_backup([0], 1 + (len(expect) - 1) % 2, [1.0], [0.0], -0.75)


def case_resign_root(tree):
    """the tree under the max-count / resign case"""
    t = tree(dict(actor_num_simulation=4))
    build_resign_root(t)
    assert t.root() == (f32(5), f32(-0.75))


ALL = [case_tie_rule, case_flipping_player, case_rescale_discount_atari, case_rescale_needs_two_bounds, case_gumbel_start_nodes, case_policy_root,
       case_resign_root]


class OracleAdapter:
    def __init__(self, oracle, conf):
        self.conf = ":".join(f"{k}={str(v).lower() if isinstance(v, bool) else v}" for k, v in conf.items())
        self.t = oracle.OracleTree(self.conf, 200)

    def reset(self, root_player): self.t.reset(root_player)
    def select(self, start=-1): return [int(x) for x in self.t.select(start)]
    def expand_backup(self, actions, player, policy, logit, value, reward=0.0): self.t.expand_backup(actions, player, policy, logit, value, reward)

    def bound(self):
        import ctypes as C
        lo, hi = C.c_float(), C.c_float()
        n = self.t.L.mzo_tree_value_bound(self.t.h, C.byref(lo), C.byref(hi))
        return (n, f32(lo.value), f32(hi.value))

    def root(self):
        d = self.t.dump()
        return (f32(d["count"][0]), f32(d["mean"][0]))


class PoolAdapter:
    """one game of the HIP node pool through the C ABI"""
    A = 8

    def __init__(self, mz, conf):
        self.pool = mz.Pool(1, 201, self.A, conf.get("actor_num_simulation", 8), reward_discount=conf.get("actor_mcts_reward_discount", 1.0),
                            value_rescale=conf.get("actor_mcts_value_rescale", False), atari_init_q=conf.get("atari_init_q", False))

    def reset(self, root_player): self.pool.reset_search(np.array([root_player], np.int32))

    def select(self, start=-1):
        pl, paths, _ = self.pool.select(None if start < 0 else np.array([start], np.int32))
        return [int(x) for x in paths[0, :pl[0]]]

    def expand_backup(self, actions, player, policy, logit, value, reward=0.0):
        k = len(actions)
        ca, cp, cl = np.zeros((1, self.A), np.int32), np.zeros((1, self.A), np.float32), np.zeros((1, self.A), np.float32)
        ca[0, :k], cp[0, :k], cl[0, :k] = actions, policy, logit
        self.pool.expand_backup(np.array([k], np.int32), ca, cp, cl, np.array([player], np.int32), np.array([value], np.float32), np.array([reward], np.float32))

    def bound(self):
        rr = self.pool.root_read()
        return (int(rr["bound_size"][0]), f32(rr["bound_lo"][0]), f32(rr["bound_hi"][0]))

    def root(self):
        rr = self.pool.root_read()
        return (f32(rr["root_count"][0]), f32(rr["root_mean"][0]))
