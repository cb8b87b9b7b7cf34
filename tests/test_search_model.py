"""The search model of tests/search_model.py (a third implementation, written from the reference's text) pinned by paper-and-pencil literals, then compared with
the oracle's search as exact strings: action played, P tag, V tag, resignation, move by move.  The same table of configurations runs against the HIP worker in
tests/test_gpu_search_model.py.  A second table (GAME_CASES, GAME_NOISY) holds the rows of the games no oracle plays — Gomoku, Hex, NoGo, Havannah — and
whole games of Go and Othello, which the model plays over tests/rule_envs.py: tests/test_search_model_games.py pins what they show, tests/test_gpu_search_model_games.py runs them against the HIP
worker.  Nothing here compares with a tolerance."""
import ctypes as C
import re

import numpy as np
import pytest

from atari_synth import AtariSynth
import hand_cases as H
from helpers import sharpen
import rule_envs
import search_model as S
from tictactoe_rules import TicTacToe

f32 = np.float32


# ---------------------------------------------------------------------------------------------
# a. literal expectations that pin the model itself (no oracle is loaded by these)
# ---------------------------------------------------------------------------------------------
class ModelAdapter:
    """the tree of the model behind the interface of hand_cases.ALL"""

    def __init__(self, conf):
        self.t = S.Tree(S.Cfg(**conf))
        self.path = None

    def reset(self, root_player): self.t.reset(root_player)

    def select(self, start=-1):
        self.path = self.t.select() if start < 0 else [0] + self.t.select_from(start)
        return list(self.path)

    def expand_backup(self, actions, player, policy, logit, value, reward=0.0):
        if len(actions):
            self.t.expand(self.path[-1], list(zip(actions, [player] * len(actions), policy, logit)))
        self.t.backup(self.path, value, reward)

    def bound(self):
        return (len(self.t.bound), f32(min(self.t.bound)), f32(max(self.t.bound)))

    def root(self):
        return (self.t.count[0], self.t.mean[0])


@pytest.mark.parametrize("case", H.ALL, ids=lambda c: c.__name__)
def test_model_tree_on_hand_cases(case):
    case(ModelAdapter)


# (n, m) -> (first budget, [(simulations finished, sample size, budget) of every halving]), by hand from gumbel_zero.cpp:99,109-115.
# log2: 16 -> 4, 12 -> 3.58496, 3 -> 1.58496, 5 -> 2.32193, 2 -> 1, 8 -> 3, 18 -> 4.16993, 32 -> 5.
BUDGETS = {
    (50, 16): (1, [(16, 8, 2), (24, 4, 5), (36, 2, 11)]),  # 50/64 -> 1; 50/32 = 1.56; 50/16 = 3.1; 50/8 = 6.25; then 12 each, a sample of 2 stays
    (16, 16): (1, []),                                      # 16/64 -> 1; next = floor(16/32) = 0: never halved
    (50, 12): (1, [(12, 6, 3), (24, 3, 7), (36, 1, 16)]),   # 50/43.02 = 1.16; 50/21.51 = 2.32; 50/10.75 = 4.65; 50/5.377 = 9.3 and 3 / 2 = 1
    (24, 3): (5, [(15, 1, 15)]),                            # 24/4.755 = 5.05; 24/2.377 = 10.09, 3 / 2 = 1
    (16, 5): (1, [(5, 2, 3)]),                              # 16/11.61 = 1.38; 16/5.80 = 2.76; then a sample of 2 stays
    (9, 2): (4, []),                                        # 9/2 = 4.5; the sample never exceeds 2
    (7, 16): (1, []),                                       # n < m: nine candidates are never visited
    (100, 8): (4, [(32, 4, 12), (64, 2, 28)]),              # 100/24 = 4.17; 100/12 = 8.3; 100/6 = 16.7
    (40, 18): (1, [(18, 9, 2), (27, 4, 4), (35, 2, 8)]),    # 40/75.06 -> 1; 40/37.53 = 1.07; 40/18.76 = 2.13 and 9 / 2 = 4; 40/8.34 = 4.8
    (64, 32): (1, []),                                      # 64/160 -> 1; next = floor(64/80) = 0
}


@pytest.mark.parametrize("nm", list(BUDGETS), ids=lambda nm: f"n{nm[0]}_m{nm[1]}")
def test_budget_sequence(nm):
    assert S.halving_schedule(*nm) == BUDGETS[nm]


def _scripted_gumbel():
    cfg = S.Cfg(actor_num_simulation=12, actor_gumbel_sample_size=4, actor_use_gumbel=True)
    a, gz = ModelAdapter(dict(actor_num_simulation=12)), S.GumbelRoot(cfg)
    a.reset(2)
    starts, paths = [], []
    for sim in range(13):
        a.path = gz.selection(a.t)
        if sim:
            starts.append(a.path[1])
            paths.append(list(a.path))
        H.gumbel_script_expand(a, a.path)
        if sim == 12:
            selected = gz.decide(a.t)
        gz.sequential_halving(a.t)
    return a.t, gz, starts, paths, selected


def test_scripted_gumbel_root():
    t, gz, starts, paths, selected = _scripted_gumbel()
    assert starts == H.GUMBEL_STARTS and paths == H.GUMBEL_PATHS
    assert gz.log == H.GUMBEL_HALVINGS
    assert gz.candidates == H.GUMBEL_FINAL_CANDIDATES and selected == 2 and t.action[selected] == 11
    assert [int(t.count[c]) for c in t.kids(0)] == [1, 5, 5, 1, 0]


def test_completed_q_policy():
    a = ModelAdapter(dict(actor_num_simulation=3))
    H.build_policy_root(a)
    gz = S.GumbelRoot(S.Cfg(actor_num_simulation=3, actor_gumbel_sample_size=2, actor_use_gumbel=True))
    assert gz.policy(a.t) == H.POLICY_EXPECT
    assert a.t.root_value_string() == H.POLICY_V
    # Gumbel noise on the logits leaves the policy alone where logit + g - g rounds back: g = 0.5 is exact for every logit of this root
    for c in a.t.kids(0):
        a.t.noise[c], a.t.logit[c] = f32(0.5), f32(a.t.logit[c] + f32(0.5))
    assert gz.policy(a.t) == H.POLICY_EXPECT


def test_max_count_tie_and_resign():
    a = ModelAdapter(dict(actor_num_simulation=4, actor_resign_threshold=-0.5))
    H.build_resign_root(a)
    t = a.t
    assert t.select_by_max_count() == H.RESIGN_EXPECT["selected"]
    assert t.distribution() == H.RESIGN_EXPECT["P"] and t.root_value_string() == H.RESIGN_EXPECT["V"]
    assert t.is_resign(1) is True
    t.cfg.actor_resign_threshold = -0.9
    assert t.is_resign(1) is False
    t.cfg.actor_resign_threshold = -0.75  # strictly below
    assert t.is_resign(1) is False


# ---------------------------------------------------------------------------------------------
# the environment and the network the model is handed: the pinned halves of the oracle, or plain Python
# ---------------------------------------------------------------------------------------------
class OracleEnvAdapter:
    """OracleEnv behind the model's environment interface; a clone replays the moves"""

    def __init__(self, oracle, conf, hist=()):
        self.o, self.conf, self.hist = oracle, conf, []
        self.e = oracle.OracleEnv(conf)
        self.e.reset()
        for a, p in hist:
            self.act(a, p)

    def clone(self): return OracleEnvAdapter(self.o, self.conf, self.hist)

    def act(self, a, player):
        assert self.e.act(a, player), (a, player, self.hist)
        self.hist.append((a, player))

    def num_players(self): return 2
    def turn(self): return self.e.turn()
    def legal(self): return self.e.legal_mask()
    def terminal(self): return self.e.is_terminal()
    def eval_score(self): return f32(self.e.eval_score())
    def reward(self): return f32(self.e.reward())
    def features(self): return self.e.features()

    def action_features(self, a, player):
        buf = np.zeros(4096, np.float32)
        n = self.e.L.mzo_env_action_features(self.e.h, a, player, buf.ctypes.data_as(C.POINTER(C.c_float)))
        return buf[:n].copy()


class NetAdapter:
    def __init__(self, net): self.net = net

    def forward(self, feat):
        p, l, v = self.net.forward_az(feat[None])
        return p[0], l[0], v[0]

    def initial(self, feat):
        p, l, v, h = self.net.initial(feat[None])
        return p[0], l[0], v[0], h[0]

    def recurrent(self, hidden, action):
        p, l, v, r, h = self.net.recurrent(hidden[None], action[None])
        return p[0], l[0], v[0], r[0], h[0]


def test_python_tictactoe_equals_oracle_env(oracle):
    rng = np.random.default_rng(3)
    for _ in range(12):
        mine, theirs = TicTacToe(), OracleEnvAdapter(oracle, "env_game=tictactoe")
        while True:
            assert mine.turn() == theirs.turn() and mine.terminal() == theirs.terminal() and list(theirs.legal()) == mine.legal()
            assert np.array_equal(mine.features(), theirs.features()) and mine.eval_score() == theirs.eval_score() and mine.reward() == theirs.reward()
            if mine.terminal():
                break
            a = int(rng.choice(np.flatnonzero(mine.legal())))
            assert np.array_equal(mine.action_features(a, mine.turn()), theirs.action_features(a, mine.turn()))
            p = mine.turn()
            mine.act(a, p)
            theirs.act(a, p)


def test_python_atari_equals_oracle_env(oracle):
    """the synthetic Atari-shaped game of tests/atari_synth.py against the oracle's: the float arrays bit for bit, at every step of random games to their end"""
    rng = np.random.default_rng(5)
    for length in (1, 3, 11, 30):
        theirs = OracleEnvAdapter(oracle, f"env_game=atari:env_atari_episode_length={length}")
        mine = AtariSynth(theirs.e.seed(), length)
        steps = 0
        while True:
            assert mine.turn() == theirs.turn() == 1 and mine.terminal() == theirs.terminal() and list(theirs.legal()) == mine.legal()
            f, g = mine.features(), theirs.features()
            assert f.dtype == g.dtype == np.float32 and f.shape == g.shape and np.array_equal(f.view(np.uint32), g.view(np.uint32))
            assert mine.eval_score() == theirs.eval_score() and mine.reward() == theirs.reward()
            if mine.terminal():
                break
            a = int(rng.integers(18))
            assert np.array_equal(mine.action_features(a, 1).view(np.uint32), theirs.action_features(a, 1).view(np.uint32))
            mine.act(a, 1)
            theirs.act(a, 1)
            steps += 1
        assert steps == length
    # a seed with the sign bit set hashes as its 32-bit pattern; a reward of 1 is in reach of a short game (5 % a step)
    e = AtariSynth(-5, 200)
    for _ in range(200):
        e.act(0)
    assert AtariSynth(-5, 1).useed == 2 ** 32 - 5 and 1 <= float(e.eval_score()) <= 30


# ---------------------------------------------------------------------------------------------
# the table of configurations (shared with tests/test_gpu_search_model.py)
# ---------------------------------------------------------------------------------------------
QUIET = (":actor_use_dirichlet_noise=false:actor_use_random_rotation_features=false:actor_select_action_by_count=true:actor_select_action_by_softmax_count=false"
         ":zero_disable_resign_ratio=0:zero_num_threads=1:program_seed=7:nn_file_name=m.pt")
GO8 = ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero")
GO8_MZ = GO8[:12] + ("muzero",)
GO128 = ("go_9x9", 18, 9, 9, 128, 9, 9, 1, 1, 82, 16, 1, "alphazero")
OTH8 = ("othello_8x8", 4, 8, 8, 8, 8, 8, 1, 1, 65, 16, 1, "alphazero")
TTT16 = ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 1, 9, 16, 1, "alphazero")
ATARI32 = ("atari_ms_pacman", 32, 96, 96, 32, 6, 6, 18, 1, 18, 32, 601, "muzero_atari")
ATARI_C5 = ("atari_ms_pacman", 32, 96, 96, 64, 6, 6, 18, 6, 18, 256, 601, "muzero_atari")  # the network of the benchmark's Atari-shaped configuration


def full_conf(conf, games=None):
    """The string all three sides are configured with: QUIET first, so that a case's own keys (the Dirichlet noise of a noisy case) replace it"""
    return QUIET[1:] + ":" + conf + ("" if games is None else f":zero_num_parallel_games={games}")


def _gumbel(n, m, noise=False):
    return f":actor_num_simulation={n}:actor_use_gumbel=true:actor_gumbel_sample_size={m}:actor_use_gumbel_noise={'true' if noise else 'false'}"


def _atari(moves, rescale=True, discount=0.997):
    """The Atari-shaped search: one player, value rescaling over the value-bound multiset, a reward discount, the init-Q of the reference's ATARI build.  Every
    game ends after `moves` moves, so its line carries SD, the moves and the end; the threshold keeps resignation out of it"""
    return (f"env_game=atari:nn_type_name=muzero:env_atari_episode_length={moves}:zero_actor_intermediate_sequence_length=0:actor_resign_threshold=-2"
            f":actor_mcts_value_rescale={'true' if rescale else 'false'}:actor_mcts_reward_discount={discount}:atari_init_q=true")


DIRICHLET = ":actor_use_dirichlet_noise=true:actor_dirichlet_noise_alpha=0.03:actor_dirichlet_noise_epsilon=0.25"

# name -> (configuration, network, weight seeds, moves, games, gain on the value head's last layer or None).  The weight seeds are those for which the model raises no AmbiguousOrder (chosen on the CPU with
# the model alone; a seed that raised it would fail its case in test_model_equals_oracle).
CASES = {}
for _n, _m in ((50, 16), (16, 16), (50, 12), (40, 18)):
    CASES[f"go_gumbel_n{_n}_m{_m}"] = ("env_game=go:env_board_size=9" + _gumbel(_n, _m), GO8, (2, 3), 3, 4, None)
# the value head times 32: black's first root is worth 0.64 (seed 1) or 0.69 (seed 4) and black plays, then white resigns; with seed 2 black resigns at once
CASES["go_puct_n24_resign"] = ("env_game=go:env_board_size=9:actor_num_simulation=24:actor_resign_threshold=0.5", GO8, (1, 2, 4), 3, 4, 32)
CASES["go_puct_n24"] = ("env_game=go:env_board_size=9:actor_num_simulation=24", GO8, (2, 3), 3, 4, None)
for _n, _m in ((16, 16), (50, 16), (24, 3)):
    CASES[f"othello_gumbel_n{_n}_m{_m}"] = ("env_game=othello:env_board_size=8" + _gumbel(_n, _m), OTH8, (1, 2), 5, 4, None)
for _m in (4, 5, 2):
    CASES[f"ttt_gumbel_n16_m{_m}"] = ("env_game=tictactoe" + _gumbel(16, _m), TTT16, (1, 2, 3), 6, 4, None)
CASES["ttt_puct_n16"] = ("env_game=tictactoe:actor_num_simulation=16", TTT16, (1, 2, 3), 6, 4, None)
for _n, _m in ((16, 16), (50, 16), (33, 6), (12, 8)):
    CASES[f"go_mz_gumbel_n{_n}_m{_m}"] = ("env_game=go:env_board_size=9:nn_type_name=muzero" + _gumbel(_n, _m), GO8_MZ, (2, 3), 3, 4, None)
CASES["go128_gumbel_n50_m16"] = ("env_game=go:env_board_size=9" + _gumbel(50, 16), GO128, (1,), 3, 4, None)
# MuZero with PUCT: the hidden-state slab, children that are never masked below the root, the reward in the backup.  Weight seed 4 raises AmbiguousOrder at n = 24.
CASES["go_mz_puct_n24"] = ("env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=24", GO8_MZ, (2,), 3, 4, None)
CASES["go_mz_puct_n50"] = ("env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=50", GO8_MZ, (3,), 2, 4, None)
# The Atari-shaped rows.  Each game draws its own seed (its SD tag) and is compared with the model's game of that seed.  (16, 4): the small row the GPU file
# runs on every execution mode; (16, 16): never halved; (7, 16): n < m; (50, 12): m no power of two; (40, 18): every root child sampled, sorts beyond 16.
ATARI_MOVES, ATARI_GAMES = 3, 3
for _n, _m in ((16, 4), (16, 16), (7, 16), (50, 12), (40, 18)):
    CASES[f"atari_gumbel_n{_n}_m{_m}"] = (_atari(ATARI_MOVES) + _gumbel(_n, _m), ATARI32, (1, 2) if (_n, _m) == (16, 4) else (2,), ATARI_MOVES, ATARI_GAMES, None)
CASES["atari_c5_gumbel_n16_m4"] = (_atari(ATARI_MOVES) + _gumbel(16, 4), ATARI_C5, (1,), ATARI_MOVES, ATARI_GAMES, None)
for _n in (12, 24):
    CASES[f"atari_puct_n{_n}"] = (_atari(ATARI_MOVES) + f":actor_num_simulation={_n}", ATARI32, (1,), ATARI_MOVES, ATARI_GAMES, None)
# rescale on and off at discount 1.0: the value-bound multiset is all that differs between these two; the first differs from atari_gumbel_n16_m4 in the discount
CASES["atari_gumbel_n16_m4_undiscounted"] = (_atari(ATARI_MOVES, True, 1.0) + _gumbel(16, 4), ATARI32, (1,), ATARI_MOVES, ATARI_GAMES, None)
CASES["atari_gumbel_n16_m4_plain"] = (_atari(ATARI_MOVES, False, 1.0) + _gumbel(16, 4), ATARI32, (1,), ATARI_MOVES, ATARI_GAMES, None)

# the noisy first move: (configuration, network, weight seed, kind of noise at the root)
NOISY = {
    "ttt": ("env_game=tictactoe" + _gumbel(16, 4, True), TTT16, 1, "gumbel"),
    "othello": ("env_game=othello:env_board_size=8" + _gumbel(16, 16, True), OTH8, 1, "gumbel"),
    "go": ("env_game=go:env_board_size=9" + _gumbel(50, 16, True), GO8, 1, "gumbel"),
    "atari": (_atari(1) + _gumbel(16, 4, True), ATARI32, 1, "gumbel"),
    "go_dirichlet": ("env_game=go:env_board_size=9:actor_num_simulation=24" + DIRICHLET, GO8, 2, "dirichlet"),
    "go_mz_dirichlet": ("env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=24" + DIRICHLET, GO8_MZ, 2, "dirichlet"),
    "othello_dirichlet": ("env_game=othello:env_board_size=8:actor_num_simulation=24" + DIRICHLET, OTH8, 1, "dirichlet"),
    "atari_dirichlet": (_atari(1) + ":actor_num_simulation=24" + DIRICHLET, ATARI32, 1, "dirichlet"),
}
NOISY_GAMES = 8

# ---------------------------------------------------------------------------------------------
# Gomoku, Hex, NoGo and Havannah: no oracle plays these games, so their rows are the model's alone — over tests/rule_envs.py — and run against the HIP
# worker in tests/test_gpu_search_model_games.py.  Rows of the form of CASES, in a table of their own: test_model_equals_oracle keeps the rows it has.
# ---------------------------------------------------------------------------------------------
def _net(name, planes, side, actions):
    """1 block x 32 channels, 16 value-hidden channels: the width the simulation-kernel instances of these boards are built for"""
    return (name, planes, side, side, 32, side, side, 1, 1, actions, 16, 1, "alphazero")


def _hex(n, swap=True): return f"env_game=hex:env_board_size={n}" + ("" if swap else ":env_hex_use_swap_rule=false"), _net(f"hex_{n}x{n}", 4, n, n * n)
def _nogo(n): return f"env_game=nogo:env_board_size={n}", _net(f"nogo_{n}x{n}", 18, n, n * n + 1)
def _hav(N): return f"env_game=havannah:env_board_size={N}", _net(f"havannah{N}x{N}", 20, 2 * N - 1, (2 * N - 1) ** 2)


def _gomoku(n, rule="standard", five=True):
    conf = f"env_game=gomoku:env_board_size={n}" + ("" if rule == "standard" else f":env_gomoku_rule={rule}") + ("" if five else ":env_gomoku_exactly_five_stones=false")
    return conf, _net(f"gomoku_{'oo_' if rule == 'outer_open' else ''}{n}x{n}", 4, n, n * n)


def _go(n, komi=0.5, rule="positional", net=None):
    conf = f"env_game=go:env_board_size={n}:env_go_komi={komi}" + ("" if rule == "positional" else f":env_go_ko_rule={rule}")
    return conf, net or _net(f"go_{n}x{n}", 18, n, n * n + 1)


def _othello(n, net=None): return f"env_game=othello:env_board_size={n}", net or _net(f"othello_{n}x{n}", 4, n, n * n + 1)


# the boards with a simulation-kernel instance (32 channels; Go 9x9 and Othello 8x8 also on the 8-channel networks GO8 and OTH8): every other board of these
# games plays lock-step on the default plan
SIM_BOARDS = {("hex", 11), ("gomoku", 15), ("nogo", 9), ("havannah", 8), ("havannah", 4), ("go", 7), ("go", 9), ("othello", 8)}


def has_sim_instance(conf):
    game, n, _ = rule_envs.parse(full_conf(conf))
    return (game, n) in SIM_BOARDS


# the weight seeds of the Go and Othello rows (PUCT, Gumbel), chosen like the others
# (seed 1 raises AmbiguousOrder on Go 9x9 under Gumbel with either network, seed 3 with GO8; go9 PUCT seed 1 and go7 PUCT seed 3 end after 3 and 4 moves)
GO4_SEEDS, GO5_SEEDS, GO7_SEEDS, GO9_SEEDS, GO9C8_SEEDS = ((3, 4), (1, 2)), ((1, 4), (1,)), ((1,), (1,)), ((2,), (2,)), ((1, 2), (2,))
GO5_POS_SEEDS = ((11,), (1,))  # (PUCT seed 11: the row on which the two ko rules give different games)
OTH8_SEEDS, OTH4_SEEDS, OTH6_SEEDS, GO4_N50_SEEDS, OTH4_N50_SEEDS = ((1, 2), (3,)), ((1, 4), (1,)), ((3,), (1,)), (3,), (1,)
PUCT16, GUMBEL16, GUMBEL50, PUCT50 = ":actor_num_simulation=16", _gumbel(16, 16), _gumbel(50, 16), ":actor_num_simulation=50"
NO_RESIGN = ":actor_resign_threshold=-2"
WHOLE = 400  # more moves than any of these boards has cells: a whole-game row ends where the game does

# name -> (configuration, network, weight seeds, moves, games, gain on the value head).  The weight seeds are chosen on the CPU with the model alone: none
# raises AmbiguousOrder (seed 1 does on Hex 11x11 under PUCT, on Gomoku 15x15 and on Havannah 8 under Gumbel), and together they show what
# test_game_rows_show_what_they_are_for asks for.
GAME_CASES = {}
# a. the first three moves on every simulation-kernel instance.  Seeds with the swap taken: hex11 PUCT 2 and 3 (the same action three times: Black's
# stone, White's swap, Black on the cell the swap left empty), hex11 Gumbel 5, hav8 PUCT 3, hav8 Gumbel 4, hav4 1; declined: the others.
for _b, (_c, _d), _seeds in (("hex11", _hex(11), ((2, 3), (2, 5), (2,))), ("gomoku15", _gomoku(15), ((2,), (2,), (2,))), ("gomoku15oo", _gomoku(15, "outer_open"), ((2,), (3,), None)),
                             ("nogo9", _nogo(9), ((1,), (2,), (2,))), ("hav8", _hav(8), ((2, 3), (2, 4), (3,))), ("hav4", _hav(4), ((1, 2), (1, 2), None))):
    for _s, _search, _sd in zip(("puct_n16", "gumbel_n16", "gumbel_n50"), (PUCT16, GUMBEL16, GUMBEL50), _seeds):
        if _sd:
            GAME_CASES[f"{_b}_{_s}"] = (_c + _search, _d, _sd, 3, 4, None)
# b. whole games through the simulation kernel, c. whole games on boards without an instance (lock-step), both without resignation
for _b, (_c, _d), _seeds in (("hav4", _hav(4), ((2, 3), (2, 6))), ("nogo9", _nogo(9), ((2, 3), (2,))), ("hex11", _hex(11), ((2,), (2,))), ("gomoku15", _gomoku(15), ((2,), (2,))),
                             ("hav8", _hav(8), ((9,), (8,))),  # (the model alone finishes these in 8 s and 2 s; seed 2 raises AmbiguousOrder on this board)
                             ("hex4", _hex(4), ((1,), (1,))), ("hex4_noswap", _hex(4, False), ((2,), (1,))), ("hex5", _hex(5), ((4,), (2,))), ("hex5_noswap", _hex(5, False), ((1,), (4,))),
                             ("nogo4", _nogo(4), ((4,), (2,))), ("gomoku5", _gomoku(5), ((1,), (1,))), ("gomoku6", _gomoku(6), ((1, 3), (2,))),
                             ("gomoku6_freestyle", _gomoku(6, five=False), ((1,), (1,)))):
    for _s, _search, _sd in zip(("puct", "gumbel"), (PUCT16, GUMBEL16), _seeds):
        GAME_CASES[f"{_b}_game_{_s}"] = (_c + _search + NO_RESIGN, _d, _sd, WHOLE, 2, None)
# d. the default resign threshold (-0.9) with the value head times 32: with seed 3 Black plays one move and White resigns, with seed 2 Black resigns at once
GAME_CASES["hex11_puct_n16_resign"] = (_hex(11)[0] + PUCT16, _hex(11)[1], (2, 3), 3, 4, 32)
# f. Go and Othello, whole games in the environment of the rules models (tests/go_rules.py, tests/othello_rules.py; tests/test_go_model.py and
# tests/test_othello_model.py hold the host engine and the oracle to them): captures, superko refusals along the tree path, two-pass leaves, leaves past
# the move cap, Tromp-Taylor results with a komi at which both colours win; forced passes and the end of the game in Othello.  go4, go5: lock-step;
# go7, go9: sim_kernel_wide<7,7,32,32,1> and <9,9,32,32,2>; go9c8: sim_kernel<9,9,20,8,2>; oth8: sim_kernel<8,8,4,8,kRulesOthello>; oth4, oth6: lock-step
GO_OTHELLO_ROWS = (("go4", _go(4, 1.0), GO4_SEEDS), ("go5", _go(5), GO5_POS_SEEDS), ("go5_sit", _go(5, 0.5, "situational"), GO5_SEEDS), ("go7", _go(7), GO7_SEEDS), ("go9", _go(9), GO9_SEEDS),
                   ("go9c8", _go(9, net=GO8), GO9C8_SEEDS), ("oth8", _othello(8, OTH8), OTH8_SEEDS), ("oth4", _othello(4), OTH4_SEEDS), ("oth6", _othello(6), OTH6_SEEDS))
for _b, (_c, _d), _seeds in GO_OTHELLO_ROWS:
    for _s, _search, _sd in zip(("puct", "gumbel"), (PUCT16, GUMBEL16), _seeds):
        GAME_CASES[f"{_b}_game_{_s}"] = (_c + _search + NO_RESIGN, _d, _sd, WHOLE, 2, None)
# 50 simulations on the smallest boards: trees deep enough for two-pass leaves
GAME_CASES["go4_game_puct_n50"] = (_go(4, 1.0)[0] + PUCT50 + NO_RESIGN, _go(4)[1], GO4_N50_SEEDS, WHOLE, 2, None)
GAME_CASES["oth4_game_puct_n50"] = (_othello(4)[0] + PUCT50 + NO_RESIGN, _othello(4)[1], OTH4_N50_SEEDS, WHOLE, 2, None)
GO_ROWS = [n for n in GAME_CASES if re.match(r"go\d", n)]
OTHELLO_ROWS = [n for n in GAME_CASES if n.startswith("oth")]
WHOLE_GAMES = [name for name, c in GAME_CASES.items() if c[3] == WHOLE]
# whole-game rows whose model takes more than about ten seconds on the CPU (DESIGN.md lists the seconds of every row)
SLOW_GAMES = ("gomoku15_game_puct",)
ALL_GAME_CASES = [pytest.param(name, s, marks=[pytest.mark.slow] if name in SLOW_GAMES else []) for name, c in GAME_CASES.items() for s in c[2]]


# e. the noisy first move, rows of the form of NOISY.  Havannah 8: the root has 169 children, not 225, and the Dirichlet draws are one per legal child in child
# order (noisy_model counts the legal actions of the root)
GAME_NOISY = {
    "hex11": (_hex(11)[0] + _gumbel(16, 16, True), _hex(11)[1], 2, "gumbel"),
    "hav8_dirichlet": (_hav(8)[0] + ":actor_num_simulation=24" + DIRICHLET, _hav(8)[1], 2, "dirichlet"),
}


def row(name):
    return CASES[name] if name in CASES else GAME_CASES[name]


def noisy_row(name):
    return NOISY[name] if name in NOISY else GAME_NOISY[name]


MOVE = re.compile(r";([BW])\[(\d+)\]P\[([^\]]*)\]V\[([^\]]*)\]R\[([^\]]*)\]")
SEED = re.compile(r"SD\[(-?\d+)\]")


def model_cfg(conf):
    """(the model's Cfg, MuZero?, all keys) of a case's configuration string: every key of Cfg is read from full_conf(conf), so the string alone defines the case"""
    kv = dict(x.split("=", 1) for x in full_conf(conf).split(":") if x)
    kw = {}
    for key, default in vars(S.Cfg()).items():
        if key not in kv:
            continue
        if key == "actor_mcts_value_flipping_player":
            kw[key] = {"B": S.BLACK, "W": S.WHITE}[kv[key]]
        elif isinstance(default, bool):
            assert kv[key] in ("true", "false"), (key, kv[key])
            kw[key] = kv[key] == "true"
        else:
            kw[key] = type(default)(kv[key])
    return S.Cfg(**kw), kv.get("nn_type_name") == "muzero", kv


def case_weights(oracle, desc_args, wseed, vgain=None):
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    w = oracle.gen_weights(od, wseed)
    return w if vgain is None else sharpen(od, w, 1, vgain)


def is_atari(conf):
    return model_cfg(conf)[2]["env_game"] == "atari"


ORACLE_PLAYS = ("go", "othello", "tictactoe")


def make_env(oracle, conf, env_seed=None, rules=False):
    """the environment the model plays in; an Atari-shaped game is that of `env_seed`, the SD tag of the record it is compared with.  rules: the rules model
    of tests/rule_envs.py also for the games the oracle plays (the rows of GAME_CASES; test_first_move_rows_on_the_rules_models)"""
    kv = model_cfg(conf)[2]
    if kv["env_game"] == "tictactoe" and not rules:
        return TicTacToe()
    if kv["env_game"] == "atari":
        assert env_seed is not None, "an Atari-shaped game is defined by its seed"
        return AtariSynth(env_seed, int(kv["env_atari_episode_length"]))
    if rules or kv["env_game"] not in ORACLE_PLAYS:
        return rule_envs.RuleEnv(full_conf(conf))  # no oracle for these games: the rules models of tests/, configured by the worker's own string
    return OracleEnvAdapter(oracle, ":".join(f"{k}={kv[k]}" for k in ("env_game", "env_board_size") if k in kv))


def parse_record(record, moves):
    """[(action id, P dictionary, V string, R string)] of the first `moves` moves of a record"""
    out = []
    for _, a, p, v, r in MOVE.findall(record)[:moves]:
        out.append((int(a), {int(x.split(":")[0]): x.split(":")[1] for x in p.split(",")} if p else {}, v, r))
    return out


def expected_from_model(oracle, conf, desc_args, wseed, moves, first_noise=None, weights=None, halvings=None, env_seed=None, trace=None, env=None):
    """what the model plays: ([(action, P, V, R)] of the moves played, resigned at the next search?, finished (terminal or resigned) within `moves`);
    `trace`, a dictionary, receives the environment as the game left it; `env` replaces the environment of the configuration"""
    cfg, muzero, _ = model_cfg(conf)
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    w = oracle.gen_weights(od, wseed) if weights is None else weights
    env = make_env(oracle, conf, env_seed) if env is None else env
    got = S.play(cfg, env, NetAdapter(oracle.OracleNet(od, w)), moves, muzero, first_noise)
    if trace is not None:
        trace["env"] = env
    resigned = bool(got) and got[-1]["resign"]
    played = [(g["action"], g["P"], g["V"], g["R"]) for g in got if not g["resign"]]
    return played, resigned, resigned or env.terminal()


def games_of(lines, records, games, moves):
    """per game: the first finished record if the game has ended, else the record as it stands -> ([(action, P, V, R)], finished, SD tag or None)"""
    out = []
    for g in range(games):
        done = len(lines) >= games
        rec = lines[g] if done else records[g]
        mv = parse_record(rec, moves)
        sd = SEED.search(rec)
        out.append((mv, done and len(MOVE.findall(rec)) <= moves, int(sd.group(1)) if sd else None))
    return out


def check_against(model, games):
    """the comparison of §2b / §3: every game equals the model (and so its neighbours): moves, P, V, R as strings, and whether the game ended where the model's
    did.  `model` is the model's game, or for games that differ by their seed a function from a game's SD tag to the model's game of that seed"""
    for g, (mv, done, sd) in enumerate(games):
        played, resigned, finished = model(sd) if callable(model) else model
        assert [m[0] for m in mv] == [m[0] for m in played], f"game {g}: actions {[m[0] for m in mv]} != model {[m[0] for m in played]}"
        for k, (a, b) in enumerate(zip(mv, played)):
            assert a[2] == b[2], f"game {g} move {k}: V {a[2]} != model {b[2]}"
            assert a[1] == b[1], f"game {g} move {k}: P differs from the model: {sorted(set(a[1].items()) ^ set(b[1].items()))}"
            assert b[3] is None or a[3] == b[3], f"game {g} move {k}: R {a[3]} != model {b[3]}"
        assert done == finished, f"game {g}: ended {done}, model {finished} (resigned {resigned})"


def oracle_games(oracle, conf, desc_args, w, games, moves):
    cfg = model_cfg(conf)[0]
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    og = oracle.OracleGroup(full_conf(conf, games), od, w)
    og.cycles((cfg.actor_num_simulation + 1) * (moves + 1))
    return games_of(og.lines(), og.peek_records(games), games, moves)


_MODEL_CACHE = {}


def model_of(oracle, name, wseed, env_seed=None):
    """the model's games are computed once and shared (the GPU file asks for the same ones)"""
    if (name, wseed, env_seed) not in _MODEL_CACHE:
        conf, desc_args, _, moves, _, vgain = row(name)
        trace = {}
        _MODEL_CACHE[name, wseed, env_seed] = expected_from_model(oracle, conf, desc_args, wseed, moves, weights=case_weights(oracle, desc_args, wseed, vgain),
                                                                  env_seed=env_seed, trace=trace, env=make_env(oracle, conf, rules=True) if name in GAME_CASES else None)
        _MODEL_CACHE["env", name, wseed, env_seed] = trace["env"]
    return _MODEL_CACHE[name, wseed, env_seed]


def model_env_of(oracle, name, wseed):
    """the environment as the model's game of a row left it (a RuleEnv for the rows of GAME_CASES: its final position and the terminal leaves of its searches)"""
    model_of(oracle, name, wseed)
    return _MODEL_CACHE["env", name, wseed, None]


def case_model(oracle, name, wseed):
    """what check_against takes for a row: the one game all games of the pool play, or for an Atari-shaped row the game of each seed"""
    if is_atari(row(name)[0]):
        return lambda sd: model_of(oracle, name, wseed, sd)
    return model_of(oracle, name, wseed)


def check_atari_pool_shows_something(games):
    """A multi-move Atari-shaped row must show a reward of 1 and, at some move, two different V strings over its games: without the first the reward's way
    into the backup and the R tag goes unseen, without the second a leak between games does"""
    assert all(sd is not None for _, _, sd in games) and len({sd for _, _, sd in games}) == len(games)
    assert any(m[3] == "1" for mv, _, _ in games for m in mv), "no game of the pool earned a reward"
    assert any(len({mv[k][2] for mv, _, _ in games}) > 1 for k in range(min(len(mv) for mv, _, _ in games))), "all games have the same values"


ALL_CASES = [(name, s) for name, c in CASES.items() for s in c[2]]


@pytest.mark.parametrize("name,wseed", ALL_CASES, ids=lambda x: str(x))
def test_model_equals_oracle(oracle, name, wseed):
    """§2b; an AmbiguousOrder raised by the model fails the case: the committed seeds raise none"""
    conf, desc_args, _, moves, games, vgain = CASES[name]
    model = case_model(oracle, name, wseed)
    got = oracle_games(oracle, conf, desc_args, case_weights(oracle, desc_args, wseed, vgain), games, moves)
    check_against(model, got)
    if callable(model):
        check_atari_pool_shows_something(got)
        assert all(len(model(sd)[0]) == moves and model(sd)[2] for _, _, sd in got)
    else:
        assert len(model[0]) >= 1 or model[1]


RULES_CASES = [(n, s) for n, s in ALL_CASES if n.startswith(("go", "othello", "ttt"))]


@pytest.mark.parametrize("name,wseed", RULES_CASES, ids=lambda x: str(x))
def test_first_move_rows_on_the_rules_models(oracle, name, wseed):
    """the Go, Othello and TicTacToe rows of CASES played by the model in the rules models' environment (tests/rule_envs.py) give the same games as in the
    oracle's: actions, P, V and R strings, and where the game ended"""
    conf, desc_args, _, moves, _, vgain = CASES[name]
    got = expected_from_model(oracle, conf, desc_args, wseed, moves, weights=case_weights(oracle, desc_args, wseed, vgain), env=make_env(oracle, conf, rules=True))
    assert got == model_of(oracle, name, wseed)


def test_resign_case_resigns_and_plays(oracle):
    """the PUCT case is there for max count, P counts and the resign test: over its seeds the model must both play moves and resign"""
    outcomes = [model_of(oracle, "go_puct_n24_resign", s) for s in CASES["go_puct_n24_resign"][2]]
    assert any(o[1] for o in outcomes) and any(len(o[0]) > 0 for o in outcomes)


def test_model_cfg_reads_every_key():
    """a case is defined by its configuration string alone: every key of the model's Cfg comes out of it"""
    keys = dict(actor_num_simulation=(9, "9"), actor_mcts_puct_base=(100.0, "100"), actor_mcts_puct_init=(2.5, "2.5"), actor_mcts_reward_discount=(0.997, "0.997"),
                actor_mcts_value_rescale=(True, "true"), actor_mcts_value_flipping_player=(S.BLACK, "B"), actor_use_gumbel=(True, "true"),
                actor_gumbel_sample_size=(5, "5"), actor_gumbel_sigma_visit_c=(40.0, "40"), actor_gumbel_sigma_scale_c=(0.1, "0.1"),
                actor_use_dirichlet_noise=(True, "true"), actor_dirichlet_noise_epsilon=(0.5, "0.5"), actor_resign_threshold=(-2.0, "-2"), atari_init_q=(True, "true"))
    assert set(keys) == set(vars(S.Cfg()))
    cfg = model_cfg("env_game=go:" + ":".join(f"{k}={v[1]}" for k, v in keys.items()))[0]
    assert vars(cfg) == {k: v[0] for k, v in keys.items()}
    quiet = model_cfg("env_game=go")[0]
    assert vars(quiet) == dict(vars(S.Cfg()), actor_use_dirichlet_noise=False)


# ---------------------------------------------------------------------------------------------
# c. the noisy first move
# ---------------------------------------------------------------------------------------------
def noise_draws(oracle, kind, seed, games, nc, alpha=0.0):
    """the first `games` vectors of nc values of the Gumbel stream (kind 3 of mzo_rng_vector) or the Dirichlet stream (kind 2), both pinned to the reference in
    tests/golden/ref_rng_rotation_config.json"""
    out = np.zeros(games * nc, np.float64)
    oracle.lib().mzo_rng_vector(seed, {"dirichlet": 2, "gumbel": 3}[kind], games * nc, nc, alpha, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out.astype(np.float32).reshape(games, nc)


def noisy_model(oracle, name, g, env_seed=None):
    """With rotation off, selection by count and one RNG stream, nothing draws from the slave thread's generator (seeded program_seed + 0, actor_group.cpp:66-70)
    before the first root is expanded: the resign coin of the first reset() comes from the main thread's generator (actor_group.cpp:179-187), and so does the
    seed an Atari-shaped game draws there.  The actors expand their first roots in index order in the second cycle, so game g takes draws [g * nc, (g + 1) * nc)
    of the noise stream, Gumbel or Dirichlet; test_noisy_first_move establishes it on the oracle by playing eight different first moves right."""
    if ("noisy", name, g, env_seed) not in _MODEL_CACHE:
        conf, desc_args, wseed, kind = noisy_row(name)
        cfg, _, kv = model_cfg(conf)
        assert (kind == "dirichlet") == cfg.actor_use_dirichlet_noise and (kind == "gumbel") == (kv.get("actor_use_gumbel_noise") == "true")
        nc = int(np.sum(make_env(oracle, conf, env_seed).legal()))
        draws = noise_draws(oracle, kind, int(kv["program_seed"]), NOISY_GAMES, nc, float(kv.get("actor_dirichlet_noise_alpha", 0.03)))
        _MODEL_CACHE["noisy", name, g, env_seed] = expected_from_model(oracle, conf, desc_args, wseed, 1, first_noise=draws[g], env_seed=env_seed)
    return _MODEL_CACHE["noisy", name, g, env_seed]


def check_noisy(oracle, name, games):
    """every game against the model under its own noise vector (and in its own Atari-shaped game) -> the set of first actions"""
    assert len(games) == NOISY_GAMES
    first = set()
    for g, game in enumerate(games):
        assert (game[2] is not None) == is_atari(noisy_row(name)[0])
        model = noisy_model(oracle, name, g, game[2])
        check_against(model, [game])
        first.add(model[0][0][0])
    return first


@pytest.mark.parametrize("name", list(NOISY))
def test_noisy_first_move(oracle, name):
    conf, desc_args, wseed, _ = NOISY[name]
    first_actions = check_noisy(oracle, name, oracle_games(oracle, conf, desc_args, case_weights(oracle, desc_args, wseed), NOISY_GAMES, 1))
    assert len(first_actions) > 1, "eight noise vectors that all lead to one first move show nothing"
