"""The search model of tests/search_model.py (a third implementation, written from the reference's text) pinned by paper-and-pencil literals, then compared with
the oracle's search as exact strings: action played, P tag, V tag, resignation, move by move.  The same table of configurations runs against the HIP worker in
tests/test_gpu_search_model.py.  Nothing here compares with a tolerance."""
import ctypes as C
import re

import numpy as np
import pytest

import hand_cases as H
from helpers import sharpen
import search_model as S

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


class TicTacToe:
    """environment/tictactoe/tictactoe.cpp: rules, result and the four planes (own, opponent, player 1 to move, player 2 to move)"""
    LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]

    def __init__(self, board=None, to_move=1):
        self.board, self.to_move = list(board or [0] * 9), to_move

    def clone(self): return TicTacToe(self.board, self.to_move)

    def act(self, a, player):
        assert self.board[a] == 0
        self.board[a], self.to_move = player, 3 - player

    def turn(self): return self.to_move
    def legal(self): return [int(b == 0) for b in self.board]

    def winner(self):
        for i, j, k in self.LINES:
            if self.board[i] and self.board[i] == self.board[j] == self.board[k]:
                return self.board[i]
        return 0

    def terminal(self): return self.winner() != 0 or 0 not in self.board
    def eval_score(self): return f32({0: 0.0, 1: 1.0, 2: -1.0}[self.winner()])
    def reward(self): return f32(0)

    def features(self):
        me, you = self.to_move, 3 - self.to_move
        return np.array([b == me for b in self.board] + [b == you for b in self.board] + [me == 1] * 9 + [me == 2] * 9, np.float32)

    def action_features(self, a, player):
        f = np.zeros(9, np.float32)
        f[a] = 1
        return f


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


def _gumbel(n, m, noise=False):
    return f":actor_num_simulation={n}:actor_use_gumbel=true:actor_gumbel_sample_size={m}:actor_use_gumbel_noise={'true' if noise else 'false'}"


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

# the noisy first move: (configuration, network, weight seed, action count of the first position)
NOISY = {
    "ttt": ("env_game=tictactoe" + _gumbel(16, 4, True), TTT16, 1),
    "othello": ("env_game=othello:env_board_size=8" + _gumbel(16, 16, True), OTH8, 1),
    "go": ("env_game=go:env_board_size=9" + _gumbel(50, 16, True), GO8, 1),
}
NOISY_GAMES = 8

MOVE = re.compile(r";([BW])\[(\d+)\]P\[([^\]]*)\]V\[([^\]]*)\]R\[[^\]]*\]")


def model_cfg(conf):
    kv = dict(x.split("=", 1) for x in conf.split(":") if x)
    kw = dict(actor_num_simulation=int(kv.get("actor_num_simulation", 50)), actor_use_gumbel=kv.get("actor_use_gumbel") == "true",
              actor_gumbel_sample_size=int(kv.get("actor_gumbel_sample_size", 16)), actor_resign_threshold=float(kv.get("actor_resign_threshold", -0.9)))
    return S.Cfg(**kw), kv.get("nn_type_name") == "muzero", kv


def case_weights(oracle, desc_args, wseed, vgain=None):
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    w = oracle.gen_weights(od, wseed)
    return w if vgain is None else sharpen(od, w, 1, vgain)


def make_env(oracle, conf):
    kv = model_cfg(conf)[2]
    if kv["env_game"] == "tictactoe":
        return TicTacToe()
    return OracleEnvAdapter(oracle, ":".join(f"{k}={kv[k]}" for k in ("env_game", "env_board_size") if k in kv))


def parse_record(record, moves):
    """[(action id, P dictionary, V string)] of the first `moves` moves of a record"""
    out = []
    for _, a, p, v in MOVE.findall(record)[:moves]:
        out.append((int(a), {int(x.split(":")[0]): x.split(":")[1] for x in p.split(",")} if p else {}, v))
    return out


def expected_from_model(oracle, conf, desc_args, wseed, moves, first_noise=None, weights=None, halvings=None):
    """what the model plays: ([(action, P, V)] of the moves played, resigned at the next search?, finished (terminal or resigned) within `moves`)"""
    cfg, muzero, _ = model_cfg(conf)
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    w = oracle.gen_weights(od, wseed) if weights is None else weights
    env = make_env(oracle, conf)
    got = S.play(cfg, env, NetAdapter(oracle.OracleNet(od, w)), moves, muzero, first_noise)
    resigned = bool(got) and got[-1]["resign"]
    played = [(g["action"], g["P"], g["V"]) for g in got if not g["resign"]]
    return played, resigned, resigned or env.terminal()


def games_of(lines, records, games, moves):
    """per game: the first finished record if the game has ended, else the record as it stands -> ([(action, P, V)], finished)"""
    out = []
    for g in range(games):
        done = len(lines) >= games
        rec = lines[g] if done else records[g]
        mv = parse_record(rec, moves)
        out.append((mv, done and len(MOVE.findall(rec)) <= moves))
    return out


def check_against(model, games):
    """the comparison of §2b / §3: every game equals the model (and so its neighbours): moves, P, V as strings, and whether the game ended where the model's did"""
    played, resigned, finished = model
    for g, (mv, done) in enumerate(games):
        assert [m[0] for m in mv] == [m[0] for m in played], f"game {g}: actions {[m[0] for m in mv]} != model {[m[0] for m in played]}"
        for k, (a, b) in enumerate(zip(mv, played)):
            assert a[2] == b[2], f"game {g} move {k}: V {a[2]} != model {b[2]}"
            assert a[1] == b[1], f"game {g} move {k}: P differs from the model: {sorted(set(a[1].items()) ^ set(b[1].items()))}"
        assert done == finished, f"game {g}: ended {done}, model {finished} (resigned {resigned})"


def oracle_games(oracle, conf, desc_args, w, games, moves):
    cfg = model_cfg(conf)[0]
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    og = oracle.OracleGroup(conf + f":zero_num_parallel_games={games}" + QUIET, od, w)
    og.cycles((cfg.actor_num_simulation + 1) * (moves + 1))
    return games_of(og.lines(), og.peek_records(games), games, moves)


_MODEL_CACHE = {}


def model_of(oracle, name, wseed):
    """the model's games are computed once and shared (the GPU file asks for the same ones)"""
    if (name, wseed) not in _MODEL_CACHE:
        conf, desc_args, _, moves, _, vgain = CASES[name]
        _MODEL_CACHE[name, wseed] = expected_from_model(oracle, conf, desc_args, wseed, moves, weights=case_weights(oracle, desc_args, wseed, vgain))
    return _MODEL_CACHE[name, wseed]


ALL_CASES = [(name, s) for name, c in CASES.items() for s in c[2]]


@pytest.mark.parametrize("name,wseed", ALL_CASES, ids=lambda x: str(x))
def test_model_equals_oracle(oracle, name, wseed):
    """§2b; an AmbiguousOrder raised by the model fails the case: the committed seeds raise none"""
    conf, desc_args, _, moves, games, vgain = CASES[name]
    model = model_of(oracle, name, wseed)
    check_against(model, oracle_games(oracle, conf, desc_args, case_weights(oracle, desc_args, wseed, vgain), games, moves))
    assert len(model[0]) >= 1 or model[1]


def test_resign_case_resigns_and_plays(oracle):
    """the PUCT case is there for max count, P counts and the resign test: over its seeds the model must both play moves and resign"""
    outcomes = [model_of(oracle, "go_puct_n24_resign", s) for s in CASES["go_puct_n24_resign"][2]]
    assert any(o[1] for o in outcomes) and any(len(o[0]) > 0 for o in outcomes)


# ---------------------------------------------------------------------------------------------
# c. the noisy first move
# ---------------------------------------------------------------------------------------------
def gumbel_draws(oracle, seed, games, nc):
    """the first games * nc values of the Gumbel stream (kind 3 of mzo_rng_vector, pinned to the reference in tests/golden/ref_rng_rotation_config.json)"""
    out = np.zeros(games * nc, np.float64)
    oracle.lib().mzo_rng_vector(seed, 3, games * nc, nc, 0.0, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out.astype(np.float32).reshape(games, nc)


def noisy_models(oracle, name):
    """With rotation off, selection by count and one RNG stream, nothing draws from the slave thread's generator (seeded program_seed + 0, actor_group.cpp:66-70)
    before the first root is expanded: the resign coin of the first reset() comes from the main thread's generator (actor_group.cpp:179-187).  The actors expand
    their first roots in index order in the second cycle, so game g takes draws [g * nc, (g + 1) * nc) of the Gumbel stream; test_noisy_first_move establishes
    it on the oracle by playing eight different first moves right."""
    if ("noisy", name) not in _MODEL_CACHE:
        conf, desc_args, wseed = NOISY[name]
        nc = int(np.sum(make_env(oracle, conf).legal()))
        draws = gumbel_draws(oracle, 7, NOISY_GAMES, nc)
        _MODEL_CACHE["noisy", name] = [expected_from_model(oracle, conf, desc_args, wseed, 1, first_noise=draws[g]) for g in range(NOISY_GAMES)]
    return _MODEL_CACHE["noisy", name]


def check_noisy(models, games):
    for g, game in enumerate(games):
        check_against(models[g], [game])
    return {m[0][0][0] for m in models}


@pytest.mark.parametrize("name", list(NOISY))
def test_noisy_first_move(oracle, name):
    conf, desc_args, wseed = NOISY[name]
    models = noisy_models(oracle, name)
    first_actions = check_noisy(models, oracle_games(oracle, conf, desc_args, case_weights(oracle, desc_args, wseed), NOISY_GAMES, 1))
    assert len(first_actions) > 1, "eight noise vectors that all lead to one first move show nothing"
