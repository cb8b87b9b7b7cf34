"""The pure-Python rules models (tests/gomoku_rules.py, hex_rules.py, nogo_rules.py, havannah_rules.py, go_rules.py, othello_rules.py, tictactoe_rules.py)
behind the environment interface that
tests/search_model.py plays in: clone, act(a, player), num_players, turn, legal, terminal, eval_score, reward, features.  One adapter, configured by the
string the worker is configured with, so that a row of the case table is defined by one string for both sides.  This file imports neither the oracle nor
the product.

The keys read, with the defaults of config.cpp / game_kind.h: env_game; env_board_size (gomoku 15, hex 11, nogo 9, havannah 8 — Havannah's is the edge
size N, its planes and policy are those of the (2N - 1) x (2N - 1) array); env_gomoku_rule (standard; outer_open restricts the first move),
env_gomoku_exactly_five_stones (true), env_hex_use_swap_rule (true), env_havannah_use_swap_rule (true), env_go_komi (7.5), env_go_ko_rule (positional); Go's
board defaults to 9, Othello's to 8, TicTacToe's is 3.  Every other key of the string is someone else's.

What the search sees: legal() has the length of the network's policy (NoGo: n * n + 1 with the pass slot never legal; Go and Othello: n * n + 1 with the
pass; Havannah: (2N - 1)^2 with the cut-off cells never legal); features() is the flat float32 array at rotation 0; eval_score() and reward() are float32 and the reward is 0.  The adapter and
its clones share `stats`: every eval_score() call — the search asks for the score at a terminal leaf and nowhere else — is kept with the actions that led
to the position, so that a test can count the terminal leaves a game's searches backed up and replay them elsewhere.  For Go and Othello `stats` also
counts, over every legal() call that is not on a clone-free root — that is, inside a search — the superko refusals (Go: points the history-free rules would
allow) and the forced passes (Othello: the pass is the only legal action while the board is not full)."""
import copy

import numpy as np

from go_rules import Go
from gomoku_rules import Gomoku
from havannah_rules import Havannah
from hex_rules import Hex
from nogo_rules import NoGo
from othello_rules import Othello
from tictactoe_rules import TicTacToe

f32 = np.float32
GAMES = ("gomoku", "hex", "nogo", "havannah", "go", "othello", "tictactoe")
DEFAULT_BOARD = {"gomoku": 15, "hex": 11, "nogo": 9, "havannah": 8, "go": 9, "othello": 8, "tictactoe": 3}


def _flag(kv, key, default):
    v = kv.get(key, "true" if default else "false").upper()
    assert v in ("TRUE", "1", "FALSE", "0"), (key, kv[key])
    return v in ("TRUE", "1")


def parse(conf):
    """(game, board size, the constructor's keyword arguments) of a configuration string"""
    kv = dict(x.split("=", 1) for x in conf.split(":") if x)
    game = kv["env_game"]
    assert game in GAMES, game
    n = int(kv.get("env_board_size", 0)) or DEFAULT_BOARD[game]
    if game == "gomoku":
        return game, n, dict(outer_open=kv.get("env_gomoku_rule", "standard") == "outer_open", exactly_five=_flag(kv, "env_gomoku_exactly_five_stones", True))
    if game == "hex":
        return game, n, dict(swap=_flag(kv, "env_hex_use_swap_rule", True))
    if game == "havannah":
        return game, n, dict(swap=_flag(kv, "env_havannah_use_swap_rule", True))
    if game == "go":
        return game, n, dict(komi=float(kv.get("env_go_komi", 7.5)), ko_rule=kv.get("env_go_ko_rule", "positional"))
    if game == "tictactoe":
        assert n == 3
    return game, n, {}


def policy_size(conf):
    game, n, _ = parse(conf)
    return {"gomoku": n * n, "hex": n * n, "nogo": n * n + 1, "havannah": (2 * n - 1) ** 2, "go": n * n + 1, "othello": n * n + 1, "tictactoe": 9}[game]


class TicTacToeModel:
    """tests/tictactoe_rules.py behind the interface of the other models"""

    def __init__(self, n=3, t=None):
        self.t = TicTacToe() if t is None else t

    turn = property(lambda self: self.t.turn())

    def clone(self): return TicTacToeModel(t=self.t.clone())

    def act(self, a, player):
        if not (0 <= a < 9) or self.t.board[a] != 0:
            return False
        self.t.act(a, player)
        return True

    def legal_mask(self): return np.array(self.t.legal(), np.uint8)
    def is_terminal(self): return self.t.terminal()
    def eval_score(self): return self.t.eval_score()
    def features(self, rot=0): return self.t.features()


def _copy_model(m):
    """a model's mutable state one level deep (its lists, dicts and tuples of sets); what is never changed in place — Havannah's cell sets, the rows of
    NoGo's history — stays shared"""
    if hasattr(m, "clone"):
        return m.clone()
    c = copy.copy(m)
    for k, v in vars(m).items():
        if isinstance(v, list):
            setattr(c, k, list(v))
        elif isinstance(v, dict):
            setattr(c, k, dict(v))
        elif isinstance(v, tuple) and v and isinstance(v[0], set):
            setattr(c, k, tuple(set(s) for s in v))
    return c


class RuleEnv:
    def __init__(self, conf, _from=None):
        if _from is not None:
            self.game, self.n, self.model, self.hist, self.stats = _from.game, _from.n, _copy_model(_from.model), list(_from.hist), _from.stats
            self.in_search = True
            return
        self.game, self.n, kw = parse(conf)
        self.model = {"gomoku": Gomoku, "hex": Hex, "nogo": NoGo, "havannah": Havannah, "go": Go, "othello": Othello, "tictactoe": TicTacToeModel}[self.game](self.n, **kw)
        self.hist = []
        self.in_search = False  # a clone is a position inside a search
        # shared with every clone: (the actions that led there, the score) of every eval_score() call; legal() calls of clones that show a superko refusal
        # (Go) or a forced pass (Othello)
        self.stats = {"terminal_leaves": [], "superko_in_tree": 0, "forced_pass_in_tree": 0}

    def clone(self): return type(self)(None, _from=self)

    def act(self, a, player):
        assert player == self.model.turn, f"{self.game}: player {player} moves out of turn after {self.hist}"
        ok = self.model.act(a) if self.game == "havannah" else self.model.act(a, player)
        assert ok, f"{self.game}: action {a} of player {player} refused after {self.hist}"
        self.hist.append(int(a))

    def num_players(self): return 2
    def turn(self): return self.model.turn

    def legal(self):
        m = self.model.legal_mask()
        if self.in_search and self.game == "go":
            self.stats["superko_in_tree"] += any(isinstance(self.model.refusal(a), tuple) for a in np.flatnonzero(m[:-1] == 0))
        if self.in_search and self.game == "othello":
            self.stats["forced_pass_in_tree"] += bool(m[-1]) and 0 in self.model.board
        return m

    def terminal(self): return bool(self.model.is_terminal())

    def eval_score(self):
        self.stats["terminal_leaves"].append((tuple(self.hist), self.score()))
        return self.score()

    def score(self): return f32(self.model.eval_score())  # (uncounted: for the tests)
    def reward(self): return f32(0)

    def features(self):
        f = self.model.features() if self.game == "havannah" else self.model.features(0)
        assert f.dtype == np.float32 and f.ndim == 1
        return f

    def action_features(self, a, player):
        """ref go.cpp:310-315, othello.cpp:257-262: one plane with the action's point, empty for the pass"""
        assert self.game in ("go", "othello", "tictactoe")
        f = np.zeros(self.n * self.n, np.float32)
        if a < self.n * self.n:
            f[a] = 1
        return f
