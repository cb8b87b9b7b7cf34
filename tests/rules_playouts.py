"""The playout table of the Go and Othello rules models (tests/go_rules.py, tests/othello_rules.py): whole games played BY THE MODEL, with a policy that
seeks captures, and what they show, counted on the model alone.  tests/test_go_model.py and tests/test_othello_model.py hold the host engine and the
oracle to these games move by move; tests/test_gpu_go_model.py holds the device engine to them.  This file imports neither the oracle nor the product.

The Go policy, per move: with probability 1/2 a uniformly random choice among the legal points that capture, if there are any; else a pass with the
row's pass probability; else a uniformly random legal point (a pass if there is none).  Othello's moves are uniformly random among the legal actions."""
import numpy as np

from go_rules import Go
from othello_rules import Othello

# name -> (board, ko rule, komi, pass probability, games, first seed).  The seeds were chosen until the conditions of
# test_go_model.py::test_what_the_playout_table_shows and test_othello_model.py::test_what_the_playout_table_shows hold.
GO_ROWS = {
    "go2_pos": (2, "positional", 0.5, 0.10, 30, 200),
    "go2_sit": (2, "situational", 0.5, 0.10, 30, 230),
    "go3_pos_komi9": (3, "positional", 9.0, 0.15, 40, 300),   # Black owning the board is a draw
    "go3_sit": (3, "situational", 0.5, 0.05, 40, 340),
    "go5_pos": (5, "positional", 0.5, 0.03, 30, 500),
    "go5_sit": (5, "situational", 7.5, 0.03, 30, 530),
    "go5_pos_nopass": (5, "positional", 0.5, 0.0, 6, 560),    # to the move cap
    "go8_pos": (8, "positional", 7.5, 0.02, 6, 800),
    "go8_sit": (8, "situational", 0.5, 0.02, 4, 810),
    "go9_pos": (9, "positional", 7.5, 0.02, 6, 900),
    "go9_sit": (9, "situational", 0.5, 0.02, 4, 910),
    "go9_pos_nopass": (9, "positional", 7.5, 0.0, 2, 920),
    "go11_pos": (11, "positional", 0.5, 0.01, 2, 1100),
    "go11_sit": (11, "situational", 7.5, 0.01, 1, 1110),
    "go13_pos": (13, "positional", 7.5, 0.01, 2, 1300),
    "go13_sit": (13, "situational", 0.5, 0.01, 1, 1310),
    "go16_pos": (16, "positional", 7.5, 0.005, 1, 1600),      # P = 256: exactly four 64-bit words
    "go16_sit": (16, "situational", 0.5, 0.005, 1, 1610),
    "go19_pos_nopass": (19, "positional", 7.5, 0.0, 1, 1900),  # 723 actions: the fullest superko table
    "go19_sit": (19, "situational", 0.5, 0.003, 1, 1910),
}
OTHELLO_ROWS = {"othello4": (4, 60, 40), "othello6": (6, 20, 60), "othello8": (8, 12, 80)}  # name -> (board, games, first seed)


def other_rule(rule):
    return "situational" if rule == "positional" else "positional"


def play_go(n, ko_rule, komi, pass_prob, seed):
    """One game by the model: (actions, events).  The events are counted over the game's positions, for the player to move."""
    rng = np.random.default_rng(seed)
    g = Go(n, komi, ko_rule)
    twin = Go(n, komi, other_rule(ko_rule)) if n <= 5 else None  # the same game under the other ko rule, while it stays legal there
    P = n * n
    ev = dict(max_capture=0, multi_block_captures=0, suicide_single=0, suicide_multi=0, simple_ko=0, long_superko=0, ko_rules_differ=0, passes=0)
    actions = []
    while not g.is_terminal():
        why = [g.refusal(a) for a in range(P)]
        legal = [a for a in range(P) if why[a] is None]
        for a in range(P):
            if why[a] == "suicide":
                alone = not any(g.board[q] == g.turn for q in g.neighbours(a))
                ev["suicide_single" if alone else "suicide_multi"] += 1
            elif isinstance(why[a], tuple):
                ev["simple_ko" if why[a][1] == 2 else "long_superko"] += 1
        if twin is not None and legal != [a for a in range(P) if twin.is_legal(a)]:
            ev["ko_rules_differ"] += 1
        capturing = {a: g.place(a, g.turn)[1] for a in legal if not g._quiet(a, g.turn)}
        capturing = {a: c for a, c in capturing.items() if c}
        if capturing and rng.random() < 0.5:
            a = int(rng.choice(sorted(capturing)))
        elif rng.random() < pass_prob or not legal:
            a = P
        else:
            a = int(rng.choice(legal))
        if a in capturing:
            ev["max_capture"] = max(ev["max_capture"], sum(len(b) for b in capturing[a]))
            ev["multi_block_captures"] += len(capturing[a]) >= 2
        ev["passes"] += a == P
        assert g.act(a)
        if twin is not None and not twin.act(a):
            twin = None
        actions.append(a)
    ev["ended_by"] = "passes" if actions[-2:] == [P, P] else "cap"
    ev["result"] = g.eval_score()
    ev["length"] = len(actions)
    return actions, ev


def play_othello(n, seed):
    rng = np.random.default_rng(seed)
    g = Othello(n)
    P = n * n
    ev = dict(forced_pass_midgame=0)
    actions = []
    while not g.is_terminal():
        legal = np.flatnonzero(g.legal_mask())
        a = int(rng.choice(legal))
        if a == P and g.can_place(3 - g.turn):
            ev["forced_pass_midgame"] += 1
        assert g.act(a)
        actions.append(a)
    ev["empty_at_end"] = g.board.count(0)
    ev["result"] = g.eval_score()
    ev["length"] = len(actions)
    return actions, ev


_CACHE = {}


def go_games(name):
    """[(seed, actions, events)] of a row, played once and shared"""
    if name not in _CACHE:
        n, rule, komi, pass_prob, games, seed0 = GO_ROWS[name]
        _CACHE[name] = [(seed0 + i,) + play_go(n, rule, komi, pass_prob, seed0 + i) for i in range(games)]
    return _CACHE[name]


def othello_games(name):
    if name not in _CACHE:
        n, games, seed0 = OTHELLO_ROWS[name]
        _CACHE[name] = [(seed0 + i,) + play_othello(n, seed0 + i) for i in range(games)]
    return _CACHE[name]


def go_row_summary(name):
    """what a row shows, summed (or maximised) over its games"""
    games = go_games(name)
    out = {k: (max if k == "max_capture" else sum)(e[k] for _, _, e in games) for k in games[0][2] if k not in ("ended_by", "result", "length")}
    out["ended_by_passes"] = sum(e["ended_by"] == "passes" for _, _, e in games)
    out["ended_by_cap"] = sum(e["ended_by"] == "cap" for _, _, e in games)
    for r, key in ((1.0, "black_wins"), (-1.0, "white_wins"), (0.0, "draws")):
        out[key] = sum(e["result"] == r for _, _, e in games)
    out["longest"] = max(e["length"] for _, _, e in games)
    return out
