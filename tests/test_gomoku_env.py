"""Gomoku's host rules engine (env.cpp Gomoku; ref environment/gomoku/gomoku.cpp) on the CPU: known answers from the rule text, then random playouts
against the pure-Python restatement of the rules (tests/gomoku_rules.py) under all four rule combinations — legal mask, turn, terminal flag, result
and the 4 feature planes (float and bit-packed) under every rotation.  Also: a Go configuration that carries the two Gomoku keys plays unchanged."""
import numpy as np
import pytest

import gomoku_rules as R

RULES = [("standard", True), ("standard", False), ("outer_open", True), ("outer_open", False)]


def _conf(n=15, rule="standard", five=True):
    return f"env_game=gomoku:env_board_size={n}:env_gomoku_rule={rule}:env_gomoku_exactly_five_stones={'true' if five else 'false'}"


def _p(x, y, n=15):
    return y * n + x


def _play(mz, conf, black, white, n=15):
    """Black and white alternate from black: black[0], white[0], black[1], ... (len(white) is len(black) or one less); every move must be accepted
    and none may come after the end of the game."""
    assert len(white) in (len(black), len(black) - 1)
    moves = [m for pair in zip(black, white) for m in pair] + ([black[-1]] if len(white) < len(black) else [])
    env = mz.Env(conf)
    for i, m in enumerate(moves):
        assert not env.is_terminal(), f"the game ended before move {i}"
        assert env.act(_p(*m, n)), f"move {i} refused"
    return env


FILLER = [(0, 14), (2, 14), (4, 14), (6, 14), (8, 14), (10, 14), (12, 14), (14, 12), (14, 10)]  # white stones that form no line of five


@pytest.mark.parametrize("line", [
    [(3, 7), (4, 7), (6, 7), (7, 7), (5, 7)],        # a row, completed in the middle
    [(1, 0), (2, 0), (3, 0), (4, 0), (0, 0)],        # a row, completed at the edge
    [(14, 5), (14, 6), (14, 7), (14, 8), (14, 4)],   # a column on the right edge
    [(1, 1), (2, 2), (4, 4), (5, 5), (3, 3)],        # the diagonal (1, 1)
    [(5, 1), (4, 2), (2, 4), (1, 5), (3, 3)],        # the diagonal (1, -1)
])
def test_five_in_a_row_wins(mz, line):
    env = _play(mz, _conf(), line[:4], FILLER[:4])
    assert not env.is_terminal() and env.eval_score() == 0.0  # four in a row does not win
    assert env.act(_p(*line[4]))
    assert env.is_terminal() and env.eval_score() == 1.0 and env.turn() == 2


def test_white_five_scores_minus_one(mz):
    white = [(3, 3), (3, 4), (3, 5), (3, 6), (3, 7)]
    black = [(10, 0), (12, 0), (10, 2), (12, 2), (10, 4)]
    env = _play(mz, _conf(), black, white)
    assert env.is_terminal() and env.eval_score() == -1.0 and env.turn() == 1


def test_overline(mz):
    six = [(2, 7), (3, 7), (4, 7), (6, 7), (7, 7), (5, 7)]
    env = _play(mz, _conf(five=True), six, FILLER[:5])
    assert not env.is_terminal() and env.eval_score() == 0.0  # exactly five: a six does not win ...
    assert env.act(_p(9, 9))                                  # ... and play continues
    env = _play(mz, _conf(five=False), six, FILLER[:5])
    assert env.is_terminal() and env.eval_score() == 1.0      # freestyle: it wins
    # a six on the row and exactly five on the column through the same stone: a win under exactly-five
    black = [(2, 7), (3, 7), (4, 7), (6, 7), (7, 7), (5, 3), (5, 4), (5, 5), (5, 6), (5, 7)]
    env = _play(mz, _conf(five=True), black, FILLER[:9])
    assert env.is_terminal() and env.eval_score() == 1.0


def test_full_board(mz):
    env = mz.Env(_conf(4))  # no line of five fits: the full board is a draw
    for a in range(16):
        assert not env.is_terminal()
        assert env.act(a)
    assert env.is_terminal() and env.eval_score() == 0.0
    # 5x5, the last empty point completes black's five: a win, not a draw
    rows = ["_BBBB", "BBWWW", "WWBBW", "BWWWB", "WBWBW"]
    black = [(x, y) for y in range(5) for x in range(5) if rows[y][x] == "B"]
    white = [(x, y) for y in range(5) for x in range(5) if rows[y][x] == "W"]
    env = _play(mz, _conf(5), black + [(0, 0)], white, n=5)
    assert env.is_terminal() and env.eval_score() == 1.0 and env.legal_mask().sum() == 0


def test_resign_eval(mz):
    env = mz.Env(_conf())
    assert env.eval_score(resign=True) == -1.0  # black to move resigns: white is scored
    assert env.act(_p(7, 7))
    assert env.eval_score(resign=True) == 1.0 and env.eval_score() == 0.0


def test_outer_open(mz):
    env = mz.Env(_conf(rule="outer_open"))
    m = env.legal_mask()
    assert len(m) == 225 and m.sum() == 104  # the outer two rings of 15x15: 225 - 11 * 11
    assert m[_p(0, 0)] and m[_p(1, 7)] and m[_p(13, 13)] and not m[_p(2, 2)] and not m[_p(7, 7)]
    assert not env.act(_p(7, 7))  # refused, nothing changes
    assert env.turn() == 1 and env.legal_mask().sum() == 104
    assert env.act(_p(0, 0))
    m = env.legal_mask()
    assert m.sum() == 224 and m[_p(7, 7)] and not m[_p(0, 0)]  # the second move: any empty point
    # the rule counts moves played, not whose turn it is: a first move by white is restricted too
    env = mz.Env(_conf(rule="outer_open"))
    assert not env.act(_p(7, 7), player=2) and env.act(_p(14, 14), player=2) and env.turn() == 1
    assert env.act(_p(7, 7))
    # any other rule value is the standard rule (the reference does not validate it)
    env = mz.Env("env_game=gomoku:env_gomoku_rule=renju")
    assert env.legal_mask().sum() == 225 and env.name() == "gomoku_15x15"


def test_action_strings_names_and_sizes(mz):
    env = mz.Env(_conf())
    assert env.policy_size() == 225  # no pass action
    assert env.action_from_string("A1") == 0 and env.action_from_string("H1") == 7 and env.action_from_string("J1") == 8  # I is skipped
    assert env.action_from_string("P15") == 224 and env.action_from_string("h8") == _p(7, 7)
    assert env.action_from_string("pass") == -1 and env.action_from_string("PASS") == -1
    assert mz.Env("env_game=gomoku").name() == "gomoku_15x15"
    assert mz.Env("env_game=gomoku:env_gomoku_rule=outer_open").name() == "gomoku_oo_15x15"
    assert mz.Env("env_game=gomoku:env_board_size=19:env_gomoku_rule=outer_open").name() == "gomoku_oo_19x19"
    assert mz.Env("env_game=gomoku:env_board_size=9").name() == "gomoku_9x9"
    assert mz.Env("env_game=gomoku:env_board_size=3").policy_size() == 9  # smaller boards are accepted, as in the reference
    with pytest.raises(mz.MzError, match="gomoku board size 20"):
        mz.Env("env_game=gomoku:env_board_size=20")
    with pytest.raises(mz.MzError):
        mz.Env("env_game=gomoku:env_gomoku_exactly_five_stones=maybe")


def _compare(env, model, rot, where):
    n = model.n
    assert env.turn() == model.turn, where
    assert env.is_terminal() == model.is_terminal(), where
    assert env.eval_score() == model.eval_score(), where
    assert env.eval_score(resign=True) == model.eval_score(resign=True), where
    assert np.array_equal(env.legal_mask(), model.legal_mask()), where
    assert np.array_equal(env.features(rot), model.features(rot)), where
    assert np.array_equal(env.feature_bits(rot, 4, n * n), model.feature_bits(rot)), where


@pytest.mark.parametrize("n,games", [(15, 3), (9, 4), (5, 8)])
@pytest.mark.parametrize("rule,five", RULES)
def test_random_playouts_against_the_rules_model(mz, n, games, rule, five):
    rng = np.random.default_rng(1000 * n + 10 * RULES.index((rule, five)))
    ended = {"win": 0, "full": 0}
    for g in range(games):
        env, model = mz.Env(_conf(n, rule, five)), R.Gomoku(n, rule == "outer_open", five)
        ply = 0
        while True:
            where = f"{n}x{n} {rule} five={five} game {g} ply {ply} moves {model.actions}"
            _compare(env, model, int(rng.integers(8)), where)
            if model.is_terminal():
                ended["win" if model.winner else "full"] += 1
                break
            illegal = [a for a in range(n * n) if not model.is_legal(a)]
            if illegal:  # refused, and nothing changes
                bad = int(rng.choice(illegal))
                assert not env.act(bad), where
                assert env.turn() == model.turn and np.array_equal(env.legal_mask(), model.legal_mask()), where
            a = int(rng.choice(np.nonzero(model.legal_mask())[0]))
            assert env.act(a) and model.act(a), where
            ply += 1
    for r in range(8):  # the last position under every rotation
        _compare(env, model, r, f"{n}x{n} {rule} final position, rotation {r}")
    assert ended["win"] + ended["full"] == games


def test_go_configuration_ignores_the_gomoku_keys(mz):
    """The two keys are inert for every other game: the same Go game with and without them."""
    rng = np.random.default_rng(5)
    plain = mz.Env("env_game=go:env_board_size=9")
    keyed = mz.Env("env_game=go:env_board_size=9:env_gomoku_rule=outer_open:env_gomoku_exactly_five_stones=false")
    assert plain.policy_size() == keyed.policy_size() == 82
    for ply in range(60):
        m = plain.legal_mask()
        assert np.array_equal(m, keyed.legal_mask()) and np.array_equal(plain.features(ply % 8), keyed.features(ply % 8))
        if plain.is_terminal():
            break
        a = int(rng.choice(np.nonzero(m)[0]))
        assert plain.act(a) and keyed.act(a)
    assert plain.eval_score() == keyed.eval_score()
