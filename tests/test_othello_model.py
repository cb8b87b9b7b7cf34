"""The host engine (minizero_amd/csrc/env.cpp) and the oracle's restatement (oracle/o_env.cpp) of Othello, each held to the rules model of
tests/othello_rules.py, which shares no code and no data structure with either: every action sequence of the 4x4 board to depth 6, and whole uniformly random
games on 4x4, 6x6 and 8x8 (tests/rules_playouts.py) — legal mask, terminal flag, result (at every position: 0 while either side can place), player to move,
and the 4 planes under all 8 rotations.  Every comparison is exact."""
import pytest

from othello_rules import Othello
import rules_playouts as R
from test_go_model import check_position, exhaustive


def engines(mz, oracle, n):
    conf = f"env_game=othello:env_board_size={n}"
    return {"host engine": mz.Env(conf), "oracle": oracle.OracleEnv(conf)}


def test_every_sequence_of_4x4_to_depth_6(mz, oracle):
    model = Othello(4)
    start = list(model.board)
    counts = exhaustive(model, engines(mz, oracle, 4), 6)
    print(f"othello 4x4: sequences per depth {counts}")
    assert counts[:3] == [1, 4, 12]  # the four openings are one under the board's symmetries, and each has three answers
    assert model.board == start and model.actions == []


def test_the_start(mz, oracle):
    """Black on the lower-left and upper-right of the centre (othello.cpp:22-26), no pass at the start (:17)"""
    for n in (4, 6, 8):
        g, h = Othello(n), n // 2
        assert [p for p in range(n * n) if g.board[p] == 1] == [(h - 1) * n + h - 1, h * n + h]
        assert [p for p in range(n * n) if g.board[p] == 2] == [(h - 1) * n + h, h * n + h - 1]
        assert sorted(g.legal_mask().nonzero()[0]) == sorted([(h - 1) * n + h + 1, (h - 2) * n + h, h * n + h - 2, (h + 1) * n + h - 1])
        check_position(g, engines(mz, oracle, n), f"start of {n}x{n}", range(8))


@pytest.mark.parametrize("name", list(R.OTHELLO_ROWS))
def test_random_playouts(mz, oracle, name):
    n = R.OTHELLO_ROWS[name][0]
    for seed, actions, _ in R.othello_games(name):
        model, envs = Othello(n), engines(mz, oracle, n)
        for i, a in enumerate(actions):
            assert model.act(a)
            for e_name, e in envs.items():
                assert e.act(a), f"{e_name} refuses action {i} = {a} of {name} seed {seed}"
            check_position(model, envs, f"{name} seed {seed} after {actions[:i + 1]}", range(8))
        assert model.is_terminal() and actions[-2:] == [n * n, n * n]


def test_what_the_playout_table_shows():
    """counted on the model alone: a forced pass in mid-game, a game that ends on a board that is not full, all three results, a draw on 4x4"""
    games = [e for name in R.OTHELLO_ROWS for _, _, e in R.othello_games(name)]
    for name in R.OTHELLO_ROWS:
        g = [e for _, _, e in R.othello_games(name)]
        print(name, dict(games=len(g), forced_pass_midgame=sum(e["forced_pass_midgame"] for e in g), ended_not_full=sum(e["empty_at_end"] > 0 for e in g),
                         black_wins=sum(e["result"] == 1 for e in g), white_wins=sum(e["result"] == -1 for e in g), draws=sum(e["result"] == 0 for e in g)))
    assert sum(e["forced_pass_midgame"] for e in games) >= 1
    assert any(e["empty_at_end"] > 0 for e in games)
    assert {e["result"] for e in games} == {1.0, -1.0, 0.0}
    assert any(e["result"] == 0.0 for _, _, e in R.othello_games("othello4"))
