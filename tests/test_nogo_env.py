"""NoGo's host rules engine (env.cpp NoGo; ref environment/nogo/nogo.h over GoEnv) on the CPU: the known leaf counts of the move tree, positions by
hand in both colours, then random playouts against the pure-Python restatement of the rules (tests/nogo_rules.py) — legal mask, turn, terminal flag,
result and the 18 feature planes (float and bit-packed) under all eight rotations."""
import numpy as np
import pytest

import nogo_rules as R


def _conf(n=9):
    return f"env_game=nogo:env_board_size={n}"


# sequences of length 1, 2, ... from the empty board
COUNTS = {
    2: [4, 12, 16, 0],
    3: [9, 72, 496, 2832, 12768, 41328, 80352, 43776, 0],
    4: [16, 240, 3352, 43264, 511776],
    5: [25, 600, 13792, 302896],
    9: [81, 6480, 511912],
}
ENDED = {  # (length, winner) -> finished games, where the whole tree is walked
    2: {(3, 1): 16},                                  # 16 games, all of length 3, all won by Black
    3: {(6, 2): 1152, (7, 1): 45792, (8, 2): 43776},  # 90 720 games of length 6 .. 8: 45 792 Black wins, 44 928 White wins
}


def _engine_legal_moves(mz, n):
    env = mz.Env(_conf(n))

    def legal(actions):
        env.reset()
        for a in actions:
            assert env.act(a)
        m = env.legal_mask()
        assert env.is_terminal() == (m.sum() == 0)
        return [int(a) for a in np.nonzero(m)[0]]
    return legal


@pytest.mark.parametrize("n", sorted(COUNTS))
def test_known_leaf_counts_on_the_model(n):
    counts, ended = R.count_tree(n, len(COUNTS[n]), R.model_legal_moves(n))
    assert counts == COUNTS[n]
    if n in ENDED:
        assert ended == ENDED[n]


@pytest.mark.parametrize("n", sorted(COUNTS))
def test_known_leaf_counts_on_the_engine(mz, n):
    counts, ended = R.count_tree(n, len(COUNTS[n]), _engine_legal_moves(mz, n))
    assert counts == COUNTS[n]
    if n in ENDED:
        assert ended == ENDED[n]


@pytest.mark.parametrize("mover", [1, 2])
@pytest.mark.parametrize("name", sorted(R.HAND))
def test_hand_positions(mz, name, mover):
    """Each position with the mover Black and with the mover White: the engine agrees with the expectation (and the model) on the point in question,
    refuses it without changing anything when it is illegal, and on the whole mask."""
    actions, point, legal = R.hand_sequence(name, mover)
    env, model = mz.Env(_conf()), R.NoGo(9)
    for a in actions:
        assert env.act(a) and model.act(a), (name, mover, a)
    assert env.turn() == mover == model.turn
    assert model.is_legal(point) == legal
    assert np.array_equal(env.legal_mask(), model.legal_mask())
    assert bool(env.legal_mask()[point]) == legal
    assert env.act(point) == legal
    if not legal:
        assert env.turn() == mover and np.array_equal(env.legal_mask(), model.legal_mask())
        assert np.array_equal(env.features(0), model.features(0))


def test_the_pass_action_is_refused(mz):
    for n in (2, 5, 9):
        env = mz.Env(_conf(n))
        assert env.policy_size() == n * n + 1 and env.legal_mask()[n * n] == 0
        assert not env.act(n * n) and env.turn() == 1
        assert env.act(0) and not env.act(n * n) and env.turn() == 2
        assert not env.act(-1) and not env.act(n * n + 1)


def _first_game_won_by(winner, n=3):
    """The first complete game of the model's move tree (actions in ascending order) that `winner` wins."""
    g = R.NoGo(n)

    def walk():
        legal = [a for a in range(n * n) if g.is_legal(a)]
        if not legal:
            return list(g.actions) if 3 - g.turn == winner else None
        for a in legal:
            g.act(a)
            found = walk()
            g.undo()
            if found:
                return found
        return None
    return walk()


@pytest.mark.parametrize("winner", [1, 2])
def test_terminal_with_empty_points_left_and_the_result(mz, winner):
    actions = _first_game_won_by(winner)
    env = mz.Env(_conf(3))
    for i, a in enumerate(actions):
        assert not env.is_terminal(), i
        # (the result is the player not to move, at every position: nogo.h:68-76 does not look at the board)
        assert env.eval_score() == (1.0 if env.turn() == 2 else -1.0) == env.eval_score(resign=True)
        assert env.act(a)
    assert env.is_terminal() and env.legal_mask().sum() == 0
    assert len(actions) < 9  # points are left, and none of them is legal
    assert env.turn() == 3 - winner
    assert env.eval_score() == (1.0 if winner == 1 else -1.0)
    assert env.eval_score(resign=True) == env.eval_score()
    for a in range(10):
        assert not env.act(a)


def test_names_sizes_and_action_strings(mz):
    assert mz.Env("env_game=nogo").name() == "nogo_9x9"  # the default size
    assert mz.Env("env_game=nogo:env_board_size=0").name() == "nogo_9x9"
    assert mz.Env("env_game=nogo").policy_size() == 82  # Go's: the pass slot is in the policy
    assert mz.Env(_conf(5)).name() == "nogo_5x5" and mz.Env(_conf(2)).policy_size() == 5
    assert mz.Env("env_game=nogo").features(0).size == 18 * 81
    with pytest.raises(mz.MzError, match="nogo board size 10 "):
        mz.Env(_conf(10))
    with pytest.raises(mz.MzError, match="nogo board size 1 "):
        mz.Env(_conf(1))
    mz.Env("env_game=nogo:env_go_ko_rule=whatever")  # not read
    env = mz.Env("env_game=nogo")
    assert env.action_from_string("A1") == 0 and env.action_from_string("H1") == 7 and env.action_from_string("J1") == 8  # I is skipped
    assert env.action_from_string("J9") == 80 and env.action_from_string("e5") == 4 * 9 + 4
    assert env.action_from_string("pass") == 81  # Go's action id; never legal
    with pytest.raises(mz.MzError, match="nogo"):  # the list of games in the message
        mz.Env("env_game=nogoo")


def _compare(env, model, where):
    n = model.n
    assert env.turn() == model.turn, where
    assert env.is_terminal() == model.is_terminal(), where
    assert env.eval_score() == model.eval_score(), where
    assert env.eval_score(resign=True) == model.eval_score(), where
    assert np.array_equal(env.legal_mask(), model.legal_mask()), where
    for rot in range(8):
        assert np.array_equal(env.features(rot), model.features(rot)), (where, rot)
        assert np.array_equal(env.feature_bits(rot, 18, n * n), model.feature_bits(rot)), (where, rot)


LENGTHS = {2: (3, 3), 3: (6, 8), 5: (19, 24), 9: (70, 79)}  # moves of a random game, as measured on the model over 2000 / 2000 / 2000 / 300 games


@pytest.mark.parametrize("n,games", [(2, 6), (3, 10), (5, 6), (9, 2)])
def test_random_playouts_against_the_rules_model(mz, n, games):
    rng = np.random.default_rng(n)
    P = n * n
    winners = set()
    for g in range(games):
        env, model = mz.Env(_conf(n)), R.NoGo(n)
        ply = 0
        while True:
            where = f"{n}x{n} game {g} ply {ply} actions {model.actions}"
            _compare(env, model, where)
            if model.is_terminal():
                break
            illegal = [a for a in range(P + 1) if not model.is_legal(a)]
            bad = int(rng.choice(illegal))  # (never empty: the pass slot) refused, and nothing changes
            assert not env.act(bad), where
            assert env.turn() == model.turn and np.array_equal(env.legal_mask(), model.legal_mask()), where
            a = int(rng.choice(np.nonzero(model.legal_mask())[0]))
            assert env.act(a) and model.act(a), where
            ply += 1
        assert LENGTHS[n][0] <= ply <= LENGTHS[n][1], where
        assert 0 in model.board  # a game never reaches P moves: the last empty point is always suicide
        winners.add(3 - model.turn)
    if n == 3:
        assert winners == {1, 2}


def test_go_is_untouched_by_the_variant(mz):
    """Go's row still answers to its own name, and captures there."""
    go = mz.Env("env_game=go:env_board_size=9")
    assert go.name() == "go_9x9" and go.legal_mask()[81] == 1
    for a in (1, 0, 9):  # B[1] W[0] B[9] captures the corner stone
        assert go.act(a)
    assert go.features(0).reshape(18, 81)[0][0] == 0 and go.features(0).reshape(18, 81)[1][0] == 0
