"""Hex's host rules engine (env.cpp Hex; ref environment/hex/hex.{h,cpp}) on the CPU: known answers from the rule text, then random playouts against
the pure-Python restatement of the rules (tests/hex_rules.py) with the swap rule on and off — legal mask, turn, terminal flag, result and the 4
feature planes (float and bit-packed) under all eight rotation arguments, which Hex ignores.  Also: a Go configuration that carries the key plays
unchanged."""
import numpy as np
import pytest

import hex_rules as R


def _conf(n=11, swap=True):
    return f"env_game=hex:env_board_size={n}:env_hex_use_swap_rule={'true' if swap else 'false'}"


def _play(mz, n, swap, moves):
    """moves: (x = column, y = row) in playing order, Black first; every one must be accepted, none may come after the end of the game, and the
    model must agree on the state after each."""
    env, model = mz.Env(_conf(n, swap)), R.Hex(n, swap)
    for i, (x, y) in enumerate(moves):
        assert not env.is_terminal(), f"the game ended before action {i}"
        assert env.act(y * n + x) and model.act(y * n + x), f"action {i} refused"
        assert env.is_terminal() == model.is_terminal() and env.eval_score() == model.eval_score(), f"after action {i}"
    return env


def _interleave(black, white):
    assert len(white) in (len(black), len(black) - 1)
    return [m for pair in zip(black, white) for m in pair] + ([black[-1]] if len(white) < len(black) else [])


def test_a_straight_black_row_wins(mz):
    black = [(x, 2) for x in range(5)]
    white = [(x, 0) for x in range(4)]  # a row of White's touches one of White's edges only
    env = _play(mz, 5, False, _interleave(black[:4], white))
    assert not env.is_terminal() and env.eval_score() == 0.0
    assert env.act(2 * 5 + 4)
    assert env.is_terminal() and env.eval_score() == 1.0 and env.turn() == 2


def test_a_straight_white_column_wins(mz):
    black = [(0, y) for y in range(5)]  # a column of Black's touches one of Black's edges only
    white = [(2, y) for y in range(5)]
    env = _play(mz, 5, False, _interleave(black, white[:4]))
    assert not env.is_terminal() and env.eval_score() == 0.0
    assert env.act(4 * 5 + 2)
    assert env.is_terminal() and env.eval_score() == -1.0 and env.turn() == 1


# a Black chain on 7x7 from column 0 to column 6 whose consecutive stones are joined by every one of the six adjacencies:
# (+1,0) (+1,+1) (0,+1) (+1,0) (0,-1) (0,-1) (-1,-1) (0,-1) (-1,0) (0,-1) (+1,0) ...; its stone (2, 2) is the only link between the two halves
CHAIN_A = [(0, 3), (1, 3), (2, 4), (2, 5), (3, 5), (3, 4), (3, 3)]
CHAIN_LINK = (2, 2)
CHAIN_B = [(2, 1), (1, 1), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0)]
CHAIN_WHITE = [(x, 6) for x in range(7)] + [(5, 3), (6, 3), (5, 4), (6, 4), (5, 5), (6, 5), (4, 5), (4, 4)]  # never on row 0: no White win


def test_the_chain_steps():
    """The chain above really uses each of the six adjacencies, in both halves' walking order."""
    chain = CHAIN_A + [CHAIN_LINK] + CHAIN_B
    steps = {(b[0] - a[0], b[1] - a[1]) for a, b in zip(chain, chain[1:])}
    assert steps == set(R.NEIGHBOURS)


def test_a_chain_over_all_six_adjacencies_wins(mz):
    black = CHAIN_A + CHAIN_B
    env = _play(mz, 7, False, _interleave(black, CHAIN_WHITE))
    assert not env.is_terminal() and env.eval_score() == 0.0 and env.turn() == 1
    assert env.act(CHAIN_LINK[1] * 7 + CHAIN_LINK[0])
    assert env.is_terminal() and env.eval_score() == 1.0


def test_the_other_diagonal_does_not_connect_and_the_full_2x2_board_is_a_win(mz):
    # Black (1, 0) and (0, 1): on both of Black's edges, but (x+1, y-1) is not adjacent — no win, the game goes on
    env = _play(mz, 2, False, [(1, 0), (0, 0), (0, 1)])
    assert not env.is_terminal() and env.eval_score() == 0.0 and env.legal_mask().sum() == 1
    # White's (1, 1) joins (0, 0) over the adjacent diagonal (x-1, y-1): rows 0 and 1 connected on the move that fills the board
    assert env.act(3)
    assert env.is_terminal() and env.eval_score() == -1.0 and env.legal_mask().sum() == 0


def test_a_chain_over_the_other_diagonal_does_not_win(mz):
    env = _play(mz, 3, False, _interleave([(0, 2), (1, 1), (2, 0)], [(0, 0), (2, 2)]))
    assert not env.is_terminal() and env.eval_score() == 0.0
    assert env.act(1 * 3 + 0)  # and the game goes on
    assert not env.is_terminal()


def test_one_edge_touched_twice_does_not_win(mz):
    black = [(0, 0), (1, 0), (1, 1), (1, 2), (0, 2)]  # leaves column 0 and comes back to it
    white = [(4, 0), (4, 1), (4, 2), (4, 3)]
    env = _play(mz, 5, False, _interleave(black, white))
    assert not env.is_terminal() and env.eval_score() == 0.0


def test_black_from_top_to_bottom_does_not_win(mz):
    black = [(1, 0), (1, 1), (1, 2), (1, 3)]  # White's edges, not Black's
    white = [(3, 0), (3, 1), (3, 2)]
    env = _play(mz, 4, False, _interleave(black, white))
    assert not env.is_terminal() and env.eval_score() == 0.0


def test_a_win_on_the_move_that_fills_the_3x3_board(mz):
    # W B B      rows y = 0, 1, 2.  Black's ninth stone (1, 0) joins (0, 1) / (1, 1) — on column 0 — with (2, 0) on column 2; before it Black's (2, 0)
    # B B W      stands alone, and White's (0, 0) | (2, 1), (2, 2) | (0, 2) never hold rows 0 and 2 in one group
    # W B W
    order = [(1, 1), (2, 1), (2, 0), (0, 2), (0, 1), (2, 2), (1, 2), (0, 0)]
    env = _play(mz, 3, False, order)
    assert not env.is_terminal() and env.eval_score() == 0.0 and env.legal_mask().sum() == 1
    assert env.act(0 * 3 + 1)
    assert env.is_terminal() and env.eval_score() == 1.0 and env.legal_mask().sum() == 0


def test_resign_eval(mz):
    env = mz.Env(_conf())
    assert env.eval_score(resign=True) == -1.0  # Black to move resigns: White is scored
    assert env.act(60)
    assert env.eval_score(resign=True) == 1.0 and env.eval_score() == 0.0


def test_swap_mask(mz):
    on, off = mz.Env(_conf(11, True)), mz.Env(_conf(11, False))
    assert on.legal_mask().sum() == off.legal_mask().sum() == 121
    assert on.act(37) and off.act(37)
    assert on.legal_mask().sum() == 121 and off.legal_mask().sum() == 120 and not off.legal_mask()[37]
    assert on.act(5) and off.act(5)  # a second action elsewhere is an ordinary move
    assert on.legal_mask().sum() == off.legal_mask().sum() == 119


def test_swap_moves_the_stone_to_its_reflection(mz):
    n, r, c = 11, 3, 2  # (not on the anti-diagonal r + c = n - 1, whose cells are their own reflections)
    env = mz.Env(_conf(n, True))
    assert env.act(r * n + c) and env.turn() == 2
    assert env.act(r * n + c)  # White takes the stone over
    assert env.turn() == 1 and not env.is_terminal()
    f = env.features(0).reshape(4, n * n)
    assert f[0].sum() == 0  # Black (to move) has no stone
    assert f[1].sum() == 1 and f[1][(n - 1 - c) * n + (n - 1 - r)] == 1  # White's is at (row n-1-c, col n-1-r)
    assert f[2].all() and not f[3].any()
    m = env.legal_mask()
    assert m.sum() == n * n - 1 and m[r * n + c] and not m[(n - 1 - c) * n + (n - 1 - r)]
    assert env.act(r * n + c)  # the vacated cell is playable again


def test_the_reflected_stone_counts_for_the_edges(mz):
    # 2x2: Black takes the corner (row 0, col 0); swapped, White's stone is on (row 1, col 1), on White's far edge.  White's next stone (col 1, row 0) is
    # adjacent to (col 1, row 1) — White's column is complete
    env = mz.Env(_conf(2, True))
    assert env.act(0) and env.act(0)
    assert env.turn() == 1 and not env.is_terminal()
    assert env.act(2)  # Black (col 0, row 1)
    assert not env.is_terminal()
    assert env.act(1)  # White (col 1, row 0)
    assert env.is_terminal() and env.eval_score() == -1.0


def test_occupied_cells_are_refused(mz):
    off = mz.Env(_conf(5, False))
    assert off.act(7) and not off.act(7) and off.turn() == 2 and off.legal_mask().sum() == 24  # rule off: refused, nothing changes
    on = mz.Env(_conf(5, True))
    assert on.act(7) and on.act(8)
    assert not on.act(7) and not on.act(8) and on.turn() == 1  # a third action on an occupied cell
    on = mz.Env(_conf(5, True))
    assert on.act(7) and on.act(7)
    assert not on.act(5 * (4 - 2) + (4 - 1)) and on.turn() == 1  # ... also on the reflected stone (row 1, col 2) -> (row 2, col 3)


def test_names_sizes_and_action_strings(mz):
    assert mz.Env("env_game=hex").name() == "hex_11x11"  # the default size
    assert mz.Env("env_game=hex").policy_size() == 121   # no pass action
    assert mz.Env("env_game=hex:env_board_size=19").name() == "hex_19x19"
    assert mz.Env("env_game=hex:env_board_size=19:env_hex_use_swap_rule=false").name() == "hex_19x19"  # no rule suffix
    assert mz.Env("env_game=hex:env_board_size=2").policy_size() == 4
    with pytest.raises(mz.MzError, match="hex board size 1 "):
        mz.Env("env_game=hex:env_board_size=1")
    with pytest.raises(mz.MzError, match="hex board size 20 "):
        mz.Env("env_game=hex:env_board_size=20")
    with pytest.raises(mz.MzError):
        mz.Env("env_game=hex:env_hex_use_swap_rule=maybe")
    env = mz.Env("env_game=hex")
    assert env.action_from_string("A1") == 0 and env.action_from_string("H1") == 7 and env.action_from_string("J1") == 8  # I is skipped
    assert env.action_from_string("L11") == 120 and env.action_from_string("f6") == 5 * 11 + 5
    assert env.action_from_string("pass") == -1 and env.action_from_string("PASS") == -1


def _compare(env, model, where):
    n = model.n
    assert env.turn() == model.turn, where
    assert env.is_terminal() == model.is_terminal(), where
    assert env.eval_score() == model.eval_score(), where
    assert env.eval_score(resign=True) == model.eval_score(resign=True), where
    assert np.array_equal(env.legal_mask(), model.legal_mask()), where
    f, b = model.features(), model.feature_bits()
    for rot in range(8):  # all eight equal to each other: the rotation argument is ignored
        assert np.array_equal(env.features(rot), f), (where, rot)
        assert np.array_equal(env.feature_bits(rot, 4, n * n), b), (where, rot)


@pytest.mark.parametrize("n,games", [(2, 12), (3, 12), (5, 60), (11, 6), (19, 4)])
@pytest.mark.parametrize("swap", [True, False])
def test_random_playouts_against_the_rules_model(mz, n, games, swap):
    rng = np.random.default_rng(100 * n + int(swap))
    P = n * n
    winners, full, longest = set(), 0, 0
    for g in range(games):
        env, model = mz.Env(_conf(n, swap)), R.Hex(n, swap)
        take_swap = swap and g % 3 == 0
        ply = 0
        while True:
            where = f"{n}x{n} swap={swap} game {g} ply {ply} actions {model.actions}"
            _compare(env, model, where)
            if model.is_terminal():
                break
            illegal = [a for a in range(P) if not model.is_legal(a)]
            if illegal:  # refused, and nothing changes
                bad = int(rng.choice(illegal))
                assert not env.act(bad), where
                assert env.turn() == model.turn and np.array_equal(env.legal_mask(), model.legal_mask()), where
            legal = np.nonzero(model.legal_mask())[0]
            if ply == 1 and swap:
                a = model.actions[0] if take_swap else int(rng.choice([x for x in legal if x != model.actions[0]]))
            else:
                a = int(rng.choice(legal))
            assert env.act(a) and model.act(a), where
            ply += 1
        assert model.winner in (1, 2), where  # no game ends without a winner
        assert model.swapped == take_swap
        winners.add(model.winner)
        full += 0 not in model.board
        longest = max(longest, len(model.actions))
    assert winners == {1, 2}
    if n <= 5:
        assert full > 0  # some game ends on the move that fills the board
    if n == 5 and swap:
        assert longest == P + 1  # a swap and then the whole board: one action more than there are cells


def test_go_configuration_ignores_the_hex_key(mz):
    """The key is inert for every other game: the same Go game with and without it."""
    rng = np.random.default_rng(5)
    plain = mz.Env("env_game=go:env_board_size=9")
    keyed = mz.Env("env_game=go:env_board_size=9:env_hex_use_swap_rule=false")
    assert plain.policy_size() == keyed.policy_size() == 82
    for ply in range(60):
        m = plain.legal_mask()
        assert np.array_equal(m, keyed.legal_mask()) and np.array_equal(plain.features(ply % 8), keyed.features(ply % 8))
        if plain.is_terminal():
            break
        a = int(rng.choice(np.nonzero(m)[0]))
        assert plain.act(a) and keyed.act(a)
    assert plain.eval_score() == keyed.eval_score()
