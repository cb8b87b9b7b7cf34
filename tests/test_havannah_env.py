"""Havannah's host rules engine (env.cpp Havannah; ref environment/havannah/havannah.{h,cpp}) on the CPU against the pure-Python restatement of the rules
(tests/havannah_rules.py: there is no oracle for this game): positions by hand with either colour as the mover, random whole games — legal mask, turn,
terminal flag, result and the 20 feature planes after every action — the two forms of the ring's hole test against each other on every position, names,
sizes and coordinates, the refusals (board sizes, a MuZero network), and the facts of game_kind.h for the games that were there before.  (The loader's refusals
are in test_gpu_havannah.py: a loader needs a device.)"""
import numpy as np
import pytest

import havannah_rules as R


def _conf(N=8, swap=True):
    return f"env_game=havannah:env_board_size={N}:env_havannah_use_swap_rule={'true' if swap else 'false'}"


def _compare(env, model, where):
    E = model.E
    assert env.turn() == model.turn, where
    assert env.is_terminal() == model.is_terminal(), where
    assert env.eval_score() == model.eval_score(), where
    assert env.eval_score(resign=True) == model.eval_score(resign=True), where
    assert np.array_equal(env.legal_mask(), model.legal_mask()), where
    f = model.features()
    for rot in (0, 3, 6):  # no symmetries: every rotation argument gives the same planes
        assert np.array_equal(env.features(rot), f), (where, rot)
    assert np.array_equal(env.feature_bits(5, 20, E * E), model.feature_bits()), where
    if model.actions:  # the reference's hole test and the whole-array form, on the group of the last stone whatever the gates said
        assert model.hole_bbox(model.last["group"]) == model.hole_rim(model.last["group"]), where


@pytest.mark.parametrize("mover", [1, 2])
@pytest.mark.parametrize("name", sorted(R.HAND))
def test_hand_positions(mz, name, mover):
    """Each position with Black and with White placing the deciding stone: the model finds what the position was built for, by the path it was built for
    (shortcut or complement flood), and the engine agrees with the model after every action."""
    h = R.HAND[name]
    N, seq = R.hand_sequence(name, mover)
    env, model = mz.Env(_conf(N)), R.Havannah(N)
    for i, a in enumerate(seq):
        assert env.act(a) and model.act(a), (name, mover, i)
        _compare(env, model, (name, mover, i))
        if i + 1 < len(seq) and h["winner"] != "b":
            assert model.winner == 0, (name, mover, i)
    assert model.turn == 3 - mover
    assert model.last["kind"] == h["expect"]
    assert model.last["flooded"] == h.get("flooded", False) and model.last["shortcut"] == h.get("shortcut", False)
    if h.get("no_hole"):
        assert not model.hole_bbox(model.last["group"]) and not model.hole_rim(model.last["group"])  # the shortcut alone wins
    if "closing_neighbours" in h:
        assert model.own_neighbours(model.cell(seq[-1]), mover) == h["closing_neighbours"]
    winner = {"a": mover, "b": 3 - mover, None: 0}[h["winner"]]
    assert model.winner == winner
    assert env.is_terminal() == (winner != 0) and env.eval_score() == {0: 0.0, 1: 1.0, 2: -1.0}[winner]
    ids = [model.ident(c) for c in model.last["group"]]
    if "two_words" in name:
        assert min(ids) < 64 <= max(ids)


def test_the_swap_of_a_corner_cell(mz):
    """After B[k];W[k] the cell is White's — White's bridge runs through it — and stays in BOTH feature bitboards, as the reference keeps them."""
    h = R.SWAP_CORNER
    N = h["N"]
    env, model = mz.Env(_conf(N)), R.Havannah(N)
    corner = model.ident(h["actions"][0])
    P = model.P
    for i, c in enumerate(h["actions"]):
        a = model.ident(c)
        if i == 1:
            assert env.legal_mask().sum() == len(model.valid) and env.legal_mask()[corner] == 1  # every cell of the board, the occupied one too
            assert env.features(0).reshape(20, P)[17].min() == 1.0                               # swappable: all ones, off-board cells too
        assert env.act(a) and model.act(a)
        _compare(env, model, i)
        if i >= 1:
            f = env.features(0).reshape(20, P)
            assert f[0][corner] == 1.0 and f[1][corner] == 1.0 and f[17].max() == 0.0
            assert model.owner[h["actions"][0]] == 2 and env.legal_mask()[corner] == 0
    assert model.last["kind"] == h["expect"] and model.winner == h["winner"]
    assert env.is_terminal() and env.eval_score() == -1.0
    # with the rule off the occupied cell is refused on the second action
    env = mz.Env(_conf(N, False))
    assert env.act(corner) and not env.act(corner) and env.turn() == 2 and env.legal_mask().sum() == len(model.valid) - 1
    assert env.features(0).reshape(20, P)[17].max() == 0.0


def test_the_full_board_is_a_draw(mz):
    env, model = mz.Env(_conf(4)), R.Havannah(4)
    assert len(R.DRAW_N4) == 37 == len(model.valid)
    for i, a in enumerate(R.DRAW_N4):
        assert not env.is_terminal() and not model.is_terminal()
        assert env.act(a) and model.act(a)
        _compare(env, model, i)
    assert model.winner == 0 and model.is_terminal() and env.is_terminal() and env.eval_score() == 0.0 and env.legal_mask().sum() == 0
    assert env.turn() == 2 and env.eval_score(resign=True) == 1.0  # Black placed the 37th stone; White to move resigns: the player not to move wins


# seeds of havannah_rules.random_game (swap rule on; the second action takes the swap when seed % 3 == 0, avoids it when seed % 3 == 1) whose games the
# model ends by each kind of win for each colour — and, at N = 4, by filling the board
SEEDS = {4: [0, 1, 2, 3, 14, 113, 118], 5: [0, 1, 2, 5, 7, 15], 8: [0, 1]}
KINDS = {(k, c) for k in ("bridge", "fork", "ring") for c in (1, 2)}


@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("N", sorted(SEEDS))
def test_random_games_against_the_rules_model(mz, N, swap):
    decided = set()
    for seed in SEEDS[N]:
        game = R.random_game(N, swap, seed, [True, False, None][seed % 3])
        decided.add(game.kinds[0] if game.kinds else "draw")
        env, model = mz.Env(_conf(N, swap)), R.Havannah(N, swap)
        rng = np.random.default_rng(seed)
        for i, a in enumerate(game.actions):
            where = f"N {N} swap {swap} seed {seed} action {i} of {game.actions}"
            _compare(env, model, where)
            illegal = [x for x in range(model.P) if not model.is_legal(x)]
            bad = int(rng.choice(illegal))  # (never empty: the cells off the board) refused, and nothing changes
            assert not env.act(bad) and env.turn() == model.turn and np.array_equal(env.legal_mask(), model.legal_mask()), where
            assert env.act(a) and model.act(a), where
        _compare(env, model, f"N {N} swap {swap} seed {seed} end")
        assert env.is_terminal() and env.eval_score() == game.eval_score()
    if swap and N in (4, 5):  # the seeds were picked on the model alone for this: the test cannot pass on bridges only
        assert KINDS <= decided, decided
    if swap and N == 4:
        assert "draw" in decided


def test_names_sizes_coordinates_and_refusals(mz):
    env = mz.Env("env_game=havannah")
    assert env.name() == "havannah8x8" and env.policy_size() == 225 and env.features(0).size == 20 * 225  # the default edge size: a 15x15 network
    assert mz.Env(_conf(4)).name() == "havannah4x4" and mz.Env(_conf(4)).policy_size() == 49
    assert mz.Env(_conf(10)).policy_size() == 361
    for N in (4, 5, 8, 10):
        m = R.Havannah(N)
        assert mz.Env(_conf(N)).legal_mask().sum() == len(m.valid) == 3 * N * (N - 1) + 1
    with pytest.raises(mz.MzError, match="havannah board size 3 .*at least 4"):
        mz.Env(_conf(3))
    with pytest.raises(mz.MzError, match="havannah board size 11 .*up to 10"):
        mz.Env(_conf(11))
    with pytest.raises(mz.MzError, match="havannah"):  # the list of games in the message
        mz.Env("env_game=havanna")
    # console coordinates are those of the E x E array, the column letters skip I; off-board cells and the pass are no actions
    m = R.Havannah(8)
    assert env.action_from_string("H1") == 7 and env.action_from_string("J1") == 8 and env.action_from_string("h15") == 14 * 15 + 7
    for a in (7, 8, 14, 7 * 15, 7 * 15 + 7, 14 * 15, 14 * 15 + 7):
        assert m.cell(a) in m.valid and env.action_from_string(m.console(a)) == a, m.console(a)
    assert m.console(8) == "J1" and m.console(14 * 15 + 7) == "H15"
    assert env.action_from_string("A1") == -1 and env.action_from_string("P15") == -1  # the two corners of the array that are cut off
    assert env.action_from_string("pass") == -1
    assert not env.act(0) and not env.act(224) and not env.act(225) and not env.act(-1) and env.turn() == 1


def _desc(mz, N, c=32, type_name="alphazero"):
    E = 2 * N - 1
    return mz.make_desc(f"havannah{N}x{N}", 20, E, E, c, E, E, 1, 1, E * E, vh=32, dv=1, type_name=type_name)


def test_the_descriptor_and_configuration_of_the_default_game(mz):
    d = mz.DESCS["havannah8x64"]()
    assert (d.num_input_channels, d.input_channel_height, d.input_channel_width, d.num_hidden_channels, d.num_blocks, d.action_size) == (20, 15, 15, 64, 6, 225)
    assert "env_game=havannah" in mz.CONFIGS["havannah8x64"] and "env_board_size=8" in mz.CONFIGS["havannah8x64"]


def test_a_muzero_network_is_refused_by_name(mz):
    """getActionFeatures throws in the reference: AlphaZero and Gumbel AlphaZero only.  (Refused before anything touches a device.)"""
    for type_name in ("muzero",):
        d = _desc(mz, 4, type_name=type_name)
        with pytest.raises(mz.MzError, match="havannah has no action features"):
            mz.Worker(f"{_conf(4)}:nn_type_name={type_name}:actor_num_simulation=4:zero_num_parallel_games=2:nn_file_name=x.pt", d, np.zeros(mz.param_count(d), np.float32))


def test_the_facts_of_the_other_games_are_unchanged(mz):
    """game_kind.h through the engines: name, planes, policy size (the pass slot), default and extreme boards of the six games that were there before."""
    facts = {  # env_game: (default name, planes, default board, policy size, a board that is refused)
        "go": ("go_9x9", 18, 9, 82, 20), "othello": ("othello_8x8", 4, 8, 65, 10), "tictactoe": ("tictactoe", 4, 3, 9, None),
        "gomoku": ("gomoku_15x15", 4, 15, 225, 20), "hex": ("hex_11x11", 4, 11, 121, 20), "nogo": ("nogo_9x9", 18, 9, 82, 10),
    }
    for game, (name, planes, n, policy, refused) in facts.items():
        env = mz.Env(f"env_game={game}")
        assert env.name() == name and env.policy_size() == policy and env.features(0).size == planes * n * n, game
        if refused:
            with pytest.raises(mz.MzError, match="not supported"):
                mz.Env(f"env_game={game}:env_board_size={refused}")
    assert mz.Env("env_game=go:env_board_size=19").policy_size() == 362 and mz.Env("env_game=hex:env_board_size=2").policy_size() == 4
    assert mz.Env("env_game=nogo:env_board_size=2").policy_size() == 5 and mz.Env("env_game=othello:env_board_size=4").policy_size() == 17
