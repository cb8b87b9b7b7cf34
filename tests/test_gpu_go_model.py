"""The device-resident rules engines of Go and Othello (go_body.h, go_dev.hip) held DIRECTLY to the rules models of tests/go_rules.py and
tests/othello_rules.py — no product code and no oracle on the reference side.  The games are the capture-seeking playouts of tests/rules_playouts.py (the
table tests/test_go_model.py holds the two CPU engines to) and the hand-built sequences of tests/hand_go.py, with the deciding moves made on the device; the
records of finished self-play games are replayed on the models.  Everything is compared exactly.

What the device engine defines, and what is compared: the planes under the rotation asked for, the player to move and the terminal flag at every position;
the legal mask at every position that is not terminal and the result at every terminal one.  The leaf bodies compute no mask at a terminal leaf (it has no
children) and no score at any other (go_body.h: `!terminal` in legalMask, `if (terminal)` around the area count): the search reads neither, so the device
does not define them and they are not compared here.  Results at positions that are not terminal and masks at terminal ones are held to the model on the
host engine and the oracle, after every action of the same games (tests/test_go_model.py, tests/test_othello_model.py)."""
import re

import numpy as np
import pytest

from go_rules import Go, replay_record as replay_go
from othello_rules import Othello, replay_record as replay_othello
import rules_playouts as R

pytestmark = pytest.mark.gpu

_EXPECT = {}


def expected(key, make_model, actions):
    """the model's side of a game, computed once: per position (turn, terminal, result, legal mask) and the model after each action (for the planes)"""
    if key not in _EXPECT:
        g = make_model()
        rows = [(g.turn, g.is_terminal(), g.eval_score(), g.legal_mask(), g.clone())]
        for a in actions:
            assert g.act(a)
            rows.append((g.turn, g.is_terminal(), g.eval_score(), g.legal_mask(), g.clone()))
        _EXPECT[key] = rows
    return _EXPECT[key]


def device_against_model(mz, key, make_model, game, n, komi, channels, actions, root_prefix, seed):
    rows = expected(key, make_model, actions)
    steps = len(actions) - root_prefix + 1
    rots = np.random.default_rng(seed).integers(0, 8, steps).astype(np.int32)
    feat, legal, term, ev, pl = mz.envdev_playout(game, n, komi, actions, root_prefix, rots, channels, n * n + 1)
    for d in range(steps):
        turn, terminal, result, mask, model = rows[root_prefix + d]
        where = f"{key} step {d} (root at {root_prefix}) after {actions[:root_prefix + d]}"
        assert pl[d] == turn, where
        assert bool(term[d]) == terminal, where
        if terminal:
            assert ev[d] == result, f"result {ev[d]} != model {result}, {where}"
        else:
            assert np.array_equal(legal[d], mask), f"legal mask differs at {np.flatnonzero(legal[d] != mask)}, {where}"
        assert np.array_equal(feat[d], model.feature_bits(int(rots[d]))), f"planes under rotation {rots[d]}, {where}"
    return steps


def go_game_on_device(mz, name, index, roots):
    n, rule, komi, _, _, _ = R.GO_ROWS[name]
    seed, actions, _ = R.go_games(name)[index]
    for root in roots:
        device_against_model(mz, (name, seed), lambda: Go(n, komi, rule), "go" if rule == "positional" else "go_situational", n, komi, 18, actions,
                             root if root >= 0 else len(actions) + root, seed + 7 * (root + 2))
    return len(actions)


# (row of the playout table, games of it).  Per game the root stands at depth 0, at a third of the game and at its last move.
GO_DEVICE_ROWS = [("go3_pos_komi9", 8), ("go3_sit", 8), ("go5_pos", 6), ("go5_sit", 6), ("go5_pos_nopass", 2), ("go8_pos", 3), ("go8_sit", 2), ("go9_pos", 3),
                  ("go9_sit", 2), ("go9_pos_nopass", 1), ("go11_pos", 1), ("go11_sit", 1), ("go13_pos", 1), ("go13_sit", 1), ("go16_pos", 1), ("go16_sit", 1)]


@pytest.mark.parametrize("name,games", GO_DEVICE_ROWS, ids=[r[0] for r in GO_DEVICE_ROWS])
def test_go_device_engine_plays_the_models_games(mz, name, games):
    """board 8: the pass bit opens a new mask word; board 16: P = 256 is exactly four 64-bit words"""
    for i in range(games):
        seed, actions, _ = R.go_games(name)[i]
        go_game_on_device(mz, name, i, (0, len(actions) // 3, -1))


def test_go_device_engine_19x19_to_the_move_cap(mz):
    """the 723-action game without a pass: at its end the superko set holds 723 positions of the table's 1024 slots (go_dev.h, kGoSeenCap).  Root at depth 0,
    every position from the device, and at depth 700, the set filled by the host's export"""
    assert go_game_on_device(mz, "go19_pos_nopass", 0, (0, 700)) == 723


def test_go_device_engine_19x19_situational(mz):
    seed, actions, _ = R.go_games("go19_sit")[0]
    go_game_on_device(mz, "go19_sit", 0, (len(actions) // 3, -1))


def test_go_device_engine_on_hand_built_sequences(mz):
    """a chain through all six words of 19x19 captured whole, one stone capturing four blocks, a snapback, a superko cycle of eight plies, the position where
    the ko rules differ: the model has confirmed each (test_go_model.hand_cases), the deciding moves are made on the device"""
    from test_go_model import hand_cases
    for name, n, rule, actions, tail in hand_cases():
        for root in (0, len(actions) - tail):
            device_against_model(mz, ("hand", name), lambda: Go(n, 0.5, rule), "go" if rule == "positional" else "go_situational", n, 0.5, 18, actions, root, 3 + root)


@pytest.mark.parametrize("name", list(R.OTHELLO_ROWS))
def test_othello_device_engine_plays_the_models_games(mz, name):
    n = R.OTHELLO_ROWS[name][0]
    for seed, actions, _ in R.othello_games(name)[:12]:
        for root in (0, len(actions) // 3, len(actions) - 1):
            device_against_model(mz, (name, seed), lambda: Othello(n), "othello", n, 0.0, 4, actions, root, seed + root)


# ---- finished self-play records, replayed on the models --------------------------------------------------------------------------------------------
# the three ways a worker evaluates leaves: the simulation kernel, lock-step with the rules on the device, lock-step with the rules on the host
PATHS = {"simulation kernel": "", "lock-step, device rules": ":mz_sim_kernel=false", "lock-step, host rules": ":mz_sim_kernel=false:mz_device_env=false"}
SIMS, GAMES = 4, 4


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("game", ["go", "othello"])
def test_finished_records_replay_on_the_model(mz, game, path):
    """a default pool — Dirichlet noise, random rotation, softmax selection — plays games to their end; every record is replayed on the model: every move legal and
    in turn, the game ends where the model ends it, RE is the model's result"""
    n, planes, longest = (9, 18, 2 * 81 + 1) if game == "go" else (8, 4, 64 + 16)
    d = mz.make_desc(f"{game}_{n}x{n}", planes, n, n, 8, n, n, 1, 1, n * n + 1, vh=16, dv=1, type_name="alphazero")
    conf = (f"env_game={game}:env_board_size={n}:actor_num_simulation={SIMS}:zero_num_parallel_games={GAMES}:program_seed=11:nn_file_name=x.pt:zero_num_threads=2"
            f":actor_resign_threshold=-2{PATHS[path]}")
    wk = mz.Worker(conf, d, mz.generate_weights(d, 3))
    wk.command("start")
    cycles = (SIMS + 1) * (longest + 1)
    assert wk.run_cycles(cycles) == cycles
    st, lines = wk.stats(), wk.pop_lines()[:GAMES]
    wk.close()
    assert (st["sim_launches"] > 0) == (path == "simulation kernel"), st
    assert (st["ms_env"] > 0) == (path == "lock-step, host rules"), st
    assert len(lines) == GAMES
    lengths = set()
    for line in lines:
        assert line.startswith("SelfPlay ")
        record = line.split(" ", 5)[5][:-2]
        if game == "go":
            assert re.search(r"KM\[([^\]]*)\]", record).group(1) == "7.500000" and f"SZ[{n}]" in record
            g, re_value, gm = replay_go(record, n, 7.5, "positional")
        else:
            g, re_value, gm = replay_othello(record, n)
        assert gm == f"{game}_{n}x{n}"
        assert g.is_terminal(), "the record ends before the game does"
        assert re_value == g.eval_score(), f"RE[{re_value}] but the model scores {g.eval_score()}"
        lengths.add(len(g.actions))
    assert len(lengths) > 1, "a default pool plays different games"
