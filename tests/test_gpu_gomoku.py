"""Gomoku on the GPU: the device rules engine (go_body.h gmkLeafBody, GoDevView::kind 3) against the host engine, the worker's three execution paths
(per-game simulation kernel sim_kernel_wide<15,15,16,C,-2>, lock-step with the device rules, lock-step with the host rules) against each other, every
finished record against the pure-Python rules model (tests/gomoku_rules.py: there is no oracle for this game), the learner-side sampler's device replay
and the `-mode sp` executable.  ref environment/gomoku/gomoku.{h,cpp}."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import gomoku_rules as R
from game_paths import GUMBEL, run_paths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [("standard", True), ("standard", False), ("outer_open", True), ("outer_open", False)]


def _conf(n=15, rule="standard", five=True):
    return f"env_game=gomoku:env_board_size={n}:env_gomoku_rule={rule}:env_gomoku_exactly_five_stones={'true' if five else 'false'}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the device engine against the host engine
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _device_vs_host(mz, conf, n, actions, root_prefix, rng):
    steps = len(actions) - root_prefix + 1
    rots = rng.integers(0, 8, steps).astype(np.int32)
    feat, legal, term, ev, pl = mz.envdev_playout_conf(conf, n, actions, root_prefix, rots, 4, n * n)
    ref = mz.Env(conf)
    for a in actions[:root_prefix]:
        assert ref.act(a)
    for d in range(steps):
        where = f"{conf} step {d} (root_prefix {root_prefix}) actions {actions[:root_prefix + d]}"
        assert pl[d] == ref.turn(), where
        assert bool(term[d]) == ref.is_terminal(), where
        assert ev[d] == ref.eval_score(), where
        assert np.array_equal(legal[d], ref.legal_mask()), where
        assert np.array_equal(feat[d], ref.feature_bits(int(rots[d]), 4, n * n)), where
        if d + 1 < steps:
            assert ref.act(actions[root_prefix + d]), where
    return ref


def _random_game(mz, conf, rng):
    env, actions = mz.Env(conf), []
    while not env.is_terminal():
        a = int(rng.choice(np.nonzero(env.legal_mask())[0]))
        assert env.act(a)
        actions.append(a)
    return actions, env.eval_score()


@pytest.mark.parametrize("n,rule,five,games", [(15, r, f, 6) for r, f in RULES] + [(19, "standard", True, 3), (19, "outer_open", False, 2),
                                                                                (5, "standard", True, 10), (5, "outer_open", False, 10),
                                                                                (8, "standard", True, 3), (9, "outer_open", False, 3)])
def test_device_engine_matches_host_engine(mz, n, rule, five, games):
    """Random whole games; the device replays the tail move by move from roots at several depths (root_prefix 0 .. the last move, so that the winning
    or board-filling stone is a device move): planes under random rotations, legal mask, terminal flag, result and player to move after every move.
    The boards cover the boundaries of the planes' words: 8x8 is one full 64-bit word, 9x9 two words of which the second has one 32-bit half only (5x5:
    the same in the first word), 15x15 four words, 19x19 the most a bitboard holds."""
    rng = np.random.default_rng(100 * n + 10 * RULES.index((rule, five)))
    conf = _conf(n, rule, five)
    outcomes = set()
    for g in range(games):
        actions, result = _random_game(mz, conf, rng)
        outcomes.add(result)
        root_prefix = [0, len(actions) // 3, len(actions) - 1][g % 3]
        _device_vs_host(mz, conf, n, actions, root_prefix, rng)
    if n == 5:
        assert 0.0 in outcomes  # full boards without a five are reachable on 5x5
    else:
        assert outcomes & {1.0, -1.0}


def _p(x, y, n=15):
    return y * n + x


def _alternate(black, white, n=15):
    return [_p(*m, n) for pair in zip(black, white) for m in pair] + ([_p(*black[-1], n)] if len(white) < len(black) else [])


FILLER = [(0, 14), (2, 14), (4, 14), (6, 14), (8, 14), (10, 14), (12, 14), (14, 12), (14, 10)]
HAND = [  # (conf, moves, expected terminal, expected eval after the last move — the device's move)
    (_conf(), _alternate([(3, 7), (4, 7), (6, 7), (7, 7), (5, 7)], FILLER[:4]), True, 1.0),
    (_conf(), _alternate([(1, 0), (2, 0), (3, 0), (4, 0), (0, 0)], FILLER[:4]), True, 1.0),
    (_conf(), _alternate([(14, 5), (14, 6), (14, 7), (14, 8), (14, 4)], FILLER[:4]), True, 1.0),
    (_conf(), _alternate([(1, 1), (2, 2), (4, 4), (5, 5), (3, 3)], FILLER[:4]), True, 1.0),
    (_conf(), _alternate([(5, 1), (4, 2), (2, 4), (1, 5), (3, 3)], FILLER[:4]), True, 1.0),
    (_conf(), _alternate([(10, 0), (12, 0), (10, 2), (12, 2), (10, 4)], [(3, 3), (3, 4), (3, 5), (3, 6), (3, 7)]), True, -1.0),
    (_conf(), _alternate([(1, 1), (2, 2), (4, 4), (5, 5)], FILLER[:4]), False, 0.0),                                       # four: no win
    (_conf(five=True), _alternate([(2, 7), (3, 7), (4, 7), (6, 7), (7, 7), (5, 7)], FILLER[:5]), False, 0.0),             # overline
    (_conf(five=False), _alternate([(2, 7), (3, 7), (4, 7), (6, 7), (7, 7), (5, 7)], FILLER[:5]), True, 1.0),             # freestyle
    (_conf(five=True), _alternate([(2, 7), (3, 7), (4, 7), (6, 7), (7, 7), (5, 3), (5, 4), (5, 5), (5, 6), (5, 7)], FILLER[:9]), True, 1.0),  # six + five
]


def _full_board_win():
    rows = ["_BBBB", "BBWWW", "WWBBW", "BWWWB", "WBWBW"]
    black = [(x, y) for y in range(5) for x in range(5) if rows[y][x] == "B"] + [(0, 0)]
    white = [(x, y) for y in range(5) for x in range(5) if rows[y][x] == "W"]
    return _alternate(black, white, 5)


def test_hand_positions_with_the_winning_stone_on_the_device(mz):
    rng = np.random.default_rng(3)
    for conf, moves, terminal, result in HAND + [(_conf(5), _full_board_win(), True, 1.0), (_conf(4), list(range(16)), True, 0.0)]:
        n = int(conf.split("env_board_size=")[1].split(":")[0])
        for root_prefix in (len(moves) - 1, 0):
            ref = _device_vs_host(mz, conf, n, moves, root_prefix, rng)
            assert ref.is_terminal() == terminal and ref.eval_score() == result, conf
    # outer-open: the first move's mask on the device is the 104 ring points; the second move's is every empty point
    feat, legal, term, ev, pl = mz.envdev_playout_conf(_conf(rule="outer_open"), 15, [0, 112], 0, [0, 0, 0], 4, 225)
    assert legal[0].sum() == 104 and not legal[0][112] and legal[1].sum() == 224 and legal[1][112] and legal[2].sum() == 223


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the worker: records equal across the three execution paths, every finished record legal
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _desc(mz, n, c, blocks, type_name="alphazero"):
    return mz.make_desc(f"gomoku_{n}x{n}", 4, n, n, c, n, n, 1, blocks, n * n, vh=32, dv=1, type_name=type_name)


def _check_records(lines, n, rule, five):
    name = f"gomoku_{'oo_' if rule == 'outer_open' else ''}{n}x{n}"
    for line in lines:
        assert line.startswith("SelfPlay ")
        record = line.split(" ", 5)[5][:-2]
        model, re_value, gm = R.replay_record(record, n, rule == "outer_open", five)
        assert gm == name
        if rule == "outer_open":
            i, j = divmod(model.actions[0], n)
            assert i < 2 or i >= n - 2 or j < 2 or j >= n - 2
        # a finished game ends at its first winning move or on the full board; an unfinished one was resigned: the player to move lost
        assert re_value == (model.eval_score() if model.is_terminal() else model.eval_score(resign=True)), record[:200]


CASES = [  # (c, blocks, extra configuration, rule, five, seed)
    (32, 2, "", "standard", True, 1),
    (64, 1, "", "standard", True, 2),
    (32, 1, GUMBEL, "standard", True, 3),
    (32, 1, "", "outer_open", True, 4),
    (32, 1, "", "standard", False, 5),
]


@pytest.mark.parametrize("c,blocks,extra,rule,five,seed", CASES)
def test_records_equal_across_the_three_paths(mz, c, blocks, extra, rule, five, seed):
    """15x15, n = 16, 8 games until every game has finished at least once: the simulation kernel, lock-step with device rules and lock-step with host
    rules write byte-identical lines and records; every finished record replays legally on the rules model with the right result."""
    n, sims, games = 15, 16, 8
    d = _desc(mz, n, c, blocks)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(n, rule, five)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2{extra}"
    cycles = (sims + 1) * 230  # longer than any game on 225 points
    lines, recs = run_paths(mz, conf, d, w, games, cycles)
    assert len(lines) >= games
    _check_records(lines, n, rule, five)


def test_default_network_takes_the_lock_step_path_with_device_rules(mz):
    """The reference's default network (1 block x 256 channels) cannot hold a 15x15 tile in LDS: the plan takes the lock-step cycle with the device
    rules resident (no simulation-kernel launch, no host environment time); its records after the first move equal the host-rules path's."""
    n, sims, games = 15, 12, 4
    d = _desc(mz, n, 256, 1)
    w = mz.generate_weights(d, 7)
    conf = f"{_conf()}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=7:nn_file_name=x.pt:zero_num_threads=2"
    _, recs = run_paths(mz, conf, d, w, games, 2 * (sims + 1), paths=("sim", "lockstep_host"), expect_sim=False)
    assert all(";B[" in r for r in recs)


def test_muzero_on_gomoku(mz):
    """MuZero (the host engine at the root only): finished records replay legally; the two MuZero paths agree."""
    n, sims, games = 9, 8, 6
    d = _desc(mz, n, 32, 1, "muzero")
    w = mz.generate_weights(d, 11)
    conf = f"{_conf(n)}:nn_type_name=muzero:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=11:nn_file_name=x.pt:zero_num_threads=2"
    out = []
    for extra in ("", ":mz_sim_kernel=false"):
        wk = mz.Worker(conf + extra, d, w)
        wk.command("start")
        assert wk.run_cycles((sims + 1) * 90) == (sims + 1) * 90
        out.append((wk.pop_lines(), wk.peek_records(games)))
        wk.close()
    assert out[0] == out[1]
    assert len(out[0][0]) >= games
    _check_records(out[0][0], n, "standard", True)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the learner-side sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _selfplay_lines(mz, n, type_name, games, sims, cycles, seed, rule="standard"):
    d = _desc(mz, n, 32, 1, type_name)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(n, rule)}:nn_type_name={type_name}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt"
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    assert wk.run_cycles(cycles) == cycles
    lines = wk.pop_lines()
    wk.close()
    assert len(lines) >= games
    return lines


@pytest.mark.parametrize("type_name,n,rule", [("alphazero", 15, "outer_open"), ("muzero", 9, "standard")])
def test_sampler_features_equal_the_host_engine(mz, type_name, n, rule):
    """DataLoader over self-play records: the planes the device replays for a sampled (game, position) are the host engine's planes of that position
    under one of the 8 rotations; MuZero's unrolled action planes are one-hot (no pass action: past the end of a game a random point, gomoku.cpp:177-185).  Any rotation is accepted here; the policy, value and reward targets, the cell the
    action plane marks and the one rotation they share with the planes are held to tests/loader_model.py in tests/test_gpu_loader_model.py."""
    lines = _selfplay_lines(mz, n, type_name, 6, 8, 9 * (n * n + 5), 21, rule)
    P = n * n
    lconf = f"{_conf(n, rule)}:nn_type_name={type_name}:learner_batch_size=64:learner_muzero_unrolling_step=3:program_seed=5"
    dl = mz.DataLoader(lconf)
    for l in lines:
        assert dl.add_record(l) == 1
    B, nf, na, npol, nv, nr = dl.shapes()
    assert nf == 4 * P
    games = [[int(a) for a in re.findall(r";[BW]\[(\d+)\]", l.split(" ", 5)[5])] for l in lines]
    for _ in range(2):
        bufs = [np.zeros((B, max(k, 1)), np.float32) for k in (nf, na, npol, nv, nr)] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]
        dl.sample_data(*bufs)
        feats, afeat, si = bufs[0], bufs[1], bufs[6]
        for b in range(B):
            g, pos = int(si[b][0]), int(si[b][1])
            env = mz.Env(_conf(n, rule))
            for a in games[g][:pos]:
                assert env.act(a)
            rots = [r for r in range(8) if np.array_equal(feats[b], env.features(r))]
            assert rots, f"sample {b}: (game {g}, position {pos}) is no rotation of the host engine's planes"
            if type_name == "muzero":
                planes = afeat[b].reshape(-1, P)
                assert np.array_equal(planes.sum(1), np.ones(len(planes), np.float32)) and set(np.unique(planes)) <= {0.0, 1.0}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the `-mode sp` executable
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sp_executable_plays_outer_open_gomoku(mz, tmp_path):
    """apps/mzgpu_sp -game gomoku on two logical devices: SelfPlay lines with GM[gomoku_oo_15x15] that replay legally."""
    from minizero_amd.export_weights import write_mzw
    env = dict(os.environ)
    if mz.device_count() < 2:
        env["MZ_DEVICE_MAP"] = "0,0"
    d = _desc(mz, 15, 32, 1)
    pt = str(tmp_path / "weight_iter_0.pt")
    write_mzw(pt[:-3] + ".mzw", d, mz.generate_weights(d, 0))
    conf_str = f"nn_file_name={pt}:program_seed=5:actor_num_simulation=8:zero_num_parallel_games=8:zero_num_threads=2:env_gomoku_rule=outer_open"
    p = subprocess.Popen([os.path.join(ROOT, "apps", "mzgpu_sp"), "-conf_str", conf_str, "-mode", "sp", "-game", "gomoku"], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    watchdog = threading.Timer(240, p.kill)
    watchdog.start()
    try:
        p.stdin.write("start\n")
        p.stdin.flush()
        lines = []
        while len(lines) < 4:
            l = p.stdout.readline().rstrip("\n")
            assert l, "the worker stopped printing"
            if l.startswith("SelfPlay "):
                lines.append(l)
        p.stdin.write("quit\n")
        p.stdin.flush()
        _, err = p.communicate(timeout=120)
    finally:
        watchdog.cancel()
        if p.poll() is None:
            p.kill()
    assert "8 games on" in err, err[-2000:]
    assert all("GM[gomoku_oo_15x15]" in l for l in lines)
    _check_records(lines, 15, "outer_open", True)
