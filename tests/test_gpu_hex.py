"""Hex on the GPU: the device rules engine (go_body.h hexLeafBody, GoDevView::kind 4) against the host engine, the worker's three execution paths
(per-game simulation kernel sim_kernel_wide<11,11,16,C,-3>, lock-step with the device rules, lock-step with the host rules) against each other, every
finished record against the pure-Python rules model (tests/hex_rules.py: there is no oracle for this game), the learner-side sampler's device replay
and the `-mode sp` executable.  ref environment/hex/hex.{h,cpp}."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import hex_rules as R
from game_paths import GUMBEL, PATHS, run_paths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(n=11, swap=True):
    return f"env_game=hex:env_board_size={n}:env_hex_use_swap_rule={'true' if swap else 'false'}"


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


def _random_game(mz, conf, rng, take_swap):
    env, actions = mz.Env(conf), []
    while not env.is_terminal():
        legal = np.nonzero(env.legal_mask())[0]
        if len(actions) == 1 and take_swap is not None:
            a = actions[0] if take_swap else int(rng.choice([x for x in legal if x != actions[0]]))
        else:
            a = int(rng.choice(legal))
        assert env.act(a)
        actions.append(a)
    return actions, env.eval_score()


@pytest.mark.parametrize("n,swap,games", [(11, True, 9), (11, False, 6), (19, True, 3), (19, False, 3), (5, True, 12), (5, False, 9), (3, True, 9), (3, False, 6),
                                          (8, False, 6), (9, True, 6)])  # 8x8: one full 64-bit word of planes; 9x9: the second word has one 32-bit half only
def test_device_engine_matches_host_engine(mz, n, swap, games):
    """Random whole games; the device replays the tail action by action from roots at several depths (root_prefix 0 .. the last move, so that the
    winning stone is a device move): planes under random rotation arguments, legal mask, terminal flag, result and player to move after every
    action.  With the rule on every third game takes the swap: from a root at depth 0 the swap is the leaf at depth 2, from a root at depth 1 (a
    case of its own below) the leaf at depth 1."""
    rng = np.random.default_rng(100 * n + int(swap))
    conf = _conf(n, swap)
    outcomes = set()
    for g in range(games):
        actions, result = _random_game(mz, conf, rng, (g % 3 == 0) if swap else None)
        outcomes.add(result)
        root_prefix = [0, len(actions) // 3, len(actions) - 1][(g // 3 + g) % 3]  # (game 0, a swapped one, from depth 0)
        _device_vs_host(mz, conf, n, actions, root_prefix, rng)
        if swap and g % 3 == 0:
            _device_vs_host(mz, conf, n, actions, 1, rng)  # the swap as the first device move
            _device_vs_host(mz, conf, n, actions, 0, rng)
    assert outcomes <= {1.0, -1.0}  # no game ends without a winner
    if n > 3:
        assert outcomes == {1.0, -1.0}


def _p(x, y, n):
    return y * n + x


def _alternate(black, white, n):
    assert len(white) in (len(black), len(black) - 1)
    return [_p(*m, n) for pair in zip(black, white) for m in pair] + ([_p(*black[-1], n)] if len(white) < len(black) else [])


CHAIN_A = [(0, 3), (1, 3), (2, 4), (2, 5), (3, 5), (3, 4), (3, 3)]
CHAIN_B = [(2, 1), (1, 1), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0)]
CHAIN_WHITE = [(x, 6) for x in range(7)] + [(5, 3), (6, 3), (5, 4), (6, 4), (5, 5), (6, 5), (4, 5), (4, 4)]
HAND = [  # (n, swap, actions, expected terminal, expected eval after the last action — the device's move); the positions of test_hex_env.py
    (5, False, _alternate([(x, 2) for x in range(5)], [(x, 0) for x in range(4)], 5), True, 1.0),                      # a Black row
    (5, False, _alternate([(0, y) for y in range(5)], [(2, y) for y in range(5)], 5), True, -1.0),                     # a White column
    (7, False, _alternate(CHAIN_A + CHAIN_B + [(2, 2)], CHAIN_WHITE, 7), True, 1.0),                                   # all six adjacencies
    (2, False, [_p(1, 0, 2), _p(0, 0, 2), _p(0, 1, 2)], False, 0.0),                                                   # (x+1, y-1) is not adjacent
    (2, False, [_p(1, 0, 2), _p(0, 0, 2), _p(0, 1, 2), _p(1, 1, 2)], True, -1.0),                                      # the full 2x2 board, White wins
    (3, False, _alternate([(0, 2), (1, 1), (2, 0)], [(0, 0), (2, 2)], 3), False, 0.0),                                 # a chain over that diagonal
    (5, False, _alternate([(0, 0), (1, 0), (1, 1), (1, 2), (0, 2)], [(4, 0), (4, 1), (4, 2), (4, 3)], 5), False, 0.0),  # one edge twice
    (4, False, _alternate([(1, 0), (1, 1), (1, 2), (1, 3)], [(3, 0), (3, 1), (3, 2)], 4), False, 0.0),                 # Black from top to bottom
    (3, False, [_p(*m, 3) for m in [(1, 1), (2, 1), (2, 0), (0, 2), (0, 1), (2, 2), (1, 2), (0, 0), (1, 0)]], True, 1.0),  # the full 3x3 board
    (2, True, [0, 0, 2, 1], True, -1.0),                                                                               # the reflected stone's edge counts
    (11, True, [3 * 11 + 2, 3 * 11 + 2], False, 0.0),                                                                  # the swap itself
]


def test_hand_positions_with_the_deciding_stone_on_the_device(mz):
    rng = np.random.default_rng(3)
    for n, swap, actions, terminal, result in HAND:
        for root_prefix in (len(actions) - 1, 0):
            ref = _device_vs_host(mz, _conf(n, swap), n, actions, root_prefix, rng)
            assert ref.is_terminal() == terminal and ref.eval_score() == result, (n, swap, actions)
    # the masks around a swap on the device: all P cells after one action with the rule on, P - 1 with it off; after the swap the vacated cell is free
    n, a = 11, 3 * 11 + 2
    feat, legal, term, ev, pl = mz.envdev_playout_conf(_conf(n, True), n, [a, a], 0, [0, 0, 0], 4, n * n)
    assert legal[0].sum() == 121 and legal[1].sum() == 121 and legal[2].sum() == 120 and legal[2][a] and not legal[2][8 * 11 + 7]
    assert list(pl) == [1, 2, 1]
    feat, legal, term, ev, pl = mz.envdev_playout_conf(_conf(n, False), n, [a, a + 1], 0, [0, 0, 0], 4, n * n)
    assert legal[0].sum() == 121 and legal[1].sum() == 120 and not legal[1][a] and legal[2].sum() == 119


def _snake(n=11):
    """A Black chain of 51 stones that winds over the 11x11 board in five rows joined at alternating ends, with White stones that never cross it."""
    black = [(x, 1) for x in range(0, 10)] + [(9, 2)] + [(x, 3) for x in range(9, 0, -1)] + [(1, 4)] + [(x, 5) for x in range(1, 10)] + [(9, 6)] \
        + [(x, 7) for x in range(9, 0, -1)] + [(1, 8)] + [(x, 9) for x in range(1, 11)]
    white = [(x, 0) for x in range(11)] + [(x, 2) for x in range(9)] + [(x, 4) for x in range(2, 11)] + [(x, 6) for x in range(9)] \
        + [(x, 8) for x in range(2, 11)] + [(x, 10) for x in range(11)]  # never (10, 1): White cannot pass row 1
    return black, white


@pytest.mark.parametrize("deciding", [0, 25, 50])
def test_a_long_winding_chain_needs_many_flood_rounds(mz, deciding):
    """The deciding stone at one end, in the middle or at the other end of a 51-stone chain with eight turns: the flood runs for up to 50 rounds."""
    n = 11
    black, white = _snake(n)
    assert len(black) == 51 and len(set(black)) == 51 and not set(black) & set(white)
    last = black[deciding]
    order = _alternate([m for m in black if m != last] + [last], white[:50], n)
    model = R.Hex(n, False)
    for a in order[:-1]:
        assert model.act(a) and not model.is_terminal()
    assert model.act(order[-1]) and model.winner == 1  # (the model agrees that only the last stone decides)
    rng = np.random.default_rng(deciding)
    ref = _device_vs_host(mz, _conf(n, False), n, order, len(order) - 1, rng)
    assert ref.is_terminal() and ref.eval_score() == 1.0
    ref = _device_vs_host(mz, _conf(n, False), n, order, len(order) // 2, rng)
    assert ref.is_terminal() and ref.eval_score() == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the worker: records equal across the three execution paths, every finished record legal
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _desc(mz, n, c, blocks, type_name="alphazero"):
    return mz.make_desc(f"hex_{n}x{n}", 4, n, n, c, n, n, 1, blocks, n * n, vh=32, dv=1, type_name=type_name)


def _check_records(lines, n, swap):
    """Every record replays legally on the model with the right result and name; returns how many of them hold a swap (B[k];W[k])."""
    swaps = 0
    for line in lines:
        assert line.startswith("SelfPlay ")
        record = line.split(" ", 5)[5][:-2]
        model, re_value, gm = R.replay_record(record, n, swap)
        assert gm == f"hex_{n}x{n}"
        swaps += model.swapped
        # a finished game ends at its first winning move; an unfinished one was resigned: the player to move lost
        assert re_value == (model.eval_score() if model.is_terminal() else model.eval_score(resign=True)), record[:200]
    return swaps


CASES = [  # (c, blocks, extra configuration, swap, seed)
    (32, 2, "", True, 1),
    (64, 1, "", True, 2),
    (32, 1, GUMBEL, True, 3),
    (32, 1, "", False, 4),
]


@pytest.mark.parametrize("c,blocks,extra,swap,seed", CASES)
def test_records_equal_across_the_three_paths(mz, c, blocks, extra, swap, seed):
    """11x11, n = 16, 8 games until every game has finished at least once: the simulation kernel (asserted to have run, for 32 and for 64 channels),
    lock-step with device rules and lock-step with host rules write byte-identical lines and records; every finished record replays legally on the
    rules model with the right result."""
    n, sims, games = 11, 16, 8
    d = _desc(mz, n, c, blocks)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(n, swap)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2{extra}"
    cycles = (sims + 1) * 125  # longer than any game: 122 actions at most
    lines, recs = run_paths(mz, conf, d, w, games, cycles)
    assert len(lines) >= games
    swaps = _check_records(lines, n, swap)
    print(f"{len(lines)} records, {swaps} with a swap")
    assert swap or swaps == 0


def _drive(mz, conf, d, w, force_swap, max_actions):
    """Per-actor stepping of one game (mz_manual_step): after every search the caller plays the searched action — except the second action, which
    repeats the first one when force_swap (the swap) — and the search continues from there; the game is emitted when it ends."""
    wk = mz.Worker(conf, d, w)
    L = wk.L
    L.mz_worker_search_action.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mz_worker_act.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    for f in (L.mz_worker_search_done, L.mz_worker_reset_search):
        f.argtypes = [C.c_void_p]
    L.mz_worker_emit_game.argtypes = [C.c_void_p, C.c_int]
    wk.command("start")
    n = d.input_channel_height
    model, actions = R.Hex(n, True), []
    while not model.is_terminal():
        assert len(actions) < max_actions
        while not L.mz_worker_search_done(wk.h):
            assert wk.run_cycles(17) >= 0
        a, p, r = C.c_int(), C.c_int(), C.c_int()
        assert L.mz_worker_search_action(wk.h, 0, C.byref(a), C.byref(p), C.byref(r)) == 0
        act = actions[0] if (force_swap and len(actions) == 1) else a.value
        assert p.value == model.turn
        assert L.mz_worker_act(wk.h, 0, act, p.value) == 1
        assert model.act(act)
        actions.append(act)
        assert L.mz_worker_reset_search(wk.h) == 0
    assert L.mz_worker_emit_game(wk.h, 0) == 0
    st = wk.stats()
    lines = wk.pop_lines()
    wk.close()
    return actions, lines, st, model


@pytest.mark.parametrize("n,c", [(11, 32), (5, 32)])
def test_a_swap_in_self_play_and_the_search_after_it(mz, n, c):
    """One game driven action by action with the second action forced to be the swap: the searches after it (roots with Black's stone gone and
    White's on the reflection) agree on all three paths — same actions, byte-identical record, legal on the model.  (5x5 has no simulation-kernel
    instance: its default plan is the lock-step cycle with the device rules.)"""
    sims = 16
    d = _desc(mz, n, c, 1)
    w = mz.generate_weights(d, 9)
    conf = f"{_conf(n, True)}:actor_num_simulation={sims}:zero_num_parallel_games=1:program_seed=9:nn_file_name=x.pt:zero_num_threads=1:mz_manual_step=true"
    out = {}
    for path in PATHS:
        actions, lines, st, model = _drive(mz, conf + PATHS[path], d, w, True, n * n + 1)
        if n == 11:
            assert (st["sim_launches"] > 0) == (path == "sim"), (path, st)
        assert model.swapped and actions[1] == actions[0] and len(lines) == 1
        assert f";B[{actions[0]}]" in lines[0] and f";W[{actions[0]}]" in lines[0]  # the record keeps the chosen id: B[k];W[k]
        assert _check_records(lines, n, True) == 1
        out[path] = (actions, lines)
    assert out["lockstep_device"] == out["sim"] and out["lockstep_host"] == out["sim"]


def test_default_network_path(mz):
    """The reference's default network (1 block x 256 channels) on 11x11: whichever path the plan takes, the device rules are resident and its records
    after the first moves equal the host-rules path's."""
    n, sims, games = 11, 12, 4
    d = _desc(mz, n, 256, 1)
    w = mz.generate_weights(d, 7)
    conf = f"{_conf()}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=7:nn_file_name=x.pt:zero_num_threads=2"
    out = []
    for extra in ("", ":mz_device_env=false"):
        wk = mz.Worker(conf + extra, d, w)
        wk.command("start")
        assert wk.run_cycles(3 * (sims + 1)) == 3 * (sims + 1)
        st = wk.stats()
        assert (st["ms_env"] == 0) == (extra == ""), st
        out.append(wk.peek_records(games))
        wk.close()
    assert out[0] == out[1] and all(";B[" in r for r in out[0])


def test_muzero_and_gumbel_muzero_on_hex(mz):
    """MuZero and Gumbel MuZero (the host engine at the root only): finished records replay legally; the two MuZero paths agree."""
    n, sims, games = 7, 8, 6
    d = _desc(mz, n, 32, 1, "muzero")
    w = mz.generate_weights(d, 11)
    for variant in ("", GUMBEL):
        conf = f"{_conf(n)}:nn_type_name=muzero:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=11:nn_file_name=x.pt:zero_num_threads=2{variant}"
        out = []
        for extra in ("", ":mz_sim_kernel=false"):
            wk = mz.Worker(conf + extra, d, w)
            wk.command("start")
            assert wk.run_cycles((sims + 1) * 52) == (sims + 1) * 52
            out.append((wk.pop_lines(), wk.peek_records(games)))
            wk.close()
        assert out[0] == out[1]
        assert len(out[0][0]) >= games
        _check_records(out[0][0], n, True)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the learner-side sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name,n", [("alphazero", 11), ("muzero", 5)])
def test_sampler_features_equal_the_host_engine(mz, type_name, n):
    """DataLoader over self-play records, one of them with a forced swap (and, on 5x5, possibly P + 1 actions): the planes the device replays for a
    sampled (game, position) are the host engine's planes of that position — positions after the swap included; MuZero's unrolled action planes are
    one-hot (no pass action: past the end of a game a random cell, hex.cpp:364-371).  Hex has no rotation: the planes are compared at rotation 0 only; the policy, value and
    reward targets and the cell the action plane marks are held to tests/loader_model.py in tests/test_gpu_loader_model.py."""
    sims, games = 8, 6
    d = _desc(mz, n, 32, 1, type_name)
    w = mz.generate_weights(d, 21)
    conf = f"{_conf(n)}:nn_type_name={type_name}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=21:nn_file_name=x.pt"
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    cycles = (sims + 1) * (n * n + 3)
    assert wk.run_cycles(cycles) == cycles
    lines = wk.pop_lines()
    wk.close()
    assert len(lines) >= games
    manual = f"{_conf(n)}:nn_type_name={type_name}:actor_num_simulation={sims}:zero_num_parallel_games=1:program_seed=22:nn_file_name=x.pt:zero_num_threads=1:mz_manual_step=true"
    _, swapped, _, model = _drive(mz, manual, d, w, True, n * n + 1)
    assert model.swapped
    lines = swapped + lines[:games]
    P = n * n
    lconf = f"{_conf(n)}:nn_type_name={type_name}:learner_batch_size=96:learner_muzero_unrolling_step=3:program_seed=5"
    dl = mz.DataLoader(lconf)
    for l in lines:
        assert dl.add_record(l) == 1
    B, nf, na, npol, nv, nr = dl.shapes()
    assert nf == 4 * P
    recs = [[int(a) for a in re.findall(r";[BW]\[(\d+)\]", l.split(" ", 5)[5])] for l in lines]
    after_swap = 0
    for _ in range(3):
        bufs = [np.zeros((B, max(k, 1)), np.float32) for k in (nf, na, npol, nv, nr)] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]
        dl.sample_data(*bufs)
        feats, afeat, si = bufs[0], bufs[1], bufs[6]
        for b in range(B):
            g, pos = int(si[b][0]), int(si[b][1])
            env = mz.Env(_conf(n))
            for a in recs[g][:pos]:
                assert env.act(a)
            after_swap += g == 0 and pos >= 2
            assert np.array_equal(feats[b], env.features(0)), f"sample {b}: (game {g}, position {pos}) differs from the host engine's planes"
            if type_name == "muzero":
                planes = afeat[b].reshape(-1, P)
                assert np.array_equal(planes.sum(1), np.ones(len(planes), np.float32)) and set(np.unique(planes)) <= {0.0, 1.0}
    assert after_swap > 0  # a position after the swap was sampled


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the `-mode sp` executable
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sp_executable_plays_hex(mz, tmp_path):
    """apps/mzgpu_sp -game hex on two logical devices: SelfPlay lines with GM[hex_11x11] that replay legally."""
    from minizero_amd.export_weights import write_mzw
    env = dict(os.environ)
    if mz.device_count() < 2:
        env["MZ_DEVICE_MAP"] = "0,0"
    d = _desc(mz, 11, 32, 1)
    pt = str(tmp_path / "weight_iter_0.pt")
    write_mzw(pt[:-3] + ".mzw", d, mz.generate_weights(d, 0))
    conf_str = f"nn_file_name={pt}:program_seed=5:actor_num_simulation=8:zero_num_parallel_games=8:zero_num_threads=2"
    p = subprocess.Popen([os.path.join(ROOT, "apps", "mzgpu_sp"), "-conf_str", conf_str, "-mode", "sp", "-game", "hex"], stdin=subprocess.PIPE,
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
    assert all("GM[hex_11x11]" in l for l in lines)
    _check_records(lines, 11, True)
