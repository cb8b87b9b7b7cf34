"""Havannah on the GPU: the device rules engine (go_body.h havLeafBody, GoDevView::kind 6) against the host engine, the worker's three execution paths
(per-game simulation kernel sim_kernel_wide<E,E,32,C,-5>, lock-step with the device rules, lock-step with the host rules) against each other, every
finished record against the pure-Python rules model (tests/havannah_rules.py: there is no oracle for this game), the terminal leaves that skip the
network, the learner-side sampler's device replay and its refusals, and the `-mode sp` executable.  ref environment/havannah/havannah.{h,cpp}.
Edge size N plays on the E x E array, E = 2N - 1: N = 4 is one word per bitboard (7x7), N = 5 two (9x9), N = 8 four (15x15), N = 10 six (19x19)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import havannah_rules as R
from game_paths import GUMBEL, NO_RESIGN, child, run_paths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(N=8, swap=True):
    return f"env_game=havannah:env_board_size={N}:env_havannah_use_swap_rule={'true' if swap else 'false'}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the device engine against the host engine
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _device_vs_host(mz, conf, N, actions, root_prefix, rng):
    E = 2 * N - 1
    steps = len(actions) - root_prefix + 1
    rots = rng.integers(0, 8, steps).astype(np.int32)  # (no symmetries: the rotation argument changes nothing)
    feat, legal, term, ev, pl = mz.envdev_playout_conf(conf, E, actions, root_prefix, rots, 20, E * E)
    ref = mz.Env(conf)
    for a in actions[:root_prefix]:
        assert ref.act(a)
    for d in range(steps):
        where = f"{conf} step {d} (root_prefix {root_prefix}) actions {actions[:root_prefix + d]}"
        assert pl[d] == ref.turn(), where
        assert bool(term[d]) == ref.is_terminal(), where
        assert ev[d] == ref.eval_score(), where
        assert np.array_equal(legal[d], ref.legal_mask()), where
        assert np.array_equal(feat[d], ref.feature_bits(0, 20, E * E)), where
        if d + 1 < steps:
            assert ref.act(actions[root_prefix + d]), where
    return ref


SEEDS = {4: [0, 1, 2, 3, 14, 113, 118], 5: [0, 1, 2, 5, 7, 15], 8: [0, 1, 2], 10: [0]}  # test_havannah_env.py: every kind of win for each colour, and the draw


@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("N", sorted(SEEDS))
def test_device_engine_matches_host_engine(mz, N, swap):
    """Random whole games (the model's: won by bridge, fork and ring by either colour, and the full board); the device replays the tail action by action
    from roots at depth 0, at a third of the game and at the last move, so that the deciding stone is a device move and the history planes mix tree
    slots with the root's ring: planes, legal mask, terminal flag, result and player to move after every action."""
    rng = np.random.default_rng(10 * N + int(swap))
    decided = set()
    for k, seed in enumerate(SEEDS[N]):
        game = R.random_game(N, swap, seed, [True, False, None][seed % 3])
        decided.add(game.kinds[0] if game.kinds else "draw")
        actions = game.actions
        for root_prefix in sorted({0, len(actions) // 3, len(actions) - 1} if k < 2 or N < 8 else {[0, len(actions) // 3, len(actions) - 1][k % 3]}):
            ref = _device_vs_host(mz, _conf(N, swap), N, actions, root_prefix, rng)
            assert ref.is_terminal() and ref.eval_score() == game.eval_score()
    if swap and N in (4, 5):
        assert {(k, c) for k in ("bridge", "fork", "ring") for c in (1, 2)} <= decided
    if swap and N == 4:
        assert "draw" in decided


@pytest.mark.parametrize("name", sorted(R.HAND))
def test_hand_positions_with_the_deciding_stone_on_the_device(mz, name):
    h = R.HAND[name]
    rng = np.random.default_rng(3)
    for mover in (1, 2):
        N, seq = R.hand_sequence(name, mover)
        winner = {"a": mover, "b": 3 - mover, None: 0}[h["winner"]]
        for root_prefix in (len(seq) - 1, 0):
            ref = _device_vs_host(mz, _conf(N), N, seq, root_prefix, rng)
            assert ref.is_terminal() == (winner != 0) and ref.eval_score() == {0: 0.0, 1: 1.0, 2: -1.0}[winner], (name, mover)


def test_the_swap_and_the_draw_on_the_device(mz):
    rng = np.random.default_rng(4)
    h = R.SWAP_CORNER
    m = R.Havannah(h["N"])
    actions = [m.ident(c) for c in h["actions"]]
    for root_prefix in (0, 1, 2, len(actions) - 1):  # the swap as the second and as the first device move, and in the root
        ref = _device_vs_host(mz, _conf(4), 4, actions, root_prefix, rng)
        assert ref.is_terminal() and ref.eval_score() == -1.0
    # the masks around a swap on the device: all 37 cells after one action with the rule on, 36 with it off; after the swap the cell is taken
    a = actions[0]
    feat, legal, term, ev, pl = mz.envdev_playout_conf(_conf(4, True), 7, [a, a], 0, [0, 0, 0], 20, 49)
    assert legal[0].sum() == 37 and legal[1].sum() == 37 and legal[1][a] and legal[2].sum() == 36 and not legal[2][a] and list(pl) == [1, 2, 1]
    W32 = 2
    planes = feat.reshape(3, 20, W32)
    bit = lambda p, ch, i: (int(planes[p][ch][i >> 5]) >> (i & 31)) & 1
    assert bit(2, 0, a) == 1 and bit(2, 1, a) == 1  # after the swap the cell is in the own and in the opponent plane
    assert planes[1][17].tolist() == [0xFFFFFFFF, 0x1FFFF] and not planes[0][17].any() and not planes[2][17].any()  # swappable: all ones over the array
    feat, legal, term, ev, pl = mz.envdev_playout_conf(_conf(4, False), 7, [a, a + 1], 0, [0, 0, 0], 20, 49)
    assert legal[0].sum() == 37 and legal[1].sum() == 36 and not legal[1][a] and legal[2].sum() == 35 and not feat.reshape(3, 20, W32)[1][17].any()
    for root_prefix in (0, 12, 36):  # the full board: terminal, result 0
        ref = _device_vs_host(mz, _conf(4), 4, R.DRAW_N4, root_prefix, rng)
        assert ref.is_terminal() and ref.eval_score() == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the worker: records equal across the three execution paths, every finished record legal
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _desc(mz, N, c, blocks, type_name="alphazero"):
    E = 2 * N - 1
    return mz.make_desc(f"havannah{N}x{N}", 20, E, E, c, E, E, 1, blocks, E * E, vh=32, dv=1, type_name=type_name)


def _check_records(lines, N, swap=True):
    """Every record replays legally on the model with the right result, name and SZ; returns how the games ended."""
    ends = []
    for line in lines:
        assert line.startswith("SelfPlay ")
        record = line.split(" ", 5)[5][:-2]
        assert f"SZ[{N}]" in record  # the edge size, not the array's side
        model, re_value, gm = R.replay_record(record, swap)
        assert gm == f"havannah{N}x{N}"
        assert model.is_terminal(), record[:200]  # (no resignation in these runs)
        assert re_value == model.eval_score(), record[:200]
        ends.append(model.last["kind"] or "draw")
    return ends


@pytest.mark.parametrize("extra,seed", [("", 1), (GUMBEL, 3)])
def test_records_equal_across_the_three_paths_whole_games(mz, extra, seed):
    """N = 4 (sim_kernel_wide<7,7,32,32,-5>), n = 16, 8 games, 1 block x 32, with PUCT and with a Gumbel root, (16 + 1) x 38 cycles — a game has 37
    actions at most, so every game finishes at least once: the three paths write byte-identical lines and records, and every finished record replays
    legally on the model with the same result."""
    N, sims, games = 4, 16, 8
    d = _desc(mz, N, 32, 1)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(N)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}{extra}"
    cycles = (sims + 1) * 38
    lines, recs = run_paths(mz, conf, d, w, games, cycles)
    assert len(lines) >= games
    ends = _check_records(lines, N)
    print(f"{len(lines)} records, ended by {sorted(set(ends))}")


@pytest.mark.parametrize("extra,seed", [("", 2), (GUMBEL, 4)])
def test_records_equal_across_the_three_paths_default_board(mz, extra, seed):
    """N = 8, the default: sim_kernel_wide<15,15,32,32,-5> for three searches of 8 games: two moves at least stand in every record."""
    N, sims, games = 8, 16, 8
    d = _desc(mz, N, 32, 1)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(N)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}{extra}"
    lines, recs = run_paths(mz, conf, d, w, games, 3 * (sims + 1))
    assert all(r.count(";B[") >= 1 and r.count(";W[") >= 1 for r in recs), recs[0][:300]


def test_other_shapes_play_lock_step_on_the_device_rules(mz):
    """N = 5 (9x9 array) has no simulation-kernel instance: the default plan is the lock-step cycle with the device rules, and its records over whole games
    equal the host-rules path's."""
    N, sims, games = 5, 8, 6
    d = _desc(mz, N, 32, 1)
    w = mz.generate_weights(d, 5)
    conf = f"{_conf(N)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=5:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}"
    lines, recs = run_paths(mz, conf, d, w, games, (sims + 1) * 62, paths=("sim", "lockstep_host"), expect_sim=False)
    assert len(lines) >= games
    _check_records(lines, N)


def test_terminal_leaves_skip_the_network(mz):
    """Winner and full board are known before the tower would start: simulations whose leaf is terminal run no planes, tower or heads (MZ_SIM_PROF counts
    them), and the records are the ones of a run that evaluates every leaf (MZ_NO_SPEC=16)."""
    games, sims = 5, 12
    args = ("havannah4x4", 20, 7, 7, 32, 7, 7, 1, 1, 49, 16, 1, "alphazero")
    conf = f"{_conf(4)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:actor_use_dirichlet_noise=false:program_seed=11:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}"
    cycles = (sims + 1) * 38
    skip = child(conf, args, 3, cycles, games, 0)
    full = child(conf, args, 3, cycles, games, 16)
    print(f"network skipped in {skip['skipped']} of {skip['sims']} simulations; with MZ_NO_SPEC=16 in {full['skipped']} of {full['sims']}")
    for r in (skip, full):
        assert r["sim_launches"] > 0 and r["sims"] == cycles * games
    assert skip["skipped"] > 0 and full["skipped"] == 0
    assert skip["lines"] == full["lines"] and skip["records"] == full["records"]
    assert len(skip["lines"]) >= games
    _check_records(skip["lines"], 4)


def test_bf16x3_takes_a_path_that_exists(mz):
    """There is no bf16x3 Havannah simulation kernel: with mz_nn_precision=bf16x3 the pool plays lock-step on the device rules, or is refused with a message."""
    N, sims, games = 4, 8, 4
    d = _desc(mz, N, 32, 1)
    w = mz.generate_weights(d, 5)
    conf = f"{_conf(N)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=5:nn_file_name=x.pt:zero_num_threads=2:mz_nn_precision=bf16x3"
    try:
        wk = mz.Worker(conf, d, w)
    except mz.MzError as e:
        assert "bf16" in str(e)
        return
    wk.command("start")
    assert wk.run_cycles(2 * (sims + 1)) == 2 * (sims + 1)
    st = wk.stats()
    assert st["sim_launches"] == 0 and st["ms_env"] == 0, st
    assert all(";B[" in r for r in wk.peek_records(games))
    wk.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the learner-side sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sampler_features_equal_the_host_engine(mz):
    """DataLoader over finished self-play records (SZ = the edge size), one hand-written record with the swap among them: the planes the device replays
    for a sampled (game, position) are the host engine's planes of that position — positions after the swap, with the cell in both planes, included.  Havannah has
    no rotation: the planes are compared at rotation 0 only; the policy and value targets are held to tests/loader_model.py in tests/test_gpu_loader_model.py."""
    N, sims, games = 4, 8, 6
    E, P = 7, 49
    d = _desc(mz, N, 32, 1)
    w = mz.generate_weights(d, 21)
    conf = f"{_conf(N)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=21:nn_file_name=x.pt{NO_RESIGN}"
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    cycles = (sims + 1) * 38
    assert wk.run_cycles(cycles) == cycles
    lines = wk.pop_lines()[:games]
    wk.close()
    assert len(lines) == games
    m = R.Havannah(N)
    swap_actions = [m.ident(c) for c in R.SWAP_CORNER["actions"]]
    swapped = "(;GM[havannah4x4]RE[-1]SZ[4]" + "".join(f";{'BW'[i & 1]}[{a}]" for i, a in enumerate(swap_actions)) + ")"
    dl = mz.DataLoader(f"{_conf(N)}:learner_batch_size=96:program_seed=5")
    assert dl.add_record(swapped) == 1, mz.last_error()
    for l in lines:
        assert dl.add_record(l) == 1
    B, nf, na, npol, nv, nr = dl.shapes()
    assert nf == 20 * P and npol == P
    recs = [swap_actions] + [[int(a) for a in re.findall(r";[BW]\[(\d+)\]", l.split(" ", 5)[5])] for l in lines]
    after_swap = late = 0
    for _ in range(2):
        bufs = [np.zeros((B, max(k, 1)), np.float32) for k in (nf, na, npol, nv, nr)] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]
        dl.sample_data(*bufs)
        feats, si = bufs[0], bufs[6]
        for b in range(B):
            g, pos = int(si[b][0]), int(si[b][1])
            env = mz.Env(_conf(N))
            for a in recs[g][:pos]:
                assert env.act(a)
            after_swap += g == 0 and pos >= 2
            late += pos >= 9  # (all eight history planes filled)
            assert np.array_equal(feats[b], env.features(0)), f"sample {b}: (game {g}, position {pos}) differs from the host engine's planes"
    assert after_swap > 0 and late > 0


def test_sampler_refuses_illegal_records_by_move_and_reason(mz):
    """SZ is the edge size; a cell off the board, an occupied cell and a move after the game ended are refused by move index and reason."""
    dl = mz.DataLoader(f"{_conf(4, False)}:learner_batch_size=4:program_seed=1")

    def record(actions, sz=4):
        return f"(;GM[havannah4x4]RE[1]SZ[{sz}]" + "".join(f";{'BW'[i & 1]}[{a}]" for i, a in enumerate(actions)) + ")"
    N, bridge = R.hand_sequence("bridge", 1)
    assert dl.add_record(record(bridge)) == 1, mz.last_error()
    spare = next(a for a in range(48, 0, -1) if R.Havannah(4).is_legal(a) and a not in bridge)
    refused = [
        ([24, 0], "move 1 ", "off the board"),
        ([24, 25, 24], "move 2 ", "occupied point"),
        ([24, 24], "move 1 ", "occupied point"),  # (the rule is off: no swap)
        (bridge + [spare], f"move {len(bridge)} ", "the game has ended"),
    ]
    for actions, where, why in refused:  # (a record that does not load is skipped: 0, with the reason as the last error)
        assert dl.add_record(record(actions)) == 0, actions
        err = mz.last_error()
        assert where in err and why in err, err
    assert dl.add_record(record(bridge, sz=7)) == 0 and "record of a 7x7 board, the loader is configured for 4x4" in mz.last_error()
    assert dl.num_games() == 1
    dl = mz.DataLoader(f"{_conf(4, True)}:learner_batch_size=4:program_seed=1")
    assert dl.add_record(record([24, 24, 25])) == 1, mz.last_error()  # with the rule on the same record is a swap


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the `-mode sp` executable
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sp_executable_plays_havannah(mz, tmp_path):
    """apps/mzgpu_sp -game havannah on two logical devices: SelfPlay lines with GM[havannah4x4] and SZ[4] that replay legally."""
    from minizero_amd.export_weights import write_mzw
    env = dict(os.environ)
    if mz.device_count() < 2:
        env["MZ_DEVICE_MAP"] = "0,0"
    d = _desc(mz, 4, 32, 1)
    pt = str(tmp_path / "weight_iter_0.pt")
    write_mzw(pt[:-3] + ".mzw", d, mz.generate_weights(d, 0))
    conf_str = f"nn_file_name={pt}:env_board_size=4:program_seed=5:actor_num_simulation=8:zero_num_parallel_games=8:zero_num_threads=2:actor_resign_threshold=-2"
    p = subprocess.Popen([os.path.join(ROOT, "apps", "mzgpu_sp"), "-conf_str", conf_str, "-mode", "sp", "-game", "havannah"], stdin=subprocess.PIPE,
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
    assert all("GM[havannah4x4]" in l for l in lines)
    _check_records(lines, 4)
