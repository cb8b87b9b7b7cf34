"""NoGo on the GPU: the device rules engine (go_body.h nogoLeafBody, GoDevView::kind kNoGo = 5: a rules variant of Go's row) against the host engine, the
worker's three execution paths (per-game simulation kernel sim_kernel<9,9,20,C,-4> / sim_kernel_wide<9,9,32,C,-4>, lock-step with the device rules,
lock-step with the host rules) against each other, every finished record against the pure-Python rules model (tests/nogo_rules.py: there is no oracle
for this game), the terminal leaves that skip the network, the learner-side sampler's device replay and the `-mode sp` executable.
ref environment/nogo/nogo.h."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import nogo_rules as R
from game_paths import GUMBEL, NO_RESIGN, child, run_paths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(n=9):
    return f"env_game=nogo:env_board_size={n}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the device engine against the host engine
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _device_vs_host(mz, n, actions, root_prefix, rng):
    conf = _conf(n)
    steps = len(actions) - root_prefix + 1
    rots = rng.integers(0, 8, steps).astype(np.int32)
    feat, legal, term, ev, pl = mz.envdev_playout_conf(conf, n, actions, root_prefix, rots, 18, n * n + 1)
    ref = mz.Env(conf)
    for a in actions[:root_prefix]:
        assert ref.act(a)
    for d in range(steps):
        where = f"{conf} step {d} (root_prefix {root_prefix}) actions {actions[:root_prefix + d]}"
        assert pl[d] == ref.turn(), where
        assert bool(term[d]) == ref.is_terminal(), where
        assert ev[d] == ref.eval_score(), where
        assert np.array_equal(legal[d], ref.legal_mask()), where
        assert np.array_equal(feat[d], ref.feature_bits(int(rots[d]), 18, n * n)), where
        if d + 1 < steps:
            assert ref.act(actions[root_prefix + d]), where
    return ref


def _random_game(mz, n, rng):
    env, actions = mz.Env(_conf(n)), []
    while not env.is_terminal():
        a = int(rng.choice(np.nonzero(env.legal_mask())[0]))
        assert env.act(a)
        actions.append(a)
    return actions, env.eval_score()


@pytest.mark.parametrize("n,games", [(9, 6), (5, 9), (3, 9), (2, 6)])
def test_device_engine_matches_host_engine(mz, n, games):
    """Random whole games; the device replays the tail action by action from roots at depth 0, a third of the game and the last move (so that the move
    that ends the game is a device move, and the history planes mix tree slots with the root's ring): planes under random rotations, legal mask,
    terminal flag, result and player to move after every action.  9x9 has two words per bitboard, the others one."""
    rng = np.random.default_rng(100 + n)
    outcomes = set()
    for g in range(games):
        actions, result = _random_game(mz, n, rng)
        outcomes.add(result)
        root_prefix = [0, len(actions) // 3, len(actions) - 1][g % 3]
        ref = _device_vs_host(mz, n, actions, root_prefix, rng)
        assert ref.is_terminal() and ref.eval_score() == result
    assert outcomes <= {1.0, -1.0}
    if n in (3, 5, 9):
        assert outcomes == {1.0, -1.0}


@pytest.mark.parametrize("mover", [1, 2])
@pytest.mark.parametrize("name", sorted(R.HAND))
def test_hand_positions_with_the_deciding_stone_on_the_device(mz, name, mover):
    """The positions of tests/test_nogo_env.py, the last stone placed by the device (and, from the empty root, all of them): the point in question is
    legal or not as stated, for the mover Black and for the mover White."""
    actions, point, legal = R.hand_sequence(name, mover)
    rng = np.random.default_rng(7)
    for root_prefix in (len(actions) - 1, 0):
        ref = _device_vs_host(mz, 9, actions, root_prefix, rng)
        assert ref.turn() == mover and bool(ref.legal_mask()[point]) == legal
    steps = 2
    feat, mask, term, ev, pl = mz.envdev_playout_conf(_conf(), 9, actions, len(actions) - 1, [0] * steps, 18, 82)
    assert bool(mask[-1][point]) == legal and mask[-1][81] == 0 and pl[-1] == mover and not term[-1]


def test_a_long_winding_chain_and_its_last_liberty(mz):
    """A Black chain of 40 stones that spirals over both words of the bitboard, every other point but one White's: the device move takes the chain's
    second-to-last liberty, which leaves Black — to move — without a legal point.  39 flood rounds for the chain, as many for White's block."""
    actions = R.spiral_chain()
    model = R.NoGo(9)
    for a in actions[:-1]:
        assert model.act(a)
    chain, libs = model.block(0)
    assert len(chain) == 40 and {63, 72} <= chain and len(libs) == 2 and not model.is_terminal()
    assert model.act(actions[-1])
    assert len(model.block(0)[1]) == 1 and model.is_terminal() and model.eval_score() == -1.0
    rng = np.random.default_rng(1)
    for root_prefix in (len(actions) - 1, len(actions) - 12):
        ref = _device_vs_host(mz, 9, actions, root_prefix, rng)
        assert ref.is_terminal() and ref.eval_score() == -1.0 and ref.turn() == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the worker: records equal across the three execution paths, every finished record legal
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _desc(mz, n, c, blocks, type_name="alphazero"):
    return mz.make_desc(f"nogo_{n}x{n}", 18, n, n, c, n, n, 1, blocks, n * n + 1, vh=32, dv=1, type_name=type_name)


def _check_records(lines, n):
    """Every finished record (no game is resigned: actor_resign_threshold=-2) replays legally on the model, ends exactly where the model has no legal
    move, and carries the name and the result of the player who moved last."""
    for line in lines:
        assert line.startswith("SelfPlay ")
        record = line.split(" ", 5)[5][:-2]
        model, re_value, gm = R.replay_record(record, n)
        assert gm == f"nogo_{n}x{n}"
        assert f"SZ[{n}]" in record and "KM[" in record  # Go's tags (ref go.h:127-133)
        assert model.is_terminal(), record[:200]
        assert re_value == (1.0 if model.turn == 2 else -1.0) == model.eval_score(), record[:200]


CASES = [  # (c, blocks, extra configuration, seed)
    (64, 1, "", 1),
    (8, 2, "", 2),
    (8, 1, GUMBEL, 3),
]


@pytest.mark.parametrize("c,blocks,extra,seed", CASES)
def test_records_equal_across_the_three_paths(mz, c, blocks, extra, seed):
    """9x9, n = 16, 8 games, (16 + 1) x 82 cycles — no game reaches 81 moves, so every game finishes at least once: the simulation kernel (asserted to
    have run, for 64 and for 8 channels), lock-step with device rules and lock-step with host rules write byte-identical lines and records."""
    n, sims, games = 9, 16, 8
    d = _desc(mz, n, c, blocks)
    w = mz.generate_weights(d, seed)
    conf = f"{_conf(n)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}{extra}"
    cycles = (sims + 1) * 82
    lines, recs = run_paths(mz, conf, d, w, games, cycles)
    assert len(lines) >= games
    _check_records(lines, n)
    winners = {re.search(r"RE\[([^\]]*)\]", l).group(1) for l in lines}
    print(f"{len(lines)} records, results {sorted(winners)}")


def test_terminal_leaves_skip_the_network(mz):
    """The terminal flag is the emptiness of the legal mask, which the body has finished before the tower would start: simulations whose leaf is terminal
    run no planes, tower or heads (MZ_SIM_PROF counts them), and the records are the ones of a run that evaluates every leaf (MZ_NO_SPEC=16)."""
    games, sims = 5, 12
    args = ("nogo_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero")
    conf = f"{_conf()}:actor_num_simulation={sims}:zero_num_parallel_games={games}:actor_use_dirichlet_noise=false:program_seed=11:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}"
    cycles = (sims + 1) * 82
    skip = child(conf, args, 3, cycles, games, 0)
    full = child(conf, args, 3, cycles, games, 16)
    print(f"network skipped in {skip['skipped']} of {skip['sims']} simulations; with MZ_NO_SPEC=16 in {full['skipped']} of {full['sims']}")
    for r in (skip, full):
        assert r["sim_launches"] > 0 and r["sims"] == cycles * games
    assert skip["skipped"] > 0 and full["skipped"] == 0
    assert skip["lines"] == full["lines"] and skip["records"] == full["records"]
    assert len(skip["lines"]) >= games
    _check_records(skip["lines"], 9)


@pytest.mark.parametrize("c", [256, 128, 32])
def test_default_network_path(mz, c):
    """The reference's default network (1 block x 256 channels) on 9x9, and the other two widths of the one-tile simulation kernel: the kernel runs, the
    device rules are resident and the records after three moves equal the host-rules path's."""
    n, sims, games = 9, 12, 4
    d = _desc(mz, n, c, 1)
    w = mz.generate_weights(d, 7)
    conf = f"{_conf()}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=7:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}"
    out = []
    for extra in ("", ":mz_device_env=false"):
        wk = mz.Worker(conf + extra, d, w)
        wk.command("start")
        assert wk.run_cycles(3 * (sims + 1)) == 3 * (sims + 1)
        st = wk.stats()
        assert (st["ms_env"] == 0) == (extra == ""), st
        assert (st["sim_launches"] > 0) == (extra == ""), st
        out.append(wk.peek_records(games))
        wk.close()
    assert out[0] == out[1] and all(";B[" in r for r in out[0])


def test_5x5_plays_lock_step_on_the_device_rules(mz):
    """5x5 has no simulation-kernel instance: the default plan is the lock-step cycle with the device rules, and its records over whole games (terminal
    leaves are frequent on a board this small) equal the host-rules path's."""
    n, sims, games = 5, 16, 6
    d = _desc(mz, n, 32, 1)
    w = mz.generate_weights(d, 5)
    conf = f"{_conf(n)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=5:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}"
    cycles = (sims + 1) * 26
    lines, recs = run_paths(mz, conf, d, w, games, cycles, paths=("sim", "lockstep_host"), expect_sim=False)
    assert len(lines) >= games
    _check_records(lines, n)


def test_bf16x3_takes_a_path_that_exists(mz):
    """There is no bf16x3 NoGo simulation kernel: with mz_nn_precision=bf16x3 the pool plays lock-step on the device rules, or is refused with a message."""
    n, sims, games = 9, 8, 4
    d = _desc(mz, n, 64, 1)
    w = mz.generate_weights(d, 5)
    conf = f"{_conf(n)}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=5:nn_file_name=x.pt:zero_num_threads=2:mz_nn_precision=bf16x3"
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


def test_muzero_and_gumbel_muzero_on_nogo(mz):
    """MuZero and Gumbel MuZero on Go's 9x9 MuZero kernels (no environment in the search; the host engine serves the root): the two paths agree, and
    finished records replay legally."""
    n, sims, games = 9, 8, 6
    d = _desc(mz, n, 8, 1, "muzero")
    w = mz.generate_weights(d, 11)
    for variant in ("", GUMBEL):
        conf = f"{_conf(n)}:nn_type_name=muzero:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=11:nn_file_name=x.pt:zero_num_threads=2{NO_RESIGN}{variant}"
        out = []
        for extra in ("", ":mz_sim_kernel=false"):
            wk = mz.Worker(conf + extra, d, w)
            wk.command("start")
            assert wk.run_cycles((sims + 1) * 82) == (sims + 1) * 82
            out.append((wk.pop_lines(), wk.peek_records(games)))
            wk.close()
        assert out[0] == out[1]
        assert len(out[0][0]) >= games
        _check_records(out[0][0], n)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the learner-side sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", ["alphazero", "muzero"])
def test_sampler_features_equal_the_host_engine(mz, type_name):
    """DataLoader over finished self-play records: the planes the device replays for a sampled (game, position) are the host engine's planes of that
    position under one of the eight rotations; MuZero's unrolled action planes are Go's (one-hot on the board, empty for the action past a game's end that lands on the pass slot).
    The policy, value and reward targets, the point the action plane marks and the one rotation they share with the planes are held to tests/loader_model.py in
    tests/test_gpu_loader_model.py."""
    n, sims, games = 9, 8, 6
    d = _desc(mz, n, 8, 1, type_name)
    w = mz.generate_weights(d, 21)
    conf = f"{_conf(n)}:nn_type_name={type_name}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed=21:nn_file_name=x.pt{NO_RESIGN}"
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    cycles = (sims + 1) * 82
    assert wk.run_cycles(cycles) == cycles
    lines = wk.pop_lines()[:games]
    wk.close()
    assert len(lines) == games
    P = n * n
    lconf = f"{_conf(n)}:nn_type_name={type_name}:learner_batch_size=64:learner_muzero_unrolling_step=3:program_seed=5"
    dl = mz.DataLoader(lconf)
    for l in lines:
        assert dl.add_record(l) == 1
    B, nf, na, npol, nv, nr = dl.shapes()
    assert nf == 18 * P and npol == (P + 1) * (4 if type_name == "muzero" else 1)
    recs = [[int(a) for a in re.findall(r";[BW]\[(\d+)\]", l.split(" ", 5)[5])] for l in lines]
    late = 0
    for _ in range(2):
        bufs = [np.zeros((B, max(k, 1)), np.float32) for k in (nf, na, npol, nv, nr)] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]
        dl.sample_data(*bufs)
        feats, afeat, si = bufs[0], bufs[1], bufs[6]
        for b in range(B):
            g, pos = int(si[b][0]), int(si[b][1])
            env = mz.Env(_conf(n))
            for a in recs[g][:pos]:
                assert env.act(a)
            late += pos >= 9  # (all eight history planes filled)
            planes8 = [env.features(r) for r in range(8)]  # (the sampler draws the rotation and does not return it)
            rots = [r for r in range(8) if np.array_equal(feats[b], planes8[r])]
            assert rots, f"sample {b}: (game {g}, position {pos}) is no rotation of the host engine's planes"
            assert len(rots) == 1 or len({f.tobytes() for f in planes8}) < 8, f"sample {b}: (game {g}, position {pos}) matches rotations {rots} of an asymmetric position"
            if type_name == "muzero":
                planes = afeat[b].reshape(-1, P)
                assert set(np.unique(planes)) <= {0.0, 1.0} and (planes.sum(1) <= 1).all()
    assert late > 0


def test_sampler_refuses_illegal_records_with_nogo_reasons(mz):
    """SZ and KM like a Go record (ref go.h:127-133: NoGoEnvLoader is GoEnvLoader); a capturing move and a pass are refused by name."""
    dl = mz.DataLoader("env_game=nogo:env_board_size=9:learner_batch_size=4:program_seed=1")
    def record(actions):
        return "(;GM[nogo_9x9]RE[1]SZ[9]KM[7.5]" + "".join(f";{'BW'[i & 1]}[{a}]" for i, a in enumerate(actions)) + ")"
    assert dl.add_record(record([1, 0, 40])) == 1
    refused = [
        ([1, 0, 9], "move 2 ", "captures or is suicide"),       # B[9] takes the last liberty of the stone on 0
        ([1, 40, 9, 0], "move 3 ", "captures or is suicide"),   # W[0]: no liberty in the corner
        ([81], "move 0 ", "NoGo has no pass"),
        ([1, 1], "move 1 ", "occupied point"),
    ]
    for actions, where, why in refused:  # (a record that does not load is skipped: 0, with the reason as the last error)
        assert dl.add_record(record(actions)) == 0, actions
        err = mz.last_error()
        assert where in err and why in err and "repeated position" not in err, err
    assert dl.num_games() == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the `-mode sp` executable
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sp_executable_plays_nogo(mz, tmp_path):
    """apps/mzgpu_sp -game nogo on two logical devices: SelfPlay lines with GM[nogo_9x9] that replay legally."""
    from minizero_amd.export_weights import write_mzw
    env = dict(os.environ)
    if mz.device_count() < 2:
        env["MZ_DEVICE_MAP"] = "0,0"
    d = _desc(mz, 9, 8, 1)
    pt = str(tmp_path / "weight_iter_0.pt")
    write_mzw(pt[:-3] + ".mzw", d, mz.generate_weights(d, 0))
    conf_str = f"nn_file_name={pt}:program_seed=5:actor_num_simulation=8:zero_num_parallel_games=8:zero_num_threads=2:actor_resign_threshold=-2"
    p = subprocess.Popen([os.path.join(ROOT, "apps", "mzgpu_sp"), "-conf_str", conf_str, "-mode", "sp", "-game", "nogo"], stdin=subprocess.PIPE,
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
    assert all("GM[nogo_9x9]" in l for l in lines)
    _check_records(lines, 9)
