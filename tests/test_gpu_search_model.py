"""The HIP worker against the search model of tests/search_model.py (written from the reference's text, independent of oracle/): action played, P tag, V tag,
R tag and the end of the game as exact strings, for the first moves of a pool of noise-free games, on every execution path that carries Gumbel or PUCT logic:
the per-game simulation kernels (sim_kernel, sim_kernel_mz under Gumbel and under PUCT, the one-tile wide kernel), the Gumbel rounds of MuZero, lock-step with
the device's and with the host's environment, the Atari-shaped search (value rescaling, reward discount, one player, 601-bin heads) on each of its execution
modes, and a first move under Gumbel or Dirichlet noise.  The configurations and the model's games are those of tests/test_search_model.py, which holds the
model to the oracle on the CPU.  The games of a noise-free board pool are identical by construction: each is compared with the model, so one that differs
from its neighbours (a leak between games) fails too; the games of an Atari-shaped pool each have their own seed and are compared with the model's game of it."""
import pytest

import test_search_model as T

pytestmark = pytest.mark.gpu

LOCKSTEP = ":mz_sim_kernel=false"
HOST_ENV = ":mz_sim_kernel=false:mz_device_env=false"
NO_ROUNDS = ":mz_sim_rounds_board=false"


def worker_games(mz, oracle, conf, desc_args, w, games, moves, extra="", searches=None):
    """moves + 1 whole searches (or `searches` of them), one call each (calls that end on a move's boundary keep the simulation kernel and the rounds in
    play); the finished lines of the run are left in the statistics under "lines" """
    n = T.model_cfg(conf)[0].actor_num_simulation
    d = mz.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    wk = mz.Worker(T.full_conf(conf, games) + extra, d, w)
    wk.command("start")
    for _ in range(moves + 1 if searches is None else searches):
        assert wk.run_cycles(n + 1) == n + 1
    st = dict(wk.stats())
    st["lines"] = wk.pop_lines()
    out = T.games_of(st["lines"], wk.peek_records(games), games, moves)
    wk.close()
    return out, st


def run_case(mz, oracle, name, wseed, extra="", games=None, searches=None):
    conf, desc_args, _, moves, case_games, vgain = T.row(name)
    got, st = worker_games(mz, oracle, conf, desc_args, T.case_weights(oracle, desc_args, wseed, vgain), games or case_games, moves, extra, searches)
    T.check_against(T.case_model(oracle, name, wseed), got)
    if T.is_atari(conf):
        T.check_atari_pool_shows_something(got)
    return st


SIM_CASES = [(n, s) for n, s in T.ALL_CASES if not n.startswith(("ttt", "atari"))]
TTT_CASES = [(n, s) for n, s in T.ALL_CASES if n.startswith("ttt")]
# lock-step: the Go (AlphaZero and MuZero, Gumbel and PUCT) and Othello rows of the table once more, one weight seed each
LOCKSTEP_CASES = [(n, c[2][0]) for n, c in T.CASES.items() if n.startswith(("go_gumbel", "go_puct", "go_mz", "othello"))]
ROUND_CASES = ["go_mz_gumbel_n16_m16", "go_mz_gumbel_n12_m8"]


@pytest.mark.parametrize("name,wseed", SIM_CASES, ids=lambda x: str(x))
def test_simulation_kernel_equals_model(mz, oracle, name, wseed):
    """sim_kernel<9,9,...>, the Othello instance, sim_kernel_mz under Gumbel (with the Gumbel rounds where the plan takes them) and under PUCT, and the
    one-tile wide kernel"""
    st = run_case(mz, oracle, name, wseed)
    assert st["sim_launches"] > 0, "the simulation kernel did not run"


@pytest.mark.parametrize("name,wseed", TTT_CASES, ids=lambda x: str(x))
def test_tictactoe_equals_model(mz, oracle, name, wseed):
    """the candidate count shrinks below the sample size move by move; terminal leaves inside the search; the environment is the test's own Python"""
    assert run_case(mz, oracle, name, wseed)["sim_launches"] > 0
    assert run_case(mz, oracle, name, wseed, LOCKSTEP)["sim_launches"] == 0


@pytest.mark.parametrize("extra", [LOCKSTEP, HOST_ENV], ids=["lockstep", "lockstep_host_env"])
@pytest.mark.parametrize("name,wseed", LOCKSTEP_CASES, ids=lambda x: str(x))
def test_lockstep_equals_model(mz, oracle, name, wseed, extra):
    """the host's gumbelSequentialHalving / gumbelSortByScore choose every simulation's start child here"""
    assert run_case(mz, oracle, name, wseed, extra)["sim_launches"] == 0


@pytest.mark.parametrize("name", ROUND_CASES)
def test_muzero_gumbel_rounds_equal_model(mz, oracle, name):
    """leaves of a round evaluated ahead of the simulations that consume them, and the same searches without rounds"""
    wseed = T.CASES[name][2][0]
    on = run_case(mz, oracle, name, wseed)
    off = run_case(mz, oracle, name, wseed, NO_ROUNDS)
    assert on["pre_evals"] > 0 and on["pre_hits"] > 0 and off["pre_evals"] == 0
    assert on["sim_launches"] > 0 and off["sim_launches"] > 0


@pytest.mark.parametrize("extra", ["", LOCKSTEP], ids=["sim_kernel", "lockstep"])
@pytest.mark.parametrize("name", list(T.NOISY))
def test_noisy_first_move_equals_model(mz, oracle, name, extra):
    """eight games, eight noise vectors (T.noisy_model says which draws).  Gumbel: the top m by noisy logit, and logit - noise in the policy; Dirichlet: PUCT
    on (1 - eps) * p + eps * noise, on Go as AlphaZero and as MuZero, on Othello and on the Atari-shaped game"""
    conf, desc_args, wseed, _ = T.NOISY[name]
    got, st = worker_games(mz, oracle, conf, desc_args, T.case_weights(oracle, desc_args, wseed), T.NOISY_GAMES, 1, extra)
    assert len(T.check_noisy(oracle, name, got)) > 1
    assert (st["sim_launches"] == 0) == bool(extra)


# ---------------------------------------------------------------------------------------------
# the Atari-shaped rows: name of the mode -> (games, configuration keys, what the counters must say)
# ---------------------------------------------------------------------------------------------
def _rounds(st): return st["sim_launches"] > 0 and st["pre_evals"] > 0 and 0 < st["pre_hits"] <= st["pre_evals"]
def _no_rounds(st): return st["sim_launches"] > 0 and st["pre_evals"] == 0 and st["pre_launches"] == 0


ATARI_MODES = {
    # the default plan: the leaves of a Gumbel round are evaluated ahead of the simulations that consume them
    "rounds": (5, "", _rounds),
    "rounds_64_games": (64, "", _rounds),
    # the batched pipeline of sim_rounds.hip, forced onto small pools by the leaves per trunk workgroup
    "rounds_batched_2": (7, ":mz_sim_round_leaves=2", lambda st: _rounds(st) and st["pre_batch_launches"] > 0),
    "rounds_batched_4": (13, ":mz_sim_round_leaves=4", lambda st: _rounds(st) and st["pre_batch_launches"] > 0),
    # one workgroup per leaf (sim_pre_kernel_mz), and the same without pairs of workgroups per leaf (sim_pre_pair_kernel_mz)
    "rounds_one_workgroup_per_leaf": (13, ":mz_sim_round_batch=false", lambda st: _rounds(st) and st["pre_batch_launches"] == 0),
    "rounds_no_pairs": (13, ":mz_sim_round_pairs=false", lambda st: _rounds(st) and st["pre_pair_launches"] == 0),
    # clusters of four workgroups per game: ragged octets (every game keeps its heads) and full octets (sim_cluster.h octetHead)
    "clusters_13_games": (13, ":mz_sim_rounds=false", _no_rounds),
    "clusters_64_games": (64, ":mz_sim_rounds=false", _no_rounds),
    "one_workgroup_per_game": (5, ":mz_sim_cluster=false:mz_sim_rounds=false", _no_rounds),
    "root_on_the_host": (5, ":mz_sim_split=false", _no_rounds),
    "lockstep": (5, LOCKSTEP, lambda st: st["sim_launches"] == 0 and st["pre_evals"] == 0),
}
FEW = ("rounds", "rounds_batched_2", "clusters_13_games", "lockstep")
# (row, weight seed, modes): the small row on every mode; the other shapes (never halved, n < m, m no power of two, m = 18) where the shape matters
ATARI_RUNS = [("atari_gumbel_n16_m4", 1, tuple(ATARI_MODES)), ("atari_gumbel_n16_m4", 2, ("rounds",))]
ATARI_RUNS += [(n, T.CASES[n][2][0], FEW) for n in ("atari_gumbel_n16_m16", "atari_gumbel_n7_m16", "atari_gumbel_n50_m12", "atari_gumbel_n40_m18")]
# the benchmark's network: its kernel instances, with and without rounds
ATARI_RUNS += [("atari_c5_gumbel_n16_m4", 1, ("rounds", "clusters_13_games"))]
# discount 1.0 with and without value rescaling (without it the cluster kernel backs up beside the expand)
ATARI_RUNS += [("atari_gumbel_n16_m4_undiscounted", 1, ("rounds", "lockstep")),
               ("atari_gumbel_n16_m4_plain", 1, ("rounds", "clusters_13_games", "one_workgroup_per_game", "lockstep"))]


@pytest.mark.parametrize("name,wseed,mode", [(n, s, m) for n, s, modes in ATARI_RUNS for m in modes], ids=lambda x: str(x))
def test_atari_gumbel_equals_model(mz, oracle, name, wseed, mode):
    """Gumbel MuZero on the Atari-shaped game, every game against the model's game of its own seed; the modes differ only in where an evaluation runs, and
    the counters say that the one meant did run"""
    games, extra, ran = ATARI_MODES[mode]
    st = run_case(mz, oracle, name, wseed, extra, games)
    assert ran(st), (mode, st)


@pytest.mark.parametrize("extra", ["", LOCKSTEP], ids=["sim_kernel", "lockstep"])
@pytest.mark.parametrize("name", ["atari_puct_n12", "atari_puct_n24"])
def test_atari_puct_equals_model(mz, oracle, name, extra):
    """value-rescaled PUCT at the root too (no Gumbel, so no rounds): the simulation kernel of the default plan, and lock-step"""
    st = run_case(mz, oracle, name, T.CASES[name][2][0], extra, 9)
    assert (st["sim_launches"] == 0) == bool(extra) and st["pre_evals"] == 0, st
