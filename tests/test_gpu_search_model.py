"""The HIP worker against the search model of tests/search_model.py (written from the reference's text, independent of oracle/): action played, P tag, V tag
and the end of the game as exact strings, for the first moves of a pool of noise-free games, on every execution path that carries Gumbel or PUCT logic: the
per-game simulation kernels (sim_kernel, sim_kernel_mz, the one-tile wide kernel), the Gumbel rounds of MuZero, lock-step with the device's and with the
host's environment, and a first move under Gumbel noise.  The configurations and the model's games are those of tests/test_search_model.py, which holds the
model to the oracle on the CPU.  The games of a noise-free pool are identical by construction: each is compared with the model, so one that differs from its
neighbours (a leak between games) fails too."""
import pytest

import test_search_model as T

pytestmark = pytest.mark.gpu

LOCKSTEP = ":mz_sim_kernel=false"
HOST_ENV = ":mz_sim_kernel=false:mz_device_env=false"
NO_ROUNDS = ":mz_sim_rounds_board=false"


def worker_games(mz, oracle, conf, desc_args, w, games, moves, extra=""):
    """moves + 1 whole searches, one call each (calls that end on a move's boundary keep the simulation kernel and the rounds in play)"""
    n = T.model_cfg(conf)[0].actor_num_simulation
    d = mz.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    wk = mz.Worker(conf + f":zero_num_parallel_games={games}" + T.QUIET + extra, d, w)
    wk.command("start")
    for _ in range(moves + 1):
        assert wk.run_cycles(n + 1) == n + 1
    st = wk.stats()
    out = T.games_of(wk.pop_lines(), wk.peek_records(games), games, moves)
    wk.close()
    return out, st


def run_case(mz, oracle, name, wseed, extra=""):
    conf, desc_args, _, moves, games, vgain = T.CASES[name]
    got, st = worker_games(mz, oracle, conf, desc_args, T.case_weights(oracle, desc_args, wseed, vgain), games, moves, extra)
    T.check_against(T.model_of(oracle, name, wseed), got)
    return st


SIM_CASES = [(n, s) for n, s in T.ALL_CASES if not n.startswith("ttt")]
TTT_CASES = [(n, s) for n, s in T.ALL_CASES if n.startswith("ttt")]
# lock-step: the Go and Othello rows of the table once more, one weight seed each
LOCKSTEP_CASES = [(n, c[2][0]) for n, c in T.CASES.items() if n.startswith(("go_gumbel", "go_puct", "othello"))]
ROUND_CASES = ["go_mz_gumbel_n16_m16", "go_mz_gumbel_n12_m8"]


@pytest.mark.parametrize("name,wseed", SIM_CASES, ids=lambda x: str(x))
def test_simulation_kernel_equals_model(mz, oracle, name, wseed):
    """sim_kernel<9,9,...>, the Othello instance, sim_kernel_mz (with the Gumbel rounds where the plan takes them) and the one-tile wide kernel"""
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
    """eight games, eight Gumbel vectors (T.noisy_models says which draws): the top m by noisy logit, and logit - noise in the policy"""
    conf, desc_args, wseed = T.NOISY[name]
    got, st = worker_games(mz, oracle, conf, desc_args, T.case_weights(oracle, desc_args, wseed), T.NOISY_GAMES, 1, extra)
    assert len(T.check_noisy(T.noisy_models(oracle, name), got)) > 1
    assert (st["sim_launches"] == 0) == bool(extra)
