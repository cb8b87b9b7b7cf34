"""Gomoku, Hex, NoGo and Havannah self-play, and whole games of Go and Othello in the environment of their rules models, held to the search model: the HIP worker against tests/search_model.py playing in tests/rule_envs.py, as exact
strings — action played, P dictionary, V tag, R tag, where the game ended and, for whole games, the RE tag — for every game of the pool, on the three
execution paths of these games: the per-game simulation kernel where the board has an instance, lock-step with the device rules, lock-step with the host
rules.  The three paths share the host search code, the candidate building and the use of the score at terminal leaves; comparing them with each other
(tests/test_gpu_{gomoku,hex,nogo,havannah}.py) cannot see a mistake there, the model can: the sign of a terminal value, the player of a child after a swap,
a candidate for NoGo's pass slot or for Havannah's cut-off cells, a draw backed up as a loss.  The rows, their weight seeds and the model's games are
those of tests/test_search_model.py (GAME_CASES, GAME_NOISY); tests/test_search_model_games.py pins on the CPU what each row shows.  The worker's
launch counters say which path ran.  Nothing here has a tolerance."""
import re

import pytest

import test_gpu_search_model as G
import test_search_model as T

pytestmark = pytest.mark.gpu

PATHS = {"default": "", "lockstep": G.LOCKSTEP, "lockstep_host_env": G.HOST_ENV}
RESULT = re.compile(r"RE\[([^\]]*)\]")


def run_row(mz, oracle, name, wseed, path):
    """one (row, seed) on one path: every game against the model; a whole-game row runs as many searches as the model's game has moves, plus one, and its
    finished records carry the model's result"""
    conf, _, _, _, games, _ = T.GAME_CASES[name]
    whole = name in T.WHOLE_GAMES
    played, resigned, finished = T.model_of(oracle, name, wseed)
    st = G.run_case(mz, oracle, name, wseed, PATHS[path], searches=len(played) + 1 if whole else None)
    if path == "default" and T.has_sim_instance(conf):
        assert st["sim_launches"] > 0, "the simulation kernel did not run"
    else:
        assert st["sim_launches"] == 0, (path, st["sim_launches"])
    if whole:
        assert len(st["lines"]) >= games
        score = float(T.model_env_of(oracle, name, wseed).score())
        for g, line in enumerate(st["lines"][:games]):
            assert float(RESULT.search(line).group(1)) == score, f"game {g}: RE {RESULT.search(line).group(1)}, the model's final position scores {score:g}"
    if resigned:  # the resign row: every game has ended, and its record holds the moves the model played before it resigned
        assert len(st["lines"]) >= games and all(len(T.MOVE.findall(line)) == len(played) for line in st["lines"][:games])
    return st


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name,wseed", T.ALL_GAME_CASES)
def test_game_row_equals_model(mz, oracle, name, wseed, path):
    """first moves on the simulation-kernel instances (Hex 11x11 with the swap, Gomoku 15x15 standard and outer-open, NoGo 9x9, Havannah edge 8 and edge 4),
    whole games through them, whole games on boards without an instance, whole Go games (4x4, 5x5 lock-step; 7x7 and 9x9 through sim_kernel_wide, 9x9 on
    8 channels through sim_kernel<9,9,20,8,2>) and Othello games (8x8 through its sim_kernel instance; 4x4, 6x6 lock-step), and the resign row: the worker resigns at the move where the model does
    (check_against compares the moves played and whether the game ended there)"""
    run_row(mz, oracle, name, wseed, path)


def test_terminal_leaves_evaluated_by_the_network_give_the_same_strings(mz, oracle, monkeypatch):
    """MZ_NO_SPEC=16 runs the network at terminal leaves too (sim_az_body.h); the value backed up there is still the score, so a whole Havannah edge 4
    game under PUCT — 130 terminal leaves in the model's searches — is the model's game either way"""
    name = "hav4_game_puct"
    monkeypatch.setenv("MZ_NO_SPEC", "16")
    st = run_row(mz, oracle, name, T.GAME_CASES[name][2][0], "default")
    assert st["sim_launches"] > 0


@pytest.mark.parametrize("path", ["default", "lockstep"])
@pytest.mark.parametrize("name", list(T.GAME_NOISY))
def test_noisy_first_move_equals_model(mz, oracle, name, path):
    """eight games, eight noise vectors: Gumbel noise on Hex 11x11, Dirichlet noise on Havannah edge 8, whose root has 169 children on the 225-cell array —
    one draw per legal child in child order, none for a cut-off corner"""
    conf, desc_args, wseed, _ = T.GAME_NOISY[name]
    got, st = G.worker_games(mz, oracle, conf, desc_args, T.case_weights(oracle, desc_args, wseed), T.NOISY_GAMES, 1, PATHS[path])
    assert len(T.check_noisy(oracle, name, got)) > 1
    assert (st["sim_launches"] == 0) == (path != "default")
