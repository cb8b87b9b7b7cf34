"""mz_think_reuse_tree as far as it can be checked without a GPU: the new entry point is declared in include/mzgpu.h and exported (the symbol list of
tests/test_capi.py, mirrored here for the new symbol), the key loads into every configuration with its type, and the refusals that need no device — on an
external-evaluator worker, on a match worker, without mz_manual_step, with a batch of one and with root noise — name the key."""
import ctypes as C

import pytest

import test_capi

KEY = "mz_think_reuse_tree"
GO = "env_game=go:env_board_size=9:actor_num_simulation=8:zero_num_parallel_games=2:actor_use_dirichlet_noise=false"
THINK = ":mz_manual_step=true:actor_mcts_think_batch_size=4"


def test_symbol_is_declared_and_exported(mz):
    L = mz.load()
    assert "mz_worker_think_reuse_stats" in test_capi.declared_symbols() and hasattr(L, "mz_worker_think_reuse_stats")
    assert "mz_worker_think_stats" in test_capi.declared_symbols(), "the existing read-out keeps its symbol"
    assert L.mz_worker_think_reuse_stats(None, None, None, None) == -1 and b"NULL" in L.mz_last_error()
    assert hasattr(mz.Worker, "think_reuse_stats")


def test_key_loads_with_its_type(mz):
    for v in ("true", "false"):
        mz.Env(f"env_game=tictactoe:{KEY}={v}").close()
    with pytest.raises(mz.MzError):
        mz.Env(f"env_game=tictactoe:{KEY}=maybe")


def test_refusals_that_need_no_device(mz):
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, 82)
    w = mz.generate_weights(d, 1)
    with pytest.raises(mz.MzError) as e:
        mz.ExternalWorker(GO + f":{KEY}=true", d, lambda rows: 0)
    assert KEY in str(e.value) and "external evaluator" in str(e.value), str(e.value)
    with pytest.raises(mz.MzError) as e:
        mz.MatchWorker(GO + f":mz_match_games=2:{KEY}=true", d, w, w)
    assert KEY in str(e.value) and "match" in str(e.value), str(e.value)
    for extra, word in ((":actor_mcts_think_batch_size=4", "mz_manual_step"), (":mz_manual_step=true", "actor_mcts_think_batch_size"),
                        (THINK + ":actor_use_dirichlet_noise=true", "actor_use_dirichlet_noise"), (THINK + ":actor_use_gumbel_noise=true", "actor_use_gumbel_noise")):
        with pytest.raises(mz.MzError) as e:
            mz.Worker(GO + extra + f":{KEY}=true", d, w)
        assert KEY in str(e.value) and word in str(e.value), str(e.value)
    # with the key false or absent the same configurations get the answers they always got
    with pytest.raises(mz.MzError) as e:
        mz.ExternalWorker(GO + f":actor_mcts_think_batch_size=2:{KEY}=false", d, lambda rows: 0)
    assert KEY not in str(e.value) and "actor_mcts_think_batch_size" in str(e.value)
