"""mz_think_symmetries as far as it can be checked without a GPU: the new entry point is declared in include/mzgpu.h and exported (the symbol list of
tests/test_capi.py, mirrored here for the new symbol) and refuses NULL, the key loads as 1 and as 8 and is refused as 3 and as x, and the refusals that need
no device — on an external-evaluator worker, on a match worker, without mz_manual_step and with a batch of one — name the key."""
import ctypes as C

import pytest

import test_capi

KEY = "mz_think_symmetries"
GO = "env_game=go:env_board_size=9:actor_num_simulation=8:zero_num_parallel_games=2:actor_use_dirichlet_noise=false"
THINK = ":mz_manual_step=true:actor_mcts_think_batch_size=4"


def test_symbol_is_declared_and_exported(mz):
    L = mz.load()
    assert "mz_worker_think_symmetry_stats" in test_capi.declared_symbols() and hasattr(L, "mz_worker_think_symmetry_stats")
    assert "mz_worker_think_stats" in test_capi.declared_symbols() and "mz_worker_think_reuse_stats" in test_capi.declared_symbols(), "the existing read-outs keep their symbols"
    q, r = C.c_longlong(5), C.c_longlong(5)
    assert L.mz_worker_think_symmetry_stats(None, C.byref(q), C.byref(r)) == -1 and b"NULL" in L.mz_last_error()
    assert (q.value, r.value) == (5, 5)
    assert hasattr(mz.Worker, "think_symmetry_stats")


def test_key_loads_as_1_and_8_only(mz):
    for v in ("1", "8"):
        mz.Env(f"env_game=tictactoe:{KEY}={v}").close()
    for v in ("3", "x", "0", "-8", "8.5", "true"):
        with pytest.raises(mz.MzError) as e:
            mz.Env(f"env_game=tictactoe:{KEY}={v}")
        assert KEY in str(e.value), str(e.value)


def test_refusals_that_need_no_device(mz):
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, 82)
    w = mz.generate_weights(d, 1)
    with pytest.raises(mz.MzError) as e:
        mz.ExternalWorker(GO + f":{KEY}=8", d, lambda rows: 0)
    assert KEY in str(e.value) and "external evaluator" in str(e.value), str(e.value)
    with pytest.raises(mz.MzError) as e:
        mz.MatchWorker(GO + f":mz_match_games=2:{KEY}=8", d, w, w)
    assert KEY in str(e.value) and "match" in str(e.value), str(e.value)
    for extra, word in ((":actor_mcts_think_batch_size=4", "mz_manual_step"), (":mz_manual_step=true", "actor_mcts_think_batch_size"),
                        (":mz_manual_step=true:actor_mcts_think_batch_size=1", "actor_mcts_think_batch_size")):
        with pytest.raises(mz.MzError) as e:
            mz.Worker(GO + extra + f":{KEY}=8", d, w)
        assert KEY in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(mz.MzError) as e:
        mz.Worker(GO + THINK + f":{KEY}=3", d, w)
    assert KEY in str(e.value), str(e.value)
    # with the key at 1 or absent the same workers get the answers they always got
    for key in ("", f":{KEY}=1"):
        with pytest.raises(mz.MzError) as e:
            mz.ExternalWorker(GO + ":actor_mcts_think_batch_size=2" + key, d, lambda rows: 0)
        assert KEY not in str(e.value) and "actor_mcts_think_batch_size" in str(e.value)
        with pytest.raises(mz.MzError) as e:
            mz.MatchWorker(GO + ":mz_match_games=2:mz_manual_step=true" + key, d, w, w)
        assert KEY not in str(e.value) and "mz_manual_step" in str(e.value)
