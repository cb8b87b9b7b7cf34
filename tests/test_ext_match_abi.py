"""The C ABI of match play (include/mzgpu.h: mz_worker_create_match, mz_worker_match_stats, mz_match_stats) as far as it can be checked without a GPU: the
symbols, the layout of the struct against the ctypes mirror (sizes and offsets printed by a C program built from the header itself), every refusal that
needs no device, and the loud error where there is no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("games_started", "games_finished", "moves", "filler_games", "a_first", "a_second", "resignations", "steps", "done", "reserved")
TTT = "env_game=tictactoe:actor_num_simulation=4"


def _ttt(mz):
    d = mz.make_desc("tictactoe", 4, 3, 3, 16, 3, 3, 1, 1, 9, vh=16, dv=1)
    return d, mz.generate_weights(d, 1)


def test_symbols_are_exported(mz):
    L = mz.load()
    for name in ("mz_worker_create_match", "mz_worker_match_stats"):
        assert hasattr(L, name), name


def test_struct_layout_equals_the_ctypes_mirror(mz, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mzgpu.h"\nint main(void) {\n    printf("%zu", sizeof(mz_match_stats));\n'
                   + "".join(f'    printf(" %zu", offsetof(mz_match_stats, {f}));\n' for f in FIELDS)
                   + '    printf(" %zu %zu\\n", sizeof(((mz_match_stats*)0)->a_first), sizeof(mz_worker_stats));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])  # the header is C, not only C++
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(mz.MatchStats)] + [getattr(mz.MatchStats, f).offset for f in FIELDS] + [24, C.sizeof(mz.WorkerStats)]  # (no existing struct changed)
    assert got == want
    assert [f for f, _ in mz.MatchStats._fields_] == list(FIELDS)


def test_refusals_that_need_no_device(mz):
    d, w = _ttt(mz)
    for keys, named in (("zero_num_parallel_games=3:mz_match_games=8", "zero_num_parallel_games"), ("zero_num_parallel_games=1:mz_match_games=8", "zero_num_parallel_games"),
                        ("zero_num_parallel_games=0:mz_match_games=8", "zero_num_parallel_games"), ("zero_num_parallel_games=4:mz_match_games=3", "mz_match_games"),
                        ("zero_num_parallel_games=4", "mz_match_games"), ("zero_num_parallel_games=4:mz_match_games=4:mz_manual_step=true", "mz_manual_step"),
                        ("zero_num_parallel_games=4:mz_match_games=4:actor_mcts_think_batch_size=2", "actor_mcts_think_batch_size"),
                        ("zero_num_parallel_games=4:mz_match_games=4:zero_actor_intermediate_sequence_length=4", "zero_actor_intermediate_sequence_length"),
                        ("zero_num_parallel_games=4:mz_match_games=4:mz_match_precision_a=fp8", "mz_match_precision_a"),
                        ("zero_num_parallel_games=4:mz_match_games=4:mz_match_precision_b=f16", "mz_match_precision_b")):
        with pytest.raises(mz.MzError) as e:
            mz.MatchWorker(TTT + ":" + keys, d, w, w)
        assert named in str(e.value) and "match" in str(e.value), str(e.value)
    with pytest.raises(mz.MzError, match="env_game=atari.*match"):
        mz.MatchWorker("env_game=atari:zero_num_parallel_games=2:mz_match_games=2", d, w, w)
    with pytest.raises(mz.MzError, match="Invalid key"):
        mz.MatchWorker(TTT + ":zero_num_parallel_games=2:mz_match_gamez=2", d, w, w)
    L = mz.load()
    assert not L.mz_worker_create_match(0, TTT.encode(), C.byref(d), None, 0, None, 0) and b"NULL" in L.mz_last_error()
    assert L.mz_worker_match_stats(None, None) == -1


def test_the_five_keys_load_into_every_configuration(mz):
    """a plain worker's configuration may carry them (they are read by a match only): the parser knows them, with their types"""
    e = mz.Env("env_game=tictactoe:mz_match_games=7:mz_match_name_a=old:mz_match_name_b=new:mz_match_precision_a=f32:mz_match_precision_b=bf16x3")
    e.close()
    with pytest.raises(mz.MzError):
        mz.Env("env_game=tictactoe:mz_match_games=seven")


def test_no_gpu_is_an_error_not_a_crash(mz):
    if mz.device_count() > 0:
        pytest.skip("GPU present")
    d, w = _ttt(mz)
    with pytest.raises(mz.MzError, match="no such GPU"):
        mz.MatchWorker(TTT + ":zero_num_parallel_games=4:mz_match_games=4", d, w, w)
    with pytest.raises(mz.MzError, match="no such GPU"):
        mz.MatchWorker(TTT + ":zero_num_parallel_games=4:mz_match_games=4", d, w, w, device=3)
