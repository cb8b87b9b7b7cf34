"""The C ABI of the external evaluator (include/mzgpu.h: mz_evaluator, mz_worker_create_external) as far as it can be checked without a GPU: the symbols, the
layout of the struct against the ctypes mirror (sizes and offsets printed by a C program built from the header itself), the refusals that need no device, and
the loud error where there is no GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("forward", "user", "features", "policy", "logits", "value", "feature_dtype", "output_dtype")
GO = "env_game=go:env_board_size=9:actor_num_simulation=4:zero_num_parallel_games=2"


def test_symbols_are_exported(mz):
    L = mz.load()
    for name in ("mz_worker_create_external", "mz_worker_evaluator_buffers", "mz_worker_evaluator_lane_policy"):
        assert hasattr(L, name), name
    assert mz.DTYPES == {"f32": 0, "f16": 1, "bf16": 2}


def test_struct_layout_equals_the_ctypes_mirror(mz, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mzgpu.h"\nint main(void) {\n    printf("%zu", sizeof(mz_evaluator));\n'
                   + "".join(f'    printf(" %zu", offsetof(mz_evaluator, {f}));\n' for f in FIELDS)
                   + '    printf(" %d %d %d\\n", MZ_F32, MZ_F16, MZ_BF16);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])  # the header is C, not only C++
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(mz.Evaluator)] + [getattr(mz.Evaluator, f).offset for f in FIELDS] + [mz.DTYPES["f32"], mz.DTYPES["f16"], mz.DTYPES["bf16"]]
    assert got == want
    assert [f for f, _ in mz.Evaluator._fields_] == list(FIELDS)


def test_package_import_does_not_import_torch():
    out = subprocess.check_output([sys.executable, "-c", "import sys; import minizero_amd; print('torch' in sys.modules)"], cwd=ROOT)
    assert out.strip() == b"False"


def test_refusals_that_need_no_device(mz):
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, 82)
    for extra, key in ((":mz_device_env=false", "mz_device_env"), (":mz_pipeline_lanes=2", "mz_pipeline_lanes"), (":nn_type_name=muzero", "nn_type_name"),
                       (":actor_mcts_think_batch_size=2", "actor_mcts_think_batch_size"), (":mz_nn_precision=bf16x3", "mz_nn_precision"),
                       (":zero_num_parallel_games=1041", "zero_num_parallel_games")):
        with pytest.raises(mz.MzError) as e:
            mz.ExternalWorker(GO + extra, d, lambda rows: 0)
        assert key in str(e.value) and "external evaluator" in str(e.value), str(e.value)
    with pytest.raises(mz.MzError, match="env_game=atari.*external evaluator"):
        mz.ExternalWorker("env_game=atari:zero_num_parallel_games=2", d, lambda rows: 0)
    d.type = 1
    with pytest.raises(mz.MzError, match=r"desc\.type=1.*external evaluator"):
        mz.ExternalWorker(GO, d, lambda rows: 0)


def test_no_gpu_is_an_error_not_a_crash(mz):
    if mz.device_count() > 0:
        pytest.skip("GPU present")
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, 82)
    with pytest.raises(mz.MzError, match="no such GPU"):
        mz.ExternalWorker(GO, d, lambda rows: 0)
    with pytest.raises(mz.MzError, match="no such GPU"):
        mz.ExternalWorker(GO, d, lambda rows: 0, device=3)
