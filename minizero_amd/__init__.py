"""minizero_amd — MI355X-native self-play worker for MiniZero (host-side Python mirror of the C ABI).

The product is libmzgpu.so (hand-written HIP for gfx950, built in-tree by `__graft_entry__.build()`).
This package only binds include/mzgpu.h with ctypes; there is no Python or CPU fallback: every entry
point raises MzError when the HIP library is missing or no GPU is visible.
"""
from .lib import (MzError, NetDesc, SearchCfg, WorkerStats, Net, Pool, Worker, ExternalWorker, MatchWorker, MatchStats, match_elo, TorchEvaluator, Evaluator, Env, DataLoader, load, lib_path, make_desc,  # noqa: F401
                  param_count, generate_weights, device_count, usable_cpus, godev_playout, envdev_playout, envdev_playout_conf, sort_candidates, invert_values_device, exp_tanh_device, tail_towers, tail_tower_tile, read_pt, read_weight_file, read_weights_once, weight_file_reads, last_error, DESCS, CONFIGS, DTYPES, MZ_HOST, MZ_DEVICE)
