"""ctypes binding of include/mzgpu.h (the C-ABI drop-in boundary)."""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MZ_HOST, MZ_DEVICE = 0, 1


class MzError(RuntimeError):
    pass


def lib_path():
    # MZ_LIBMZGPU: another build of the same library (tools/gpu_sanitize.sh: the host objects under AddressSanitizer / ThreadSanitizer); never a fallback
    return os.environ.get("MZ_LIBMZGPU") or os.path.join(_HERE, "libmzgpu.so")


class NetDesc(C.Structure):
    _fields_ = [("game_name", C.c_char * 64),
                ("num_input_channels", C.c_int), ("input_channel_height", C.c_int), ("input_channel_width", C.c_int),
                ("num_hidden_channels", C.c_int), ("hidden_channel_height", C.c_int), ("hidden_channel_width", C.c_int),
                ("num_action_feature_channels", C.c_int), ("num_blocks", C.c_int), ("action_size", C.c_int),
                ("num_value_hidden_channels", C.c_int), ("discrete_value_size", C.c_int), ("type", C.c_int)]


class SearchCfg(C.Structure):
    _fields_ = [("num_simulation", C.c_int), ("puct_base", C.c_float), ("puct_init", C.c_float), ("reward_discount", C.c_float),
                ("value_rescale", C.c_int), ("flipping_player", C.c_int), ("atari_init_q", C.c_int)]


class WorkerStats(C.Structure):
    _fields_ = [("cycles", C.c_uint64), ("leaf_evals", C.c_uint64), ("moves", C.c_uint64), ("games", C.c_uint64),
                ("ms_select", C.c_double), ("ms_env", C.c_double), ("ms_forward", C.c_double), ("ms_expand", C.c_double),
                ("ms_move", C.c_double), ("ms_total", C.c_double), ("sim_launches", C.c_uint64), ("sim_cycles", C.c_uint64),
                ("pre_evals", C.c_uint64), ("pre_hits", C.c_uint64), ("pre_alt_hits", C.c_uint64), ("pre_launches", C.c_uint64),
                ("pre_batch_launches", C.c_uint64), ("pre_pair_launches", C.c_uint64)]


EVAL_FORWARD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)


class MatchStats(C.Structure):
    """mz_match_stats (include/mzgpu.h)"""
    _fields_ = [("games_started", C.c_uint64), ("games_finished", C.c_uint64), ("moves", C.c_uint64), ("filler_games", C.c_uint64),
                ("a_first", C.c_uint64 * 3), ("a_second", C.c_uint64 * 3), ("resignations", C.c_uint64), ("steps", C.c_uint64),
                ("done", C.c_int32), ("reserved", C.c_int32)]


class Evaluator(C.Structure):
    """mz_evaluator (include/mzgpu.h): the caller's network as the worker sees it"""
    _fields_ = [("forward", EVAL_FORWARD), ("user", C.c_void_p), ("features", C.c_void_p), ("policy", C.c_void_p), ("logits", C.c_void_p),
                ("value", C.c_void_p), ("feature_dtype", C.c_int), ("output_dtype", C.c_int)]


DTYPES = {"f32": 0, "f16": 1, "bf16": 2}  # MZ_F32, MZ_F16, MZ_BF16
NET_TYPES = {"alphazero": 0, "muzero": 1, "muzero_atari": 2}


def make_desc(game, cin, h, w, ch, hh, hw, ac, blocks, actions, vh=256, dv=1, type_name="alphazero"):
    """Same argument order as the reference's create_network (network/py/create_network.py:6-18)."""
    d = NetDesc()
    d.game_name = game.encode()
    (d.num_input_channels, d.input_channel_height, d.input_channel_width) = (cin, h, w)
    (d.num_hidden_channels, d.hidden_channel_height, d.hidden_channel_width) = (ch, hh, hw)
    (d.num_action_feature_channels, d.num_blocks, d.action_size) = (ac, blocks, actions)
    (d.num_value_hidden_channels, d.discrete_value_size, d.type) = (vh, dv, NET_TYPES[type_name])
    return d


# BASELINE.json configs: network shapes and search configuration strings
DESCS = {
    "c1": lambda: make_desc("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9),
    "c2": lambda: make_desc("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82),
    "c3": lambda: make_desc("othello_8x8", 4, 8, 8, 64, 8, 8, 1, 6, 65),
    "c4": lambda: make_desc("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82, type_name="muzero"),
    "c5": lambda: make_desc("atari_ms_pacman", 32, 96, 96, 64, 6, 6, 18, 6, 18, 256, 601, type_name="muzero_atari"),
    # Havannah at its default edge size 8: the network's board is the 15x15 array (2N - 1), 20 planes, no pass
    "havannah8x64": lambda: make_desc("havannah8x8", 20, 15, 15, 64, 15, 15, 1, 6, 225),
}
CONFIGS = {
    "c1": "env_game=tictactoe:actor_num_simulation=16:zero_num_parallel_games=8:zero_num_threads=1",
    "c2": "env_game=go:env_board_size=9:actor_num_simulation=400:zero_num_parallel_games=256",
    "c3": ("env_game=othello:env_board_size=8:actor_num_simulation=16:actor_use_dirichlet_noise=false:actor_use_gumbel=true:"
           "actor_use_gumbel_noise=true:actor_gumbel_sample_size=16:actor_gumbel_sigma_visit_c=50:actor_gumbel_sigma_scale_c=1:"
           "zero_num_parallel_games=1024"),
    "c4": "env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=50:zero_num_parallel_games=256",
    # per GPU (512 games over 8 GPUs); synthetic Atari-shaped environment (ALE / ROMs are not available)
    "c5": ("env_game=atari:nn_type_name=muzero:actor_num_simulation=50:actor_use_dirichlet_noise=false:actor_use_gumbel=true:"
           "actor_use_gumbel_noise=true:actor_gumbel_sample_size=16:actor_gumbel_sigma_scale_c=0.1:actor_mcts_value_rescale=true:"
           "actor_mcts_reward_discount=0.997:atari_init_q=true:zero_actor_intermediate_sequence_length=200:learner_n_step_return=10:"
           "zero_num_parallel_games=64"),
    "havannah8x64": "env_game=havannah:env_board_size=8:actor_num_simulation=400:zero_num_parallel_games=256",
}


def load():
    """Load libmzgpu.so (fail loudly: the product has no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise MzError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    L = C.CDLL(path)
    fp, ip, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    vp = C.c_void_p
    L.mz_last_error.restype = C.c_char_p
    L.mz_net_param_count.restype = C.c_long
    L.mz_net_param_count.argtypes = [C.POINTER(NetDesc)]
    L.mz_net_generate_weights.argtypes = [C.POINTER(NetDesc), C.c_uint64, fp]
    L.mz_net_read_pt.argtypes = [C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mz_net_create.restype = vp
    L.mz_net_create.argtypes = [C.c_int, C.POINTER(NetDesc), fp, C.c_size_t]
    L.mz_net_reload.argtypes = [vp, fp, C.c_size_t]
    L.mz_net_destroy.argtypes = [vp]
    L.mz_net_get_desc.argtypes = [vp, C.POINTER(NetDesc)]
    L.mz_net_set_precision.argtypes = [vp, C.c_int]
    L.mz_net_forward_az.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int]
    L.mz_net_tower_az.argtypes = [vp, vp, C.c_int, vp]
    L.mz_net_initial.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int]
    L.mz_net_recurrent.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int]
    L.mz_net_time_forward.argtypes = [vp, C.c_int, C.c_int, fp, fp, C.POINTER(C.c_double)]
    L.mz_net_time_tower_conv.argtypes = [vp, C.c_int, C.c_int, fp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mz_pool_create.restype = vp
    L.mz_pool_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SearchCfg)]
    L.mz_pool_destroy.argtypes = [vp]
    L.mz_pool_reset_search.argtypes = [vp, u8p, ip]
    L.mz_pool_select.argtypes = [vp, ip, ip, ip, ip]
    L.mz_pool_max_depth.argtypes = [vp]
    L.mz_pool_expand_backup.argtypes = [vp, ip, ip, fp, fp, ip, fp, fp]
    L.mz_pool_root_set_noise.argtypes = [vp, u8p, fp, fp, fp]
    L.mz_pool_root_read.argtypes = [vp, ip, ip] + [fp] * 12 + [ip]
    L.mz_pool_read_nodes.argtypes = [vp, C.c_int, C.c_int, ip, ip, ip, ip] + [fp] * 7
    L.mz_pool_num_nodes.argtypes = [vp, C.c_int]
    if hasattr(L, "mz_worker_create"):
        L.mz_worker_create.restype = vp
        L.mz_worker_create.argtypes = [C.c_int, C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t]
        L.mz_worker_destroy.argtypes = [vp]
        L.mz_worker_command.argtypes = [vp, C.c_char_p]
        L.mz_worker_set_weights.argtypes = [vp, fp, C.c_size_t]
        L.mz_worker_load_model.argtypes = [vp, C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t]
        L.mz_weights_read.restype = vp
        L.mz_weights_read.argtypes = [C.c_char_p]
        L.mz_weights_desc.restype = C.POINTER(NetDesc)
        L.mz_weights_desc.argtypes = [vp]
        L.mz_weights_data.restype = fp
        L.mz_weights_data.argtypes = [vp]
        L.mz_weights_count.restype = C.c_size_t
        L.mz_weights_count.argtypes = [vp]
        L.mz_weights_free.argtypes = [vp]
        L.mz_weight_file_reads.restype = C.c_uint64
        L.mz_worker_run_cycles.argtypes = [vp, C.c_int]
        L.mz_worker_cycles_per_move.argtypes = [vp]
        L.mz_worker_lanes.argtypes = [vp]
        L.mz_net_read_weight_file.argtypes = [C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mz_worker_pop_line.argtypes = [vp, C.c_char_p, C.c_int]
        L.mz_worker_wait_lines.argtypes = [vp]
        L.mz_worker_get_stats.argtypes = [vp, C.POINTER(WorkerStats)]
        if hasattr(L, "mz_worker_think_stats"):  # (MZ_LIBMZGPU may name a build from before the batched think: tools/think_bench.py measures one)
            u64p = C.POINTER(C.c_uint64)
            L.mz_worker_think_stats.argtypes = [vp, u64p, u64p, u64p]
        if hasattr(L, "mz_worker_reset_game"):  # (per-actor stepping: likewise absent from a build that MZ_LIBMZGPU may name)
            L.mz_worker_reset_game.argtypes = [vp, C.c_int]
            L.mz_worker_env_query.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        if hasattr(L, "mz_worker_think_reuse_stats"):  # (likewise: a build from before mz_think_reuse_tree)
            L.mz_worker_think_reuse_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
        if hasattr(L, "mz_worker_think_symmetry_stats"):  # (likewise: a build from before mz_think_symmetries)
            L.mz_worker_think_symmetry_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.mz_worker_search_done.argtypes = [vp]
        L.mz_worker_search_action.argtypes = [vp, C.c_int, ip, ip, ip]
        L.mz_worker_act.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.mz_worker_reset_search.argtypes = [vp]
        L.mz_worker_finish_search.argtypes = [vp]
        L.mz_worker_peek_record.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        if hasattr(L, "mz_worker_tree"):  # (MZ_LIBMZGPU may name a build from before the tree read-out: an A/B run of bench.py measures one)
            L.mz_worker_tree_size.argtypes = [vp, C.c_int]
            L.mz_worker_tree.argtypes = [vp, C.c_int, C.c_int] + [ip] * 6 + [fp] * 7
            L.mz_worker_tree_string.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
            L.mz_worker_node_info.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.mz_worker_net.restype = vp
        L.mz_worker_net.argtypes = [vp]
        L.mz_env_create.restype = vp
        L.mz_env_create.argtypes = [C.c_char_p]
        L.mz_env_destroy.argtypes = [vp]
        L.mz_env_reset.argtypes = [vp]
        L.mz_env_reset_seed.argtypes = [vp, C.c_int]
        L.mz_env_reward.restype = C.c_float
        L.mz_env_reward.argtypes = [vp]
        L.mz_env_act.argtypes = [vp, C.c_int, C.c_int]
        for n in ("mz_env_turn", "mz_env_is_terminal", "mz_env_policy_size", "mz_env_feature_size"):
            getattr(L, n).argtypes = [vp]
        L.mz_env_eval_score.restype = C.c_float
        L.mz_env_eval_score.argtypes = [vp, C.c_int]
        L.mz_env_legal_mask.argtypes = [vp, u8p]
        L.mz_env_features.argtypes = [vp, C.c_int, fp]
        L.mz_env_feature_bits.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32)]
        L.mz_env_action_from_string.argtypes = [vp, C.c_char_p]
        L.mz_env_name.argtypes = [vp, C.c_char_p, C.c_int]
        L.mz_worker_create_shared.restype = vp
        L.mz_worker_create_shared.argtypes = [C.c_int, C.c_char_p, vp]
        if hasattr(L, "mz_worker_create_external"):  # (MZ_LIBMZGPU may name a build from before the external evaluator)
            L.mz_worker_create_external.restype = vp
            L.mz_worker_create_external.argtypes = [C.c_int, C.c_char_p, C.POINTER(NetDesc), C.POINTER(Evaluator)]
            L.mz_worker_evaluator_buffers.argtypes = [vp] + [C.POINTER(vp)] * 4
            L.mz_worker_evaluator_lane_policy.argtypes = [vp, fp, C.c_int]
        if hasattr(L, "mz_worker_create_match"):  # (MZ_LIBMZGPU may name a build from before match play)
            L.mz_worker_create_match.restype = vp
            L.mz_worker_create_match.argtypes = [C.c_int, C.c_char_p, C.POINTER(NetDesc), fp, C.c_size_t, fp, C.c_size_t]
            L.mz_worker_match_stats.argtypes = [vp, C.POINTER(MatchStats)]
        L.mz_godev_playout.argtypes = [C.c_int, C.c_int, C.c_float, ip, C.c_int, C.c_int, ip, C.POINTER(C.c_uint32), u8p, ip, fp, ip]
        L.mz_envdev_playout.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_float, ip, C.c_int, C.c_int, ip, C.POINTER(C.c_uint32), u8p, ip, fp, ip]
        L.mz_envdev_playout_conf.argtypes = [C.c_int, C.c_char_p, ip, C.c_int, C.c_int, ip, C.POINTER(C.c_uint32), u8p, ip, fp, ip]
        L.mz_sort_candidates.argtypes = [C.c_int, fp, C.c_int, ip]
        L.mz_invert_values_device.argtypes = [C.c_int, fp, C.c_int, fp]
        L.mz_exp_tanh_device.argtypes = [C.c_int, fp, C.c_int, fp, fp]
    L.mz_loader_create.restype = vp
    L.mz_loader_create.argtypes = [C.c_int, C.c_char_p]
    L.mz_loader_destroy.argtypes = [vp]
    L.mz_loader_load_data_from_file.argtypes = [vp, C.c_char_p]
    L.mz_loader_add_record.argtypes = [vp, C.c_char_p]
    L.mz_loader_sample_data.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    L.mz_loader_update_priority.argtypes = [vp, vp, vp]
    for n in ("mz_loader_num_data", "mz_loader_num_games"):
        getattr(L, n).argtypes = [vp]
    L.mz_loader_shape.argtypes = [vp, C.c_int]
    for n in ("mz_invert_value", "mz_transform_value"):
        getattr(L, n).restype = C.c_float
        getattr(L, n).argtypes = [C.c_float]
    _LIB = L
    return L


def _err(L):
    return (L.mz_last_error() or b"").decode(errors="replace")


def last_error():
    """the text of the calling thread's last libmzgpu error (mz_last_error): why a call returned an error code, or why add_record skipped a record"""
    return _err(load())


def _check(L, rc):
    if rc < 0:
        raise MzError(f"libmzgpu error {rc}: {_err(L)}")
    return rc


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def device_count():
    return load().mz_device_count()


def usable_cpus():
    return load().mz_usable_cpus()


def read_pt(path):
    """(desc, weights) of a TorchScript file written by the reference's trainer — native parser, no torch."""
    L = load()
    d = NetDesc()
    n = C.c_size_t(0)
    _check(L, L.mz_net_read_pt(path.encode(), C.byref(d), None, 0, C.byref(n)))
    w = np.empty(n.value, np.float32)
    _check(L, L.mz_net_read_pt(path.encode(), C.byref(d), _f(w), n.value, C.byref(n)))
    return d, w


def read_weight_file(path):
    """(desc, weights) of `path` as Network::loadModel is given it: the TorchScript archive, or for a missing x.pt its sibling x.mzw."""
    L = load()
    d = NetDesc()
    n = C.c_size_t(0)
    _check(L, L.mz_net_read_weight_file(path.encode(), C.byref(d), None, 0, C.byref(n)))
    w = np.empty(n.value, np.float32)
    _check(L, L.mz_net_read_weight_file(path.encode(), C.byref(d), _f(w), n.value, C.byref(n)))
    return d, w


def weight_file_reads():
    """weight files this process has opened and parsed through libmzgpu so far"""
    return int(load().mz_weight_file_reads())


def read_weights_once(path):
    """mz_weights_read: (desc, blob) from ONE open + parse of `path` (.pt, or its .mzw sibling)"""
    L = load()
    h = L.mz_weights_read(path.encode())
    if not h:
        raise MzError("mz_weights_read failed: " + _err(L))
    try:
        d = NetDesc.from_buffer_copy(L.mz_weights_desc(h).contents)
        n = L.mz_weights_count(h)
        w = np.ctypeslib.as_array(L.mz_weights_data(h), shape=(n,)).copy()
    finally:
        L.mz_weights_free(h)
    return d, w


def param_count(desc):
    return _check(load(), load().mz_net_param_count(C.byref(desc)))


def generate_weights(desc, seed=0):
    L = load()
    w = np.empty(param_count(desc), np.float32)
    _check(L, L.mz_net_generate_weights(C.byref(desc), seed, _f(w)))
    return w


class Net:
    """Mirror of minizero::network::{AlphaZeroNetwork,MuZeroNetwork} (ref network/alphazero_network.h, muzero_network.h)."""

    def __init__(self, desc, weights, device=0, handle=None):
        self.L = load()
        self.desc = desc
        self._own = handle is None
        if handle is None:
            w = np.ascontiguousarray(weights, np.float32)
            handle = self.L.mz_net_create(device, C.byref(desc), _f(w), w.size)
            if not handle:
                raise MzError("mz_net_create failed: " + _err(self.L))
        self.h = handle

    def close(self):
        if getattr(self, "h", None) and self._own:
            self.L.mz_net_destroy(self.h)
        self.h = None

    __del__ = close

    def reload(self, weights):
        w = np.ascontiguousarray(weights, np.float32)
        _check(self.L, self.L.mz_net_reload(self.h, _f(w), w.size))

    def set_precision(self, name):
        """'f32' (default) or 'bf16x3' (opt-in split-bf16 tower, outputs within 1e-3 of f32)"""
        _check(self.L, self.L.mz_net_set_precision(self.h, {"f32": 0, "bf16x3": 1}[name]))

    def hidden_size(self):
        d = self.desc
        return d.num_hidden_channels * d.hidden_channel_height * d.hidden_channel_width

    def forward(self, features):
        x = np.ascontiguousarray(features, np.float32)
        B, A = x.shape[0], self.desc.action_size
        p, l, v = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        _check(self.L, self.L.mz_net_forward_az(self.h, x.ctypes.data, B, p.ctypes.data, l.ctypes.data, v.ctypes.data, MZ_HOST))
        return p, l, v

    def tower(self, features):
        """the representation tower alone, at the current precision: the activations the heads read, [B][C][h * w]"""
        x = np.ascontiguousarray(features, np.float32)
        d = self.desc
        out = np.empty((x.shape[0], d.num_hidden_channels, d.hidden_channel_height * d.hidden_channel_width), np.float32)
        _check(self.L, self.L.mz_net_tower_az(self.h, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def initial_inference(self, features):
        x = np.ascontiguousarray(features, np.float32)
        B, A = x.shape[0], self.desc.action_size
        p, l, v = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        h = np.empty((B, self.hidden_size()), np.float32)
        _check(self.L, self.L.mz_net_initial(self.h, x.ctypes.data, B, p.ctypes.data, l.ctypes.data, v.ctypes.data, h.ctypes.data, MZ_HOST))
        return p, l, v, h

    def recurrent_inference(self, hidden, action_plane):
        hin = np.ascontiguousarray(hidden, np.float32)
        act = np.ascontiguousarray(action_plane, np.float32)
        B, A = hin.shape[0], self.desc.action_size
        p, l, v = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        r, h = np.empty(B, np.float32), np.empty((B, self.hidden_size()), np.float32)
        _check(self.L, self.L.mz_net_recurrent(self.h, hin.ctypes.data, act.ctypes.data, B, p.ctypes.data, l.ctypes.data, v.ctypes.data,
                                               r.ctypes.data, h.ctypes.data, MZ_HOST))
        return p, l, v, r, h

    def time_forward(self, batch, iters):
        t, c, fl = C.c_float(), C.c_float(), C.c_double()
        _check(self.L, self.L.mz_net_time_forward(self.h, batch, iters, C.byref(t), C.byref(c), C.byref(fl)))
        return t.value, c.value, fl.value


    def time_tower_conv(self, batch, iters):
        t, fl, by = C.c_float(), C.c_double(), C.c_double()
        _check(self.L, self.L.mz_net_time_tower_conv(self.h, batch, iters, C.byref(t), C.byref(fl), C.byref(by)))
        return t.value, fl.value, by.value


class Pool:
    """Mirror of minizero::actor::MCTS for `games` trees at once (ref actor/mcts.h:75-119)."""

    def __init__(self, games, nodes_per_game, action_size, num_simulation, puct_base=19652.0, puct_init=1.25, reward_discount=1.0,
                 value_rescale=False, flipping_player=2, atari_init_q=False, device=0):
        self.L = load()
        self.games, self.A = games, action_size
        cfg = SearchCfg(num_simulation, puct_base, puct_init, reward_discount, int(value_rescale), flipping_player, int(atari_init_q))
        self.h = self.L.mz_pool_create(device, games, nodes_per_game, action_size, C.byref(cfg))
        if not self.h:
            raise MzError("mz_pool_create failed: " + _err(self.L))
        self.max_depth = self.L.mz_pool_max_depth(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.mz_pool_destroy(self.h)
        self.h = None

    __del__ = close

    def reset_search(self, root_player, mask=None):
        rp = np.ascontiguousarray(root_player, np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        _check(self.L, self.L.mz_pool_reset_search(self.h, m, _i(rp)))

    def select(self, start_node=None):
        G = self.games
        pl = np.empty(G, np.int32)
        paths = np.empty((G, self.max_depth), np.int32)
        acts = np.empty((G, self.max_depth), np.int32)
        st = None if start_node is None else _i(np.ascontiguousarray(start_node, np.int32))
        _check(self.L, self.L.mz_pool_select(self.h, st, _i(pl), _i(paths), _i(acts)))
        return pl, paths, acts

    def expand_backup(self, cand_count, cand_action, cand_policy, cand_logit, cand_player, value, reward=None):
        cc = np.ascontiguousarray(cand_count, np.int32)
        ca = np.ascontiguousarray(cand_action, np.int32)
        cp = np.ascontiguousarray(cand_policy, np.float32)
        cl = np.ascontiguousarray(cand_logit, np.float32)
        pl = np.ascontiguousarray(cand_player, np.int32)
        v = np.ascontiguousarray(value, np.float32)
        r = np.zeros(self.games, np.float32) if reward is None else np.ascontiguousarray(reward, np.float32)
        assert ca.size == self.games * self.A
        _check(self.L, self.L.mz_pool_expand_backup(self.h, _i(cc), _i(ca), _f(cp), _f(cl), _i(pl), _f(v), _f(r)))

    def root_set_noise(self, policy, logit, noise, mask=None):
        p = np.ascontiguousarray(policy, np.float32)
        l = np.ascontiguousarray(logit, np.float32)
        n = np.ascontiguousarray(noise, np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        _check(self.L, self.L.mz_pool_root_set_noise(self.h, m, _f(p), _f(l), _f(n)))

    def root_read(self):
        G, A = self.games, self.A
        nc, act, bs = np.empty(G, np.int32), np.empty((G, A), np.int32), np.empty(G, np.int32)
        fa = [np.empty((G, A), np.float32) for _ in range(7)]
        fg = [np.empty(G, np.float32) for _ in range(5)]
        _check(self.L, self.L.mz_pool_root_read(self.h, _i(nc), _i(act), *[_f(x) for x in fa], *[_f(x) for x in fg], _i(bs)))
        keys = ["count", "mean", "policy", "logit", "noise", "value", "reward"]
        out = dict(zip(keys, fa))
        out.update(num_children=nc, action=act, bound_size=bs, root_count=fg[0], root_mean=fg[1], root_value=fg[2], bound_lo=fg[3], bound_hi=fg[4])
        return out

    def num_nodes(self, game):
        return _check(self.L, self.L.mz_pool_num_nodes(self.h, game))

    def read_nodes(self, game, n=None):
        n = self.num_nodes(game) if n is None else n
        ints = [np.empty(n, np.int32) for _ in range(4)]
        fl = [np.empty(n, np.float32) for _ in range(7)]
        _check(self.L, self.L.mz_pool_read_nodes(self.h, game, n, *[_i(x) for x in ints], *[_f(x) for x in fl]))
        keys = ["action", "player", "num_children", "first_child", "mean", "count", "policy", "logit", "noise", "value", "reward"]
        return dict(zip(keys, ints + fl))


class Worker:
    """Mirror of minizero::actor::ActorGroup (`-mode sp`, ref actor/actor_group.cpp:136-252)."""

    def __init__(self, conf, desc=None, weights=None, device=0, shared=None):
        """desc / weights None: the network is read from the configuration's nn_file_name (.pt, or its .mzw sibling);
        shared: a Net the worker runs ON instead of loading its own copy (BaseActor::setNetwork, mz_worker_create_shared)"""
        self.L = load()
        self.shared = shared  # keeps the caller's network alive
        if shared is not None:
            self.h = self.L.mz_worker_create_shared(device, conf.encode(), shared.h)
            desc = shared.desc
        elif desc is None:
            self.h = self.L.mz_worker_create(device, conf.encode(), None, None, 0)
        else:
            w = np.ascontiguousarray(weights, np.float32)
            self.h = self.L.mz_worker_create(device, conf.encode(), C.byref(desc), _f(w), w.size)
        if not self.h:
            raise MzError("mz_worker_create failed: " + _err(self.L))
        if desc is None:
            desc = NetDesc()
            _check(self.L, self.L.mz_net_get_desc(self.L.mz_worker_net(self.h), C.byref(desc)))
        self.desc = desc

    def close(self):
        if getattr(self, "h", None):
            self.L.mz_worker_destroy(self.h)
        self.h = None

    __del__ = close

    def command(self, line):
        return _check(self.L, self.L.mz_worker_command(self.h, line.encode()))

    def set_weights(self, weights):
        w = np.ascontiguousarray(weights, np.float32)
        _check(self.L, self.L.mz_worker_set_weights(self.h, _f(w), w.size))

    def load_model(self, path, desc, weights):
        """`load_model <path>` for a caller that has read the file already (one read for all devices: mz_weights_read)"""
        w = np.ascontiguousarray(weights, np.float32)
        return _check(self.L, self.L.mz_worker_load_model(self.h, path.encode(), C.byref(desc), _f(w), w.size))

    def run_cycles(self, n):
        return _check(self.L, self.L.mz_worker_run_cycles(self.h, n))

    def cycles_per_move(self):
        return _check(self.L, self.L.mz_worker_cycles_per_move(self.h))

    def lanes(self):
        return _check(self.L, self.L.mz_worker_lanes(self.h))

    def pop_lines(self, wait=True):
        """Every finished record.  wait=False: only those that are complete right now (mz_worker_pop_line never blocks: an Atari record whose OBS tag
        is still being compressed, and everything behind it, stays queued) — what a driver does between two moves."""
        if wait:
            _check(self.L, self.L.mz_worker_wait_lines(self.h))
        out = []
        buf = C.create_string_buffer(1 << 20)
        while True:
            need = _check(self.L, self.L.mz_worker_pop_line(self.h, None, 0))  # size query: Atari records carry megabytes of OBS hex
            if need == 0:
                break
            if need >= len(buf):
                buf = C.create_string_buffer(need + 1)
            _check(self.L, self.L.mz_worker_pop_line(self.h, buf, len(buf)))
            out.append(buf.value.decode())
        return out

    def peek_records(self, games):
        """Records of games 0..games-1 as they stand (unfinished ones included)."""
        buf = C.create_string_buffer(1 << 20)
        out = []
        for g in range(games):
            need = _check(self.L, self.L.mz_worker_peek_record(self.h, g, None, 0))
            if need >= len(buf):
                buf = C.create_string_buffer(need + 1)
            _check(self.L, self.L.mz_worker_peek_record(self.h, g, buf, len(buf)))
            out.append(buf.value.decode())
        return out

    def stats(self):
        s = WorkerStats()
        _check(self.L, self.L.mz_worker_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in WorkerStats._fields_}

    def think_stats(self):
        """(steps, walks, queries) of the batched think (actor_mcts_think_batch_size > 1 under mz_manual_step), summed over the games; zeros otherwise"""
        s, w, q = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(self.L, self.L.mz_worker_think_stats(self.h, C.byref(s), C.byref(w), C.byref(q)))
        return s.value, w.value, q.value

    def think_reuse_stats(self):
        """(reroots, kept, kept_visits) of mz_think_reuse_tree=true: the moves mz_worker_act handed to the re-root, those that kept a subtree for the next
        search, and the sum of the kept roots' visits — the simulations the next searches did not have to run; zeros with the key off"""
        r, k, v = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(self.L, self.L.mz_worker_think_reuse_stats(self.h, C.byref(r), C.byref(k), C.byref(v)))
        return r.value, k.value, v.value

    def think_symmetry_stats(self):
        """(queries, rows) of the batched think: the leaves evaluated and the network rows computed for them — 8 per query with mz_think_symmetries=8, 1 per
        query otherwise; zeros where the batched think does not run"""
        q, r = C.c_longlong(), C.c_longlong()
        _check(self.L, self.L.mz_worker_think_symmetry_stats(self.h, C.byref(q), C.byref(r)))
        return q.value, r.value

    def search_done(self):
        return _check(self.L, self.L.mz_worker_search_done(self.h)) == 1

    def search_action(self, game):
        """(action id, player, resigns?) of the completed search of a game (mz_manual_step)"""
        a, p, r = C.c_int(), C.c_int(), C.c_int()
        _check(self.L, self.L.mz_worker_search_action(self.h, game, C.byref(a), C.byref(p), C.byref(r)))
        return a.value, p.value, bool(r.value)

    def act(self, game, action, player):
        return _check(self.L, self.L.mz_worker_act(self.h, game, action, player)) == 1

    def reset_search(self):
        _check(self.L, self.L.mz_worker_reset_search(self.h))

    def reset_game(self, game):
        """ZeroActor::reset() of one game without the search part (mz_worker_reset_game; mz_manual_step): a new game and its resign coin"""
        _check(self.L, self.L.mz_worker_reset_game(self.h, game))

    def env_query(self, game, what):
        """mz_worker_env_query: what = 0 isTerminal, 1 getTurn, 2 getEvalScore(false), 3 getEvalScore(true), 4 number of actions played, 5 getReward"""
        out = C.c_float()
        _check(self.L, self.L.mz_worker_env_query(self.h, game, what, C.byref(out)))
        return out.value

    def tree_size(self, game):
        """the number of entries mz_worker_tree gives for the game (its visited nodes)"""
        return _check(self.L, self.L.mz_worker_tree_size(self.h, game))

    def finish_search(self):
        _check(self.L, self.L.mz_worker_finish_search(self.h))

    TREE_INTS = ("parent", "ordinal", "action", "player", "num_children", "depth")
    TREE_FLOATS = ("count", "mean", "policy", "logit", "noise", "value", "reward")

    def tree(self, game):
        """The visited tree of a game as the pool holds it (mz_worker_tree; mz_manual_step): a dict of numpy arrays, one entry per node with
        count > 0 plus the root (entry 0), breadth-first, the children of one parent contiguous and in child order.  `parent` is an entry
        index (-1 for the root), `ordinal` the index among the parent's children; unvisited children are not read back."""
        cap = self.cycles_per_move() + 1  # n + 2 entries hold every tree of n + 1 simulations: one read-out, no size query first
        out = {k: np.zeros(cap, np.int32) for k in self.TREE_INTS}
        out.update({k: np.zeros(cap, np.float32) for k in self.TREE_FLOATS})
        n = _check(self.L, self.L.mz_worker_tree(self.h, game, cap, *[_i(out[k]) for k in self.TREE_INTS], *[_f(out[k]) for k in self.TREE_FLOATS]))
        return {k: v[:n].copy() for k, v in out.items()}

    def _string(self, call, *args):
        need = _check(self.L, call(self.h, *args, None, 0))
        buf = C.create_string_buffer(need + 1)
        _check(self.L, call(self.h, *args, buf, len(buf)))
        return buf.value.decode()

    def tree_string(self, game):
        """Tree::toString(record of the game) of the reference (mz_worker_tree_string): the SGF of the visited tree"""
        return self._string(self.L.mz_worker_tree_string, game)

    def node_info(self, game, which):
        """MCTSNode::toString() of the root (which = 0) or of the node the decision chose (which = 1, once the search is done)"""
        return self._string(self.L.mz_worker_node_info, game, which)

    def net(self):
        return Net(self.desc, None, handle=self.L.mz_worker_net(self.h))


class MatchWorker(Worker):
    """Two weight blobs of one descriptor against each other (mz_worker_create_match): side A = weights_a, side B = weights_b.  The
    configuration carries mz_match_games (and the names / precisions of the sides); everything else is a Worker — with two differences for code that is
    handed a MatchWorker as a Worker: stats() is the MATCH's tally (mz_match_stats), the counters every worker has are worker_stats(); and net() raises,
    because a match gives out no network handle (mz_worker_net is NULL: its networks are fixed and take turns)."""

    def __init__(self, conf, desc, weights_a, weights_b, device=0):
        self.L = load()
        self.shared = None
        if not hasattr(self.L, "mz_worker_create_match"):
            raise MzError("this libmzgpu build has no mz_worker_create_match")
        wa, wb = np.ascontiguousarray(weights_a, np.float32), np.ascontiguousarray(weights_b, np.float32)
        self.h = self.L.mz_worker_create_match(device, conf.encode(), C.byref(desc), _f(wa), wa.size, _f(wb), wb.size)
        if not self.h:
            raise MzError("mz_worker_create_match failed: " + _err(self.L))
        self.desc = desc

    def net(self):
        raise MzError("MatchWorker: the networks of a match are fixed and take turns; there is no handle to one (mz_worker_net is NULL)")

    def worker_stats(self):
        """the counters every worker has (mz_worker_get_stats)"""
        return Worker.stats(self)

    def stats(self):
        """mz_match_stats as a dictionary; a_first / a_second are side A's [wins, draws, losses] as first and as second player"""
        s = MatchStats()
        _check(self.L, self.L.mz_worker_match_stats(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in MatchStats._fields_ if k != "reserved"}
        out["a_first"], out["a_second"], out["done"] = list(s.a_first), list(s.a_second), bool(s.done)
        return out

    def play(self):
        """runs the match to its end, a move of every game per call -> (stats, the `Match` lines in the order the games finished)"""
        self.command("start")
        lines, k = [], self.cycles_per_move()
        while not self.stats()["done"]:
            self.run_cycles(k)
            lines += self.pop_lines(wait=False)
        return self.stats(), lines + self.pop_lines()


def match_elo(stats):
    """The rating difference A - B a match's tally stands for.  With w, d, l side A's wins, draws and losses over n games, the score is s = (w + d/2) / n and
    elo = 400 log10(s / (1 - s)); the standard error of s comes from the trinomial variance, var = (w (1 - s)^2 + d (1/2 - s)^2 + l s^2) / n per game, and
    goes through the slope of the logistic curve: se_elo = 400 / (ln 10 s (1 - s)) sqrt(var / n).  s = 0 or 1 gives -inf / +inf with an infinite error; no
    games give nan.  Returns the figures for all games and separately for the games A started ("first") and the games B started ("second")."""
    def one(w, d, l):
        n = w + d + l
        if n == 0:
            return dict(games=0, score=math.nan, elo=math.nan, se=math.nan)
        s = (w + 0.5 * d) / n
        if s <= 0.0 or s >= 1.0:
            return dict(games=n, score=s, elo=math.inf if s >= 1.0 else -math.inf, se=math.inf)
        var = (w * (1.0 - s) ** 2 + d * (0.5 - s) ** 2 + l * s ** 2) / n
        return dict(games=n, score=s, elo=400.0 * math.log10(s / (1.0 - s)), se=400.0 / (math.log(10.0) * s * (1.0 - s)) * math.sqrt(var / n))
    f, s = list(stats["a_first"]), list(stats["a_second"])
    out = one(*[a + b for a, b in zip(f, s)])
    out["first"], out["second"] = one(*f), one(*s)
    return out


def _device_ptr(a, what):
    """a device pointer for mz_evaluator: a torch CUDA tensor (data_ptr(), as DataLoader._ptr takes them), a raw address, or None"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        if not (a.is_cuda and a.is_contiguous()):
            raise MzError(f"ExternalWorker: {what} must be a contiguous CUDA tensor")
        return a.data_ptr()
    return int(a)


class ExternalWorker(Worker):
    """A Worker whose network is the caller's code (mz_worker_create_external): every cycle the planes of all games' leaves are written into `features`
    ([games][C][H][W]), `forward(rows)` is called on the calling thread, and it returns (None or 0) when `logits` [games][A], `value` [games] and — unless
    it is None: then the library computes softmax(logits) — `policy` [games][A] are complete.  Buffers are torch CUDA tensors or raw device addresses;
    features=None: the library allocates all four (f32) and buffers() names them.  An exception in `forward` ends the cycle and is raised again from
    run_cycles; a non-zero return makes run_cycles raise MzError (MZ_ERR_STATE).  After either the worker runs no further cycles.
    Only type, the input planes' shape and action_size of `desc` are read."""

    def __init__(self, conf, desc, forward, *, features=None, policy=None, logits=None, value=None, feature_dtype="f32", output_dtype="f32", device=0):
        self.L = load()
        self.shared = None
        self.desc = desc
        self._keep = (features, policy, logits, value)  # the caller's tensors stay alive as long as the worker writes and reads them
        state = self._state = {"exc": None}

        def trampoline(user, rows):  # no exception may cross the C frames above this one
            try:
                rc = forward(rows)
                return 0 if rc is None else int(rc)
            except BaseException as e:  # noqa: B036 — KeyboardInterrupt too: it is raised again from run_cycles
                state["exc"] = e
                return -1

        self._cb = EVAL_FORWARD(trampoline)
        ev = Evaluator(self._cb, None, _device_ptr(features, "features"), _device_ptr(policy, "policy"), _device_ptr(logits, "logits"),
                       _device_ptr(value, "value"), DTYPES[feature_dtype], DTYPES[output_dtype])
        self.h = self.L.mz_worker_create_external(device, conf.encode(), C.byref(desc), C.byref(ev))
        if not self.h:
            raise MzError("mz_worker_create_external failed: " + _err(self.L))

    def run_cycles(self, n):
        rc = self.L.mz_worker_run_cycles(self.h, n)
        exc, self._state["exc"] = self._state["exc"], None
        if exc is not None:
            raise exc  # the exception `forward` raised, its traceback continued here
        return _check(self.L, rc)

    def buffers(self):
        """(features, policy, logits, value): the device addresses in use, library-owned ones included (policy is None where the library computes it)"""
        p = [C.c_void_p() for _ in range(4)]
        _check(self.L, self.L.mz_worker_evaluator_buffers(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def lane_policy(self, games):
        """test access: the worker's own f32 policy [games][A] as the last import left it for the search"""
        out = np.empty((games, self.desc.action_size), np.float32)
        _check(self.L, self.L.mz_worker_evaluator_lane_policy(self.h, _f(out), out.size))
        return out

    def net(self):
        raise MzError("ExternalWorker: the network is the caller's")


class TorchEvaluator:
    """A torch module as an ExternalWorker's network: the tensors of the hand-over and the callable.  `module(features)` — features [games][C][H][W] of
    `dtype` on `device` — returns (policy, logits, value) or (logits, value); which of the two is found by one call on empty planes here, and with
    (logits, value) the library computes the policy.  value is [games] or [games][1], in game scale.  Called under torch.no_grad(); the outputs are copied
    into the hand-over tensors and the current stream is synchronised.  torch is imported here, not with the package."""

    def __init__(self, module, games, C, H, W, A, dtype="f32", device="cuda"):
        import torch
        self.torch, self.module, self.games, self.dtype = torch, module, games, dtype
        td = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
        self.features = torch.zeros((games, C, H, W), dtype=td, device=device)
        self.logits = torch.zeros((games, A), dtype=td, device=device)
        self.value = torch.zeros((games,), dtype=td, device=device)
        with torch.no_grad():
            arity = len(module(self.features))
        if arity not in (2, 3):
            raise MzError(f"TorchEvaluator: the module returns {arity} outputs: (policy, logits, value) or (logits, value) expected")
        self.policy = torch.zeros((games, A), dtype=td, device=device) if arity == 3 else None

    def __call__(self, rows):
        torch = self.torch
        with torch.no_grad():
            out = self.module(self.features)
            if self.policy is not None:
                self.policy.copy_(out[0])
            self.logits.copy_(out[-2])
            self.value.copy_(out[-1].reshape(self.games))
        torch.cuda.current_stream(self.features.device).synchronize()
        return 0

    def worker(self, conf, desc, device=None):
        """the ExternalWorker that searches on this evaluator"""
        dev = self.features.device.index if device is None else device
        return ExternalWorker(conf, desc, self, features=self.features, policy=self.policy, logits=self.logits, value=self.value,
                              feature_dtype=self.dtype, output_dtype=self.dtype, device=dev or 0)


class DataLoader:
    """Mirror of the reference's learner-side `minizero_py.DataLoader` (ref learner/pybind.cpp:62-84, learner/data_loader.h:75-93): same
    method names and argument order.  `conf` is the configuration STRING (the reference takes a .cfg file name; pass its lines joined with
    ':' plus env_game).  Arrays may be numpy arrays (host) or torch CUDA tensors (the batch is then written in place on the device)."""

    def __init__(self, conf, device=0):
        self.L = load()
        self.h = self.L.mz_loader_create(device, conf.encode())
        if not self.h:
            raise MzError("mz_loader_create failed: " + _err(self.L))

    def close(self):
        if getattr(self, "h", None):
            self.L.mz_loader_destroy(self.h)
        self.h = None

    __del__ = close

    def initialize(self):  # ref data_loader.cpp:194-198: thread creation; nothing to do here
        pass

    def load_data_from_file(self, file_name):
        return _check(self.L, self.L.mz_loader_load_data_from_file(self.h, file_name.encode()))

    def add_record(self, line):
        return _check(self.L, self.L.mz_loader_add_record(self.h, line.encode()))

    def num_data(self): return _check(self.L, self.L.mz_loader_num_data(self.h))
    def num_games(self): return _check(self.L, self.L.mz_loader_num_games(self.h))

    def shapes(self):
        """(batch, floats per sample of features, action_features, policy, value, reward)"""
        return tuple(_check(self.L, self.L.mz_loader_shape(self.h, k)) for k in range(6))

    @staticmethod
    def _ptr(a):
        if a is None:
            return None, None
        if hasattr(a, "data_ptr"):  # torch tensor
            assert a.is_contiguous()
            return a.data_ptr(), bool(a.is_cuda)
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data, False

    def sample_data(self, features, action_features, policy, value, reward, loss_scale, sampled_index):
        ptrs = [self._ptr(a) for a in (features, action_features, policy, value, reward, loss_scale, sampled_index)]
        sides = {d for p, d in ptrs if p is not None}
        if len(sides) != 1:
            raise MzError("sample_data: all buffers must be on the same side (host numpy arrays or CUDA tensors)")
        _check(self.L, self.L.mz_loader_sample_data(self.h, *[p for p, _ in ptrs], MZ_DEVICE if sides.pop() else MZ_HOST))

    def update_priority(self, sampled_index, batch_values):
        si = np.ascontiguousarray(sampled_index, np.int32)
        bv = np.ascontiguousarray(batch_values, np.float32)
        _check(self.L, self.L.mz_loader_update_priority(self.h, si.ctypes.data, bv.ctypes.data))


class Env:
    """Host rules engine used by the worker for AlphaZero leaves (mirror of BaseEnv, ref environment/base/base_env.h:74-114)."""

    def __init__(self, conf):
        self.L = load()
        self.h = self.L.mz_env_create(conf.encode())
        if not self.h:
            raise MzError("mz_env_create failed: " + _err(self.L))

    def close(self):
        if getattr(self, "h", None):
            self.L.mz_env_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self): self.L.mz_env_reset(self.h)
    def reset_seed(self, seed): self.L.mz_env_reset_seed(self.h, seed)
    def reward(self): return self.L.mz_env_reward(self.h)
    def act(self, a, player=None): return bool(self.L.mz_env_act(self.h, a, self.turn() if player is None else player))
    def turn(self): return self.L.mz_env_turn(self.h)
    def is_terminal(self): return bool(self.L.mz_env_is_terminal(self.h))
    def eval_score(self, resign=False): return self.L.mz_env_eval_score(self.h, int(resign))
    def policy_size(self): return self.L.mz_env_policy_size(self.h)
    def action_from_string(self, s): return self.L.mz_env_action_from_string(self.h, s.encode())

    def name(self):
        buf = C.create_string_buffer(256)
        _check(self.L, self.L.mz_env_name(self.h, buf, len(buf)))
        return buf.value.decode()

    def legal_mask(self):
        m = np.zeros(self.policy_size(), np.uint8)
        self.L.mz_env_legal_mask(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)))
        return m

    def features(self, rot=0):
        f = np.empty(self.L.mz_env_feature_size(self.h), np.float32)
        self.L.mz_env_features(self.h, rot, _f(f))
        return f

    def feature_bits(self, rot, channels, points):
        w = np.zeros(channels * ((points + 31) // 32), np.uint32)
        _check(self.L, self.L.mz_env_feature_bits(self.h, rot, w.ctypes.data_as(C.POINTER(C.c_uint32))))
        return w


def godev_playout(board_size, komi, actions, root_prefix, rots, device=0):
    """Device Go engine: root = actions[:root_prefix] on the host engine, then one device move per remaining action.
    Returns (feat_bits [steps][18*W32], legal [steps][A], terminal [steps], eval [steps], player [steps])."""
    L = load()
    P = board_size * board_size
    acts = np.ascontiguousarray(actions, np.int32)
    steps = len(acts) - root_prefix + 1
    rots = np.ascontiguousarray(rots, np.int32)
    assert len(rots) >= steps
    W32 = (P + 31) // 32
    feat = np.zeros((steps, 18 * W32), np.uint32)
    legal = np.zeros((steps, P + 1), np.uint8)
    term = np.zeros(steps, np.int32)
    ev = np.zeros(steps, np.float32)
    pl = np.zeros(steps, np.int32)
    _check(L, L.mz_godev_playout(device, board_size, komi, _i(acts), len(acts), root_prefix, _i(rots), feat.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 legal.ctypes.data_as(C.POINTER(C.c_uint8)), _i(term), _f(ev), _i(pl)))
    return feat, legal, term, ev, pl


def envdev_playout(game, board_size, komi, actions, root_prefix, rots, channels, num_actions, device=0):
    """Device rules engine of `game` ("go", "nogo", "othello", "tictactoe", "gomoku", "hex"; "havannah" through envdev_playout_conf): root = actions[:root_prefix] on the host engine, then one device move per
    remaining action.  Returns (feat_bits [steps][channels*W32], legal [steps][num_actions], terminal, eval, player)."""
    L = load()
    P = board_size * board_size
    acts = np.ascontiguousarray(actions, np.int32)
    steps = len(acts) - root_prefix + 1
    rots = np.ascontiguousarray(rots, np.int32)
    assert len(rots) >= steps
    W32 = (P + 31) // 32
    feat = np.zeros((steps, channels * W32), np.uint32)
    legal = np.zeros((steps, num_actions), np.uint8)
    term = np.zeros(steps, np.int32)
    ev = np.zeros(steps, np.float32)
    pl = np.zeros(steps, np.int32)
    _check(L, L.mz_envdev_playout(device, game.encode(), board_size, komi, _i(acts), len(acts), root_prefix, _i(rots),
                                  feat.ctypes.data_as(C.POINTER(C.c_uint32)), legal.ctypes.data_as(C.POINTER(C.c_uint8)), _i(term), _f(ev), _i(pl)))
    return feat, legal, term, ev, pl


def envdev_playout_conf(conf, board_size, actions, root_prefix, rots, channels, num_actions, device=0):
    """envdev_playout with the game and its rules from a configuration string, as Env takes it (e.g. "env_game=gomoku:env_gomoku_rule=outer_open",
    "env_game=hex:env_hex_use_swap_rule=false").  board_size: the side of the planes (Havannah: 2N - 1 for env_board_size=N)."""
    L = load()
    P = board_size * board_size
    acts = np.ascontiguousarray(actions, np.int32)
    steps = len(acts) - root_prefix + 1
    rots = np.ascontiguousarray(rots, np.int32)
    assert len(rots) >= steps
    W32 = (P + 31) // 32
    feat = np.zeros((steps, channels * W32), np.uint32)
    legal = np.zeros((steps, num_actions), np.uint8)
    term = np.zeros(steps, np.int32)
    ev = np.zeros(steps, np.float32)
    pl = np.zeros(steps, np.int32)
    _check(L, L.mz_envdev_playout_conf(device, conf.encode(), _i(acts), len(acts), root_prefix, _i(rots), feat.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       legal.ctypes.data_as(C.POINTER(C.c_uint8)), _i(term), _f(ev), _i(pl)))
    return feat, legal, term, ev, pl


def invert_values_device(values, device=0):
    """invertValue (601-bin decode) of every element by the device function of the simulation kernel."""
    L = load()
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(len(v), np.float32)
    _check(L, L.mz_invert_values_device(device, _f(v), len(v), _f(out)))
    return out


def exp_tanh_device(x, device=0):
    """(exp, tanh) of every element by the device's deterministic mz_expf / mz_tanhf (net_dev.h), the two functions of every head and softmax."""
    L = load()
    v = np.ascontiguousarray(x, np.float32)
    e, t = np.zeros(len(v), np.float32), np.zeros(len(v), np.float32)
    _check(L, L.mz_exp_tanh_device(device, _f(v), len(v), _f(e), _f(t)))
    return e, t


def tail_towers(net, bits, members):
    """The representation tower of a 9x9 x 64 network for every row of `bits` ([T][18 * 3] bit-packed planes) on `members` = 1 (solo), 2 (pair) or 4 (quad)
    workgroups of one XCD each, as the tail help of the simulation kernel runs it (sim_help.h).  Returns (activations [T][64][81], XCC_ID + 1 of every workgroup
    [members][T], error flag of the exchanges, status: 0, or 1 = the members of a tower do not share an XCD and nothing was exchanged)."""
    L = load()
    # (declared here and not in load(): a same-box A/B swaps in the parent commit's library, which does not have the symbol)
    L.mz_tail_towers_device.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    b = np.ascontiguousarray(bits, np.uint32)
    T = b.shape[0]
    out = np.zeros((T, 64, 81), np.float32)
    xcc = np.zeros((members, T), np.uint32)
    err, status = C.c_int(0), C.c_int(0)
    _check(L, L.mz_tail_towers_device(net.h, b.ctypes.data_as(C.POINTER(C.c_uint32)), T, members, _f(out), xcc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      C.byref(err), C.byref(status)))
    return out, xcc, err.value, status.value


def tail_tower_tile(tile):
    """The pixels (0 .. 80; -1: a padding column) of MFMA pixel tile `tile` of the 9x9 tower, read from the tile map its kernels are compiled with."""
    L = load()
    L.mz_tail_tower_tile.argtypes = [C.c_int, C.POINTER(C.c_int)]
    q = np.zeros(16, np.int32)
    _check(L, L.mz_tail_tower_tile(tile, _i(q)))
    return q


def sort_candidates(policy, device=0):
    """Order of candidates under the reference's std::sort(policy descending), computed by the device path."""
    L = load()
    p = np.ascontiguousarray(policy, np.float32)
    order = np.zeros(len(p), np.int32)
    _check(L, L.mz_sort_candidates(device, _f(p), len(p), _i(order)))
    return order
