"""The external evaluator (mz_worker_create_external): the search runs on the caller's own network.  Every test creates the external worker first.

1. the library's own network behind `forward`, on library-owned buffers: lines and records byte for byte those of a Worker on the lock-step plan (and of the
   oracle where it plays the game), over the shapes at which the export and import kernels change path;
2. the same with policy = NULL: the library's softmax of the logits is the heads' policy bit for bit;
3. f16 / bf16 features and outputs;
4. an evaluator that is no CNN, written twice (numpy for tests/search_model.py, torch for the worker): moves and P strings of the independent model;
5. the manual-step surface; 6. the failure paths and the refusals.
Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import search_model as S
import test_search_model as T
from helpers import sharpen

pytestmark = pytest.mark.gpu

LOCKSTEP = ":mz_sim_kernel=false"
BASE = ":zero_num_threads=1:program_seed=5:nn_file_name=ext.pt"


def _net(name, planes, side, actions, ch=8):
    return (name, planes, side, side, ch, side, side, 1, 1, actions, 16, 1, "alphazero")


GO9 = _net("go_9x9", 18, 9, 82)
GUMBEL4 = ":actor_use_dirichlet_noise=false:actor_use_gumbel=true:actor_use_gumbel_noise=true:actor_gumbel_sample_size=4"
# name -> (configuration, network, games, cycles per run_cycles call, the oracle plays it too, (policy, value) gain on the heads or None, records must have ended)
# The shapes: TicTacToe — 4 planes of 9 points in one partial word, 9 actions; Othello — whole words, 65 actions; Go 9x9 — 18 planes, 1458 elements per game
# (the export's 4-element vectors straddle planes and games), 82 actions; Go 19x19 — 12 words per plane, 362 actions (beyond 256: six turns of the import's
# wave); Gomoku 15x15, Hex 11x11, NoGo 9x9, Havannah edge 4 = 20 planes of 7x7.
CASES = {
    "ttt": ("env_game=tictactoe:actor_num_simulation=8", _net("tictactoe", 4, 3, 9, 16), 3, [9 * 7, 9 * 23], True, None, True),
    "othello": ("env_game=othello:env_board_size=8:actor_num_simulation=8", _net("othello_8x8", 4, 8, 65), 3, [9 * 35, 9 * 40], True, None, True),
    # the defaults: PUCT, Dirichlet noise at the root, the move drawn from the softmax of the counts
    "go9_puct_noise_softmax": ("env_game=go:env_board_size=9:actor_num_simulation=16", GO9, 5, [17 * 3, 17 * 4 + 5], True, None, False),
    "go9_gumbel": ("env_game=go:env_board_size=9:actor_num_simulation=16" + GUMBEL4, GO9, 3, [17 * 5 + 3], True, None, False),
    "go9_rotation": ("env_game=go:env_board_size=9:actor_num_simulation=8:actor_use_random_rotation_features=true", GO9, 5, [9 * 6], True, None, False),
    # a sharpened value head and the default resign threshold: the games end by resignation and start again
    "go9_resign": ("env_game=go:env_board_size=9:actor_num_simulation=16", GO9, 3, [17 * 12], True, (64, 16), True),
    "go19": ("env_game=go:env_board_size=19:actor_num_simulation=8", _net("go_19x19", 18, 19, 362, 32), 2, [9 * 2], True, None, False),
    "gomoku15": ("env_game=gomoku:env_board_size=15:actor_num_simulation=8", _net("gomoku_15x15", 4, 15, 225, 32), 3, [9 * 6], False, None, False),
    "hex11_swap": ("env_game=hex:env_board_size=11:env_hex_use_swap_rule=true:actor_num_simulation=8", _net("hex_11x11", 4, 11, 121, 32), 3, [9 * 8], False, None, False),
    "nogo9": ("env_game=nogo:env_board_size=9:actor_num_simulation=8", _net("nogo_9x9", 18, 9, 82, 32), 3, [9 * 8], False, None, False),
    "havannah4": ("env_game=havannah:env_board_size=4:actor_num_simulation=8", _net("havannah4x4", 20, 7, 49, 32), 3, [9 * 45], False, None, True),
}


def case_conf(name):
    conf, _, games, *_ = CASES[name]
    return conf + f":zero_num_parallel_games={games}" + BASE


def case_net(mz, name):
    _, args, _, _, _, gain, _ = CASES[name]
    d = mz.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
    w = mz.generate_weights(d, 3)
    return d, (w if gain is None else sharpen(d, w, *gain))


# ---- device memory of the test's own (the caller's buffers where torch is not used) ----
_HIP = None


def hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")  # the runtime libmzgpu itself is linked against
        _HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _HIP.hipFree.argtypes = [C.c_void_p]
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return _HIP


class DevMem:
    def __init__(self, nbytes):
        self.p, self.nbytes = C.c_void_p(), nbytes
        assert hip().hipMalloc(C.byref(self.p), nbytes) == 0
        assert hip().hipMemset(self.p, 0, nbytes) == 0
        self.addr = self.p.value

    def __del__(self):
        if getattr(self, "p", None):
            hip().hipFree(self.p)
            self.p = None

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes and hip().hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0

    def get(self, dtype, count, offset=0):
        out = np.empty(count, dtype)
        assert offset + out.nbytes <= self.nbytes and hip().hipMemcpy(out.ctypes.data, self.addr + offset, out.nbytes, 2) == 0
        return out


def read_device(addr, dtype, count):
    out = np.empty(count, dtype)
    assert hip().hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0
    return out


class OwnNet:
    """forward = mz_net_forward_az of the library's own network on the hand-over buffers; `calls` counts"""

    def __init__(self, mz, net):
        self.mz, self.net, self.calls, self.ptr = mz, net, 0, None

    def __call__(self, rows):
        f, p, l, v = self.ptr
        self.calls += 1
        return self.mz.load().mz_net_forward_az(self.net.h, f, rows, p, l, v, self.mz.MZ_DEVICE)


def run_worker(wk, chunks, games):
    wk.command("start")
    for c in chunks:
        assert wk.run_cycles(c) == c
    return wk.pop_lines(), wk.peek_records(games)


_INTERNAL = {}


def internal(mz, name):
    """lines and records of the Worker with a network of its own on the lock-step plan: computed once, shared"""
    if name not in _INTERNAL:
        d, w = case_net(mz, name)
        wk = mz.Worker(case_conf(name) + LOCKSTEP, d, w)
        _INTERNAL[name] = run_worker(wk, CASES[name][3], CASES[name][2])
        assert wk.stats()["sim_launches"] == 0
        wk.close()
    return _INTERNAL[name]


def external_own_net(mz, name, extra="", policy_null=False):
    """(worker, evaluator, what keeps the buffers alive): the external worker of a case with the library's network as its evaluator"""
    d, w = case_net(mz, name)
    net = mz.Net(d, w)
    ev = OwnNet(mz, net)
    if not policy_null:
        wk = mz.ExternalWorker(case_conf(name) + LOCKSTEP + extra, d, ev)
        ev.ptr = wk.buffers()
        assert all(ev.ptr)
        return wk, ev, None
    G, A, feat = CASES[name][2], d.action_size, d.num_input_channels * d.input_channel_height * d.input_channel_width
    mem = [DevMem(4 * G * feat), DevMem(4 * G * A), DevMem(4 * G * A), DevMem(4 * G)]  # features, the heads' policy (kept from the worker), logits, value
    wk = mz.ExternalWorker(case_conf(name) + LOCKSTEP + extra, d, ev, features=mem[0].addr, policy=None, logits=mem[2].addr, value=mem[3].addr)
    assert wk.buffers() == (mem[0].addr, None, mem[2].addr, mem[3].addr)
    ev.ptr = tuple(m.addr for m in mem)
    return wk, ev, mem


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_own_network_as_evaluator_byte_for_byte(mz, oracle, name):
    wk, ev, _ = external_own_net(mz, name)
    conf, args, games, chunks, has_oracle, gain, ends = CASES[name]
    lines, records = run_worker(wk, chunks, games)
    assert ev.calls == sum(chunks) and wk.lanes() == 1 and wk.stats()["sim_launches"] == 0
    wk.close()
    ref_lines, ref_records = internal(mz, name)
    assert lines == ref_lines and records == ref_records
    assert bool(lines) == ends, f"{len(lines)} finished games"
    if has_oracle:
        d, w = case_net(mz, name)
        og = oracle.OracleGroup(case_conf(name), oracle.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12]), w)
        og.cycles(sum(chunks))
        assert lines == og.lines() and records == og.peek_records(games)


@pytest.mark.parametrize("name", ["go9_puct_noise_softmax", "ttt", "go19"])
def test_library_softmax_is_the_heads_policy(mz, name):
    wk, ev, mem = external_own_net(mz, name, policy_null=True)
    conf, args, games, chunks, *_ = CASES[name]
    wk.command("start")
    assert wk.run_cycles(1) == 1 and ev.calls == 1
    A = args[9]
    heads = mem[1].get(np.float32, games * A).reshape(games, A)
    lane = wk.lane_policy(games)
    assert np.array_equal(lane.view(np.uint32), heads.view(np.uint32)) and np.all(heads > 0)
    assert wk.run_cycles(chunks[0] - 1) == chunks[0] - 1
    for c in chunks[1:]:
        assert wk.run_cycles(c) == c
    lines, records = wk.pop_lines(), wk.peek_records(games)
    wk.close()
    assert (lines, records) == internal(mz, name)


# ---------------------------------------------------------------------------------------------
# dtypes: a fixed table of outputs, exactly representable in bf16 (at most 8 significant bits) and so in f16 and f32
# ---------------------------------------------------------------------------------------------
def to_dtype(a, dtype):
    a = np.asarray(a, np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        h = a.astype(np.float16)
        assert np.array_equal(h.astype(np.float32), a)
        return h
    bits = a.view(np.uint32)
    assert not np.any(bits & 0xFFFF), "not a bf16 value"
    return (bits >> 16).astype(np.uint16)


def from_dtype(raw, dtype):
    if dtype == "f32":
        return raw
    if dtype == "f16":
        return raw.view(np.float16).astype(np.float32)
    return (raw.astype(np.uint32) << 16).view(np.float32)


def table_run(mz, feature_dtype, output_dtype, feature_offset=0):
    """Go 9x9 with rotated features, 3 games, 27 cycles on the table; -> (lines, records, the features of every cycle as f32)"""
    G, A, CP, n = 3, 82, 18 * 81, 8
    conf = f"env_game=go:env_board_size=9:actor_num_simulation={n}:actor_use_random_rotation_features=true:zero_num_parallel_games={G}" + BASE
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, A)
    a, g = np.arange(A)[None, :], np.arange(G)[:, None]
    policy = ((a * 37 + g * 11) % 83 + 1).astype(np.float32) / 128   # distinct within a game
    logits = ((a * 7 + g * 3) % 32 - 16).astype(np.float32) / 8
    value = (np.arange(G) - 1).astype(np.float32) / 4
    fb, ob = (4 if feature_dtype == "f32" else 2), (4 if output_dtype == "f32" else 2)
    mem = [DevMem(fb * G * CP + 64), DevMem(ob * G * A), DevMem(ob * G * A), DevMem(ob * G)]
    for m, t in zip(mem[1:], (policy, logits, value)):
        m.put(to_dtype(t, output_dtype))
    seen = []
    raw_type = np.float32 if feature_dtype == "f32" else np.uint16

    def forward(rows):
        assert rows == G
        seen.append(from_dtype(mem[0].get(raw_type, G * CP, feature_offset), feature_dtype))

    wk = mz.ExternalWorker(conf, d, forward, features=mem[0].addr + feature_offset, policy=mem[1].addr, logits=mem[2].addr, value=mem[3].addr,
                           feature_dtype=feature_dtype, output_dtype=output_dtype)
    lines, records = run_worker(wk, [3 * (n + 1)], G)
    wk.close()
    return lines, records, np.stack(seen)


def test_dtypes_of_features_and_outputs(mz):
    ref = table_run(mz, "f32", "f32")
    assert ref[2].shape == (27, 3 * 18 * 81) and set(np.unique(ref[2])) == {0.0, 1.0} and len(set(map(bytes, ref[2]))) > 9
    assert all(";B[" in r for r in ref[1])
    runs = [("f16", "f32", 0), ("bf16", "f32", 0), ("f32", "f16", 0), ("f32", "bf16", 0), ("bf16", "bf16", 0), ("f16", "f16", 0),
            ("f32", "f32", 4), ("f16", "f16", 2)]  # the last two: a features pointer that is not aligned for the 4-element vector
    for fd, od, off in runs:
        got = table_run(mz, fd, od, off)
        assert np.array_equal(got[2], ref[2]), (fd, od, off)
        assert got[:2] == ref[:2], (fd, od, off)


# ---------------------------------------------------------------------------------------------
# any network: table + plane bits, written twice
# ---------------------------------------------------------------------------------------------
class TableNet:
    """logit[a] = pi(a) / 4 + (sum_c k_c * plane_c[a]) / 64 with k_c in {-1, 0, 1}: at most 18 planes, so two sums differ by at most 12 < 16 and the
    logits of a position are distinct; policy[a] = a fixed table of distinct values; value = a dyadic function of the stone counts of planes 0 and 1.
    Every number is a small multiple of 1/64 or 1/128: exact in float32 whatever the order of the sums."""

    def __init__(self, C_, P, A):
        self.C, self.P, self.A = C_, P, A
        rng = np.random.default_rng(11)
        assert C_ <= 18
        self.pi = (rng.permutation(A) - A // 2).astype(np.float32) / 4
        self.k = ((np.arange(C_) % 3) - 1).astype(np.float32)
        self.policy = (rng.permutation(A) + 1).astype(np.float32) / 128

    # numpy, for the model: one position
    def forward(self, feat):
        pl = np.asarray(feat, np.float32).reshape(self.C, self.P)
        logit = self.pi.copy()
        logit[:self.P] += (self.k[:, None] * pl).sum(0) / np.float32(64)
        s0, s1 = pl[0].sum(), pl[1].sum()
        value = np.float32((2 * (s0 - s1) + (s0 + s1) % 3 - 1) / 16)
        return self.policy, logit.astype(np.float32), value

    # torch, for the worker: the pool's positions at once
    def module(self, torch, device):
        pi, k, policy = (torch.tensor(x, device=device) for x in (self.pi, self.k, self.policy))

        def f(features):
            G = features.shape[0]
            pl = features.reshape(G, self.C, self.P).float()
            logit = pi.repeat(G, 1)
            logit[:, :self.P] += (k[None, :, None] * pl).sum(1) / 64
            s0, s1 = pl[:, 0].sum(1), pl[:, 1].sum(1)
            value = (2 * (s0 - s1) + torch.remainder(s0 + s1, 3) - 1) / 16
            return policy.repeat(G, 1), logit, value
        return f


MODEL_GAMES = {
    "gomoku7": ("env_game=gomoku:env_board_size=7", 4, 7, 49),
    "hex5_swap": ("env_game=hex:env_board_size=5:env_hex_use_swap_rule=true", 4, 5, 25),
    "go5": ("env_game=go:env_board_size=5", 18, 5, 26),
}
MODEL_SEARCHES = {"puct": ":actor_num_simulation=16", "gumbel": T._gumbel(16, 8)}


@pytest.mark.parametrize("search", list(MODEL_SEARCHES))
@pytest.mark.parametrize("game", list(MODEL_GAMES))
def test_any_network_equals_search_model(mz, oracle, game, search):
    torch = pytest.importorskip("torch")
    base, planes, side, A = MODEL_GAMES[game]
    conf, games, moves = base + MODEL_SEARCHES[search], 3, 3
    d = mz.make_desc(game, planes, side, side, 1, side, side, 1, 1, A)
    tn = TableNet(planes, side * side, A)
    ev = mz.TorchEvaluator(tn.module(torch, "cuda:0"), games, planes, side, side, A, "f32", device="cuda:0")
    assert ev.policy is not None
    wk = ev.worker(T.full_conf(conf, games), d)
    wk.command("start")
    cfg = T.model_cfg(conf)[0]
    for _ in range(moves + 1):
        assert wk.run_cycles(cfg.actor_num_simulation + 1) == cfg.actor_num_simulation + 1
    got = T.games_of(wk.pop_lines(), wk.peek_records(games), games, moves)
    wk.close()
    try:
        played = S.play(cfg, T.make_env(oracle, conf), tn, moves, False, None)
    except S.AmbiguousOrder as e:  # the tables give distinct policies and logits at every leaf: no case may drop out this way
        pytest.fail(f"the model met a tie: {e}")
    assert len(played) == moves and not any(m["resign"] for m in played)
    T.check_against(([(m["action"], m["P"], m["V"], m["R"]) for m in played], False, False), got)


# ---------------------------------------------------------------------------------------------
def manual_sequence(wk, games, n):
    """the manual-step surface, every answer kept"""
    out = []
    wk.command("start")
    while not wk.search_done():
        out.append(wk.run_cycles(5))
    acts = [wk.search_action(g) for g in range(games)]
    out.append(acts)
    out.append([(wk.tree_string(g), wk.node_info(g, 0), wk.node_info(g, 1)) for g in range(games)])
    trees = [wk.tree(g) for g in range(games)]
    out.append([wk.act(g, a, p) for g, (a, p, _) in enumerate(acts)])
    wk.reset_search()
    out.append(wk.run_cycles(5))
    trees += [wk.tree(g) for g in range(games)]
    wk.finish_search()
    out.append([wk.search_action(g) for g in range(games)])
    out.append([wk.tree_string(g) for g in range(games)])
    trees += [wk.tree(g) for g in range(games)]
    out.append(wk.peek_records(games))
    return out, trees


def test_manual_step_surface(mz):
    name, extra = "go9_puct_noise_softmax", ":mz_manual_step=true:actor_num_simulation=12"
    wk, ev, _ = external_own_net(mz, name, extra)
    games = CASES[name][2]
    got, got_trees = manual_sequence(wk, games, 12)
    wk.close()
    d, w = case_net(mz, name)
    ref = mz.Worker(case_conf(name) + LOCKSTEP + extra, d, w)
    want, want_trees = manual_sequence(ref, games, 12)
    ref.close()
    assert got == want
    assert len(got_trees) == len(want_trees) == 3 * games
    for a, b in zip(got_trees, want_trees):
        assert a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
    assert all(len(t["count"]) > 1 for t in got_trees)


# ---------------------------------------------------------------------------------------------
def test_forward_returning_nonzero_ends_the_worker(mz):
    name = "go9_puct_noise_softmax"
    d, w = case_net(mz, name)
    net = mz.Net(d, w)
    own = OwnNet(mz, net)
    games = CASES[name][2]

    def forward(rows):
        return 7 if own.calls == 4 else own(rows)

    wk = mz.ExternalWorker(case_conf(name) + ":mz_manual_step=true", d, forward)
    own.ptr = wk.buffers()
    wk.command("start")
    assert wk.run_cycles(4) == 4 and own.calls == 4
    before = [len(wk.tree(g)["count"]) for g in range(games)]
    assert all(b == 4 for b in before)  # the root and three visited children: the fourth cycle's expand has run, the fifth's never will
    for _ in range(2):
        with pytest.raises(mz.MzError, match=r"libmzgpu error -3: external evaluator: forward returned 7"):
            wk.run_cycles(3)
    assert own.calls == 4
    assert [len(wk.tree(g)["count"]) for g in range(games)] == before
    wk.close()


def test_exception_in_forward_is_raised_from_run_cycles(mz):
    name = "ttt"
    d, _ = case_net(mz, name)

    def forward(rows):
        raise ValueError(f"no network for {rows} rows")

    wk = mz.ExternalWorker(case_conf(name), d, forward)
    wk.command("start")
    with pytest.raises(ValueError, match="no network for 3 rows") as e:
        wk.run_cycles(2)
    assert any(tb.name == "forward" for tb in e.traceback)
    with pytest.raises(mz.MzError, match="forward returned"):
        wk.run_cycles(1)
    wk.close()


REFUSALS = [
    (":nn_type_name=muzero", {}, "nn_type_name"),
    ("", {"type": 1}, "desc.type"),
    (":mz_device_env=false", {}, "mz_device_env"),
    (":zero_num_parallel_games=1041", {}, "zero_num_parallel_games"),
    (":mz_pipeline_lanes=2", {}, "mz_pipeline_lanes"),
    (":actor_mcts_think_batch_size=4:mz_manual_step=true", {}, "actor_mcts_think_batch_size"),
    (":mz_nn_precision=bf16x3", {}, "mz_nn_precision"),
]


@pytest.mark.parametrize("extra,fields,key", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_refusals_name_the_key(mz, extra, fields, key):
    d = mz.make_desc("go_9x9", 18, 9, 9, 1, 9, 9, 1, 1, 82)
    for k, v in fields.items():
        setattr(d, k, v)
    with pytest.raises(mz.MzError) as e:
        mz.ExternalWorker("env_game=go:env_board_size=9:actor_num_simulation=4:zero_num_parallel_games=2" + extra, d, lambda rows: 0)
    assert key in str(e.value) and "external evaluator" in str(e.value)


def test_refusals_of_game_and_descriptor(mz):
    go = "env_game=go:env_board_size=9:actor_num_simulation=4:zero_num_parallel_games=2"

    def refused(conf, *shape):
        with pytest.raises(mz.MzError) as e:
            mz.ExternalWorker(conf, mz.make_desc("x", shape[0], shape[1], shape[1], 1, shape[1], shape[1], 1, 1, shape[2]), lambda rows: 0)
        assert "external evaluator" in str(e.value)
        return str(e.value)

    assert "env_game=atari" in refused("env_game=atari:actor_num_simulation=4:zero_num_parallel_games=2", 32, 96, 18)
    msg = refused(go, 17, 9, 82)
    assert "num_input_channels=17" in msg and "18" in msg
    msg = refused(go, 18, 9, 81)
    assert "action_size=81" in msg and "82" in msg
    msg = refused("env_game=havannah:env_board_size=4:actor_num_simulation=4:zero_num_parallel_games=2", 20, 4, 49)
    assert "4 x 4" in msg and "7 x 7" in msg
    # ... and the shape that fits is taken
    wk = mz.ExternalWorker("env_game=havannah:env_board_size=4:actor_num_simulation=4:zero_num_parallel_games=2", mz.make_desc("x", 20, 7, 7, 1, 7, 7, 1, 1, 49), lambda rows: 0)
    assert all(wk.buffers())
    wk.close()
