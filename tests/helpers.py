"""Shared helpers of the parity tests (pure numpy; no reference code)."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def counter_u01(seed, n):
    with np.errstate(over="ignore"):
        idx = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(seed & M64)
        z = mix64(idx)
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def binary_planes(seed, shape):
    """Same input generator as tests/golden/gen_nn_golden.py."""
    n = int(np.prod(shape))
    return (counter_u01(seed, n) < 0.3).astype(np.float32).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def frac_bit_equal(a, b):
    return float(np.mean(bits(a) == bits(b)))


# round 5: network shapes beyond BASELINE.json, goldens from the reference's Python (tests/golden/gen_nn_golden.py): the reference's default 1 block x 256 channels
# (config/configuration.cpp:70-72), wider towers, 7x7 .. 19x19 Go (go_unit.h:11), channel counts that are no multiple of 16 (run-time-shaped kernels)
WIDE_NN_CFG = {
    "w_go9_1bx256_az": ("go_9x9", 18, 9, 9, 256, 9, 9, 1, 1, 82, 256, 1, "alphazero"),
    "w_go9_6bx128_az": ("go_9x9", 18, 9, 9, 128, 9, 9, 1, 6, 82, 256, 1, "alphazero"),
    "w_go19_6bx64_az": ("go_19x19", 18, 19, 19, 64, 19, 19, 1, 6, 362, 256, 1, "alphazero"),
    "w_go7_2bx32_az": ("go_7x7", 18, 7, 7, 32, 7, 7, 1, 2, 50, 256, 1, "alphazero"),
    "w_go13_2bx96_az": ("go_13x13", 18, 13, 13, 96, 13, 13, 1, 2, 170, 64, 1, "alphazero"),
    "w_go5_3bx24_az": ("go_5x5", 18, 5, 5, 24, 5, 5, 1, 3, 26, 20, 1, "alphazero"),
    "w_go9_2bx128_mz": ("go_9x9", 18, 9, 9, 128, 9, 9, 1, 2, 82, 256, 1, "muzero"),
    "w_go7_1bx40_mz": ("go_7x7", 18, 7, 7, 40, 7, 7, 1, 1, 50, 32, 1, "muzero"),
    # the reference's default network (1 block x 256 channels) on the other two games with a device leaf: Othello, TicTacToe (docs/Training.md:23)
    "w_oth8_1bx256_az": ("othello_8x8", 4, 8, 8, 256, 8, 8, 1, 1, 65, 256, 1, "alphazero"),
    "w_ttt_1bx256_az": ("tictactoe", 4, 3, 3, 256, 3, 3, 1, 1, 9, 256, 1, "alphazero"),
}


# ---------------------------------------------------------------------------------------------
# Head surgery on a weight blob: networks whose heads put out what a TRAINED network does (logits tens apart, priors that underflow to 0 and tie,
# values that saturate) instead of the near-uniform priors and near-constant values of generate_weights.  A mirror of the blob manifest of
# minizero_amd/csrc/weights.cpp (state_dict order of the reference's modules), for all three network types.
# ---------------------------------------------------------------------------------------------
def blob_manifest(desc):
    """[(name, offset, size)] of every tensor of the blob; the heads' last layers are named policy_fc, value_fc (the last value FC) and reward_fc (muzero_atari),
    each with a `.w` ([out][in]) and a `.b` entry.  The total is asserted against param_count by the callers that have one at hand (total_params)."""
    m, off = [], [0]
    C, hw = desc.num_hidden_channels, desc.hidden_channel_height * desc.hidden_channel_width
    A, VH, DV = desc.action_size, desc.num_value_hidden_channels, desc.discrete_value_size

    def add(name, n):
        m.append((name, off[0], n))
        off[0] += n

    def conv_bn(name, cin, cout, k):
        add(name + ".w", cout * cin * k * k)
        for s in ("b", "bn_g", "bn_b", "bn_m", "bn_v"):
            add(f"{name}.{s}", cout)

    def lin(name, fin, fout):
        add(name + ".w", fout * fin)
        add(name + ".b", fout)

    def trunk(name, cin):
        conv_bn(name + ".stem", cin, C, 3)
        for b in range(2 * desc.num_blocks):
            conv_bn(f"{name}.conv{b}", C, C, 3)

    def rb(name, ch):
        conv_bn(name + ".0", ch, ch, 3)
        conv_bn(name + ".1", ch, ch, 3)

    def discrete(name, hidden, size):
        hc = (size + hw - 1) // hw
        conv_bn(name + "_conv", C, hc, 1)
        lin(name + "_fc1", hw * hc, hidden)
        lin(name + "_fc", hidden, size)

    pc = (A + hw - 1) // hw
    if desc.type == 2:
        conv_bn("repr.conv1", desc.num_input_channels, C // 2, 3)
        rb("repr.rb1", C // 2)
        conv_bn("repr.conv2", C // 2, C, 3)
        rb("repr.rb2", C)
        rb("repr.rb3", C)
        for b in range(desc.num_blocks):
            rb(f"repr.tail{b}", C)
        conv_bn("dyn.conv", C + desc.num_action_feature_channels, C, 3)
        for b in range(desc.num_blocks):
            rb(f"dyn.rb{b}", C)
        discrete("reward", C, DV)
        conv_bn("policy_conv", C, pc, 1)
        lin("policy_fc", pc * hw, A)
        discrete("value", VH, DV)
        return m
    trunk("repr", desc.num_input_channels)
    if desc.type == 1:
        trunk("dyn", C + desc.num_action_feature_channels)
    conv_bn("policy_conv", C, pc, 1)
    lin("policy_fc", pc * hw, A)
    conv_bn("value_conv", C, 1, 1)
    lin("value_fc1", hw, VH)
    lin("value_fc", VH, 1)
    return m


def total_params(desc):
    name, off, n = blob_manifest(desc)[-1]
    return off + n


def _head_slices(desc, w):
    w = np.array(w, np.float32)  # a new blob
    assert w.ndim == 1 and w.size == total_params(desc), f"blob of {w.size} floats, manifest of {total_params(desc)}"
    return w, {name: slice(off, off + n) for name, off, n in blob_manifest(desc)}


def sharpen(desc, w, policy_gain, value_gain):
    """The blob with the policy FC (weight and bias) times policy_gain and the last value FC — for muzero_atari the last reward FC too — times value_gain."""
    w, s = _head_slices(desc, w)
    for head, gain in (("policy_fc", policy_gain), ("value_fc", value_gain)) + ((("reward_fc", value_gain),) if desc.type == 2 else ()):
        for part in (".w", ".b"):
            w[s[head + part]] *= np.float32(gain)
    return w


def probe_heads(desc, w, logits=None, value_pre=None, value_bins=None, reward_bins=None):
    """The blob with the named heads' last layer made constant: weight 0, bias = the given vector, so that the head puts out exactly these
    pre-activations (policy logits; the value before tanh; the value / reward bin logits of muzero_atari) for every input."""
    w, s = _head_slices(desc, w)
    given = {"policy_fc": logits, "value_fc": value_bins if desc.type == 2 else (None if value_pre is None else [value_pre]), "reward_fc": reward_bins}
    assert desc.type == 2 or (value_bins is None and reward_bins is None), "bin ladders are for muzero_atari"
    assert desc.type != 2 or value_pre is None, "muzero_atari has no scalar value pre-activation"
    for head, vec in given.items():
        if vec is None:
            continue
        vec = np.asarray(vec, np.float32).reshape(-1)
        assert vec.size == s[head + ".b"].stop - s[head + ".b"].start, f"{head}: {vec.size} values for {s[head + '.b']}"
        w[s[head + ".w"]] = 0.0
        w[s[head + ".b"]] = vec
    return w


def sharp_logits(A, peak=None):
    """One logit ladder for A actions that holds what a trained network's policy head shows and generate_weights never does: two equal maxima, a logit whose prior
    is subnormal, logits far below the exp's cut (-500, -3e38), two equal values at max - 40, +0 and -0, a value one ulp below the maximum, +-1e-40 (subnormal
    logits), and the window max - [86.5, 88.5] in which the deterministic exp passes FLT_MIN and is then cut to 0.  Cut (small A) or cycled (large A) to A entries;
    the order puts first what a short row must keep.  peak: the index the first maximum is moved to (the 601-bin ladders: an end bin, the middle)."""
    mx = np.float32(3.0)
    k = max(0, min(70, A - 12))
    ladder = np.concatenate([
        np.array([mx, mx, mx - np.float32(86.75), -500.0, mx - 40, mx - 40, 0.0, -0.0, np.nextafter(mx, np.float32(-np.inf), dtype=np.float32), -3e38, 1e-40, -1e-40],
                 np.float32),
        (mx - np.linspace(86.5, 88.5, k)).astype(np.float32)])
    out = np.resize(ladder, A).astype(np.float32)
    rep = np.arange(A) >= ladder.size  # the cycled copies stay below the two maxima
    out[rep & (out == mx)] = mx - np.float32(1.5)
    if peak is not None:
        out[[0, peak]] = out[[peak, 0]]
    return out


def f32_range(lo, hi):
    """every float32 in [lo, hi] (both of one sign)"""
    a, b = np.array([lo, hi], np.float32).view(np.uint32).astype(np.int64)
    a, b = min(a, b), max(a, b)
    return np.arange(a, b + 1, dtype=np.int64).astype(np.uint32).view(np.float32)


def sharp_primitive_inputs():
    """The inputs on which the deterministic exp / tanh are checked (oracle against float64, device against oracle): every float around the exp's cut at -87 and
    around tanh's cut at 10 and the point where (1 - e) / (1 + e) becomes exactly 1 (e < 2^-25: |x| ~ 8.66), dense sweeps over everything a head can put out,
    the clamp at 88, the narrow range the synthetic networks live in, zeros, subnormals, infinities and the largest floats.  No NaN: see tests/test_gpu_sharp.py."""
    t = np.concatenate([f32_range(9.99, 10.01), f32_range(8.6, 8.8)])
    return np.concatenate([
        f32_range(-86.0, -88.0), t, -t,
        np.linspace(-104, 89, 200000).astype(np.float32), np.linspace(-12, 12, 200000).astype(np.float32), np.linspace(-0.8, 0, 100001).astype(np.float32),
        np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, np.inf, -np.inf, 3e38, -3e38], np.float32)])


# one network shape per heads implementation of the HIP side (argument order of make_desc)
SHARP_SHAPES = {
    "go9_1bx8": ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero"),            # fused tower's heads
    "go9_6bx64": ("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82, 256, 1, "alphazero"),
    "go7_2bx32": WIDE_NN_CFG["w_go7_2bx32_az"],                                          # one-tile tower
    "go9_1bx256": WIDE_NN_CFG["w_go9_1bx256_az"],
    "go5_3bx24": WIDE_NN_CFG["w_go5_3bx24_az"],                                          # band path, heads from global memory
    "go2_1bx4": ("go_2x2", 18, 2, 2, 4, 2, 2, 1, 1, 5, 3, 1, "alphazero"),
    "ttt_2bx16": ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9, 256, 1, "alphazero"),
    "oth_6bx64": ("othello_8x8", 4, 8, 8, 64, 8, 8, 1, 6, 65, 256, 1, "alphazero"),
    "go7_1bx40_mz": WIDE_NN_CFG["w_go7_1bx40_mz"],
    "atari_1bx32": ("atari_ms_pacman", 32, 96, 96, 32, 6, 6, 18, 1, 18, 32, 601, "muzero_atari"),
}
SHARP_GAINS = [(64, 16), (512, 4), (4096, 0)]
SHARP_VALUE_PRE = [0.0, 1e-30, 0.3, 8.6, 8.7, 10.0, float(np.nextafter(np.float32(10), np.float32(np.inf))), -11.0, 3e38]


def sharp_inputs(args, batch, seed=41):
    """network inputs of a SHARP_SHAPES entry: binary planes for the board games, planes in [0, 1) for the Atari-shaped network"""
    n = args[1] * args[2] * args[3]
    if args[12] == "muzero_atari":
        return counter_u01(seed, batch * n).reshape(batch, n).astype(np.float32)
    return binary_planes(seed, (batch, n))


# Searches on sharpened networks (tests/test_sharp_regime.py checks on the oracle that each reaches what it is here for, tests/test_gpu_sharp.py runs them on the
# GPU): name -> (configuration, network, (policy gain, value gain), games, run_cycles chunks, weight seed, execution-plan variants besides the default)
_GO9_8 = ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero")
_NO_RESIGN = ":actor_resign_threshold=-2"
_ATARI_SEARCH = ("env_game=atari:nn_type_name=muzero:actor_num_simulation=4:actor_use_dirichlet_noise=false:actor_use_gumbel=true:actor_use_gumbel_noise=true:"
                 "actor_gumbel_sample_size=4:actor_mcts_value_rescale=true:actor_mcts_reward_discount=0.997:atari_init_q=true:"
                 "zero_actor_intermediate_sequence_length=10:learner_n_step_return=3:learner_muzero_unrolling_step=2:env_atari_episode_length=45:"
                 "zero_num_parallel_games=3:actor_resign_threshold=-2")
_LOCKSTEP = (":mz_sim_kernel=false",)
SHARP_SEARCHES = {
    "go9_1bx8_p4096_v0": ("env_game=go:env_board_size=9:actor_num_simulation=400:zero_num_parallel_games=2" + _NO_RESIGN, _GO9_8, (4096, 0), 2, [401, 401], 0,
                          (":mz_sim_kernel=false", ":mz_device_env=false")),
    "go9_1bx8_p1024_v8": ("env_game=go:env_board_size=9:actor_num_simulation=400:zero_num_parallel_games=2" + _NO_RESIGN, _GO9_8, (1024, 8), 2, [401, 401], 0,
                          (":mz_sim_kernel=false", ":mz_device_env=false")),
    "go9_6bx64_p1024_v8": ("env_game=go:env_board_size=9:actor_num_simulation=400:zero_num_parallel_games=8" + _NO_RESIGN, SHARP_SHAPES["go9_6bx64"], (1024, 8), 8,
                           [401, 47], 0, _LOCKSTEP),
    "go7_1bx32_p4096_v0": ("env_game=go:env_board_size=7:actor_num_simulation=200:zero_num_parallel_games=2" + _NO_RESIGN,
                           ("go_7x7", 18, 7, 7, 32, 7, 7, 1, 1, 50, 32, 1, "alphazero"), (4096, 0), 2, [201, 201], 0, _LOCKSTEP),
    "oth_1bx8_p4096_v0": ("env_game=othello:env_board_size=8:actor_num_simulation=100:zero_num_parallel_games=4" + _NO_RESIGN,
                          ("othello_8x8", 4, 8, 8, 8, 8, 8, 1, 1, 65, 16, 1, "alphazero"), (4096, 0), 4, [101] * 3, 0, _LOCKSTEP),
    "oth_1bx8_p64_v16": ("env_game=othello:env_board_size=8:actor_num_simulation=100:zero_num_parallel_games=4" + _NO_RESIGN,
                         ("othello_8x8", 4, 8, 8, 8, 8, 8, 1, 1, 65, 16, 1, "alphazero"), (64, 16), 4, [101] * 3, 0, _LOCKSTEP),
    "ttt_2bx16_p512_v4": ("env_game=tictactoe:actor_num_simulation=50:zero_num_parallel_games=8" + _NO_RESIGN, SHARP_SHAPES["ttt_2bx16"], (512, 4), 8, [51 * 10], 0,
                          _LOCKSTEP),
    # the default resign threshold: the search's own saturated value ends the games
    "go9_1bx8_resign_p64_v16": ("env_game=go:env_board_size=9:actor_num_simulation=16:zero_num_parallel_games=4", _GO9_8, (64, 16), 4, [17 * 12], 0, _LOCKSTEP),
    "go9_1bx8_mz_puct_p1024_v8": ("env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=50:zero_num_parallel_games=4" + _NO_RESIGN,
                                  _GO9_8[:12] + ("muzero",), (1024, 8), 4, [60, 93], 0, _LOCKSTEP),
    "go9_1bx8_mz_gumbel_p1024_v8": ("env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=50:zero_num_parallel_games=4:actor_use_dirichlet_noise=false:"
                                    "actor_use_gumbel=true:actor_use_gumbel_noise=true:actor_gumbel_sample_size=8" + _NO_RESIGN,
                                    _GO9_8[:12] + ("muzero",), (1024, 8), 4, [51] * 3, 0, _LOCKSTEP),
    "atari_1bx32_p512_v4": (_ATARI_SEARCH, SHARP_SHAPES["atari_1bx32"], (512, 4), 3, [5] * 6, 0, _LOCKSTEP),
}
