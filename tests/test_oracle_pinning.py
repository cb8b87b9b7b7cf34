"""CPU tests pinning the ORACLE to the reference:
  * network math            vs tests/golden/nn_*.npz   (outputs of the reference's own Python modules)
  * RNG / rotation / config vs tests/golden/ref_rng_rotation_config.json (outputs of the reference's own C++
                               sources compiled in place, oracle/_ref) and, when present, vs oracle/_ref live.
The search/actor/env part of the oracle is PARITY UNPINNED (see oracle/oracle.h); its known-answer tests are in
test_oracle_search.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import binary_planes, counter_u01, same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

NN_CFG = {
    "c1_tictactoe_az": ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9, 256, 1, "alphazero"),
    "c2_go_az": ("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82, 256, 1, "alphazero"),
    "c3_othello_az": ("othello_8x8", 4, 8, 8, 64, 8, 8, 1, 6, 65, 256, 1, "alphazero"),
    "c4_go_mz": ("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82, 256, 1, "muzero"),
    "small_go_az": ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero"),
}
from helpers import WIDE_NN_CFG  # noqa: E402
NN_CFG.update(WIDE_NN_CFG)
ATARI_CFG = {
    "c5_atari_mz": ("atari_ms_pacman", 32, 96, 96, 64, 6, 6, 18, 6, 18, 256, 601, "muzero_atari"),
    "small_atari_mz": ("atari_ms_pacman", 32, 96, 96, 32, 6, 6, 18, 1, 18, 32, 601, "muzero_atari"),
}
TOL = 1e-5  # f32 reference outputs; observed max |diff| ~1e-7 (logits) .. 7e-7 (hidden states)


@pytest.mark.parametrize("name", sorted(NN_CFG))
def test_oracle_network_matches_reference_python(oracle, name):
    args = NN_CFG[name]
    g = np.load(os.path.join(GOLD, f"nn_{name}.npz"))
    assert [str(a) for a in args] == list(g["create_network_args"])
    d = oracle.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
    net = oracle.OracleNet(d, oracle.gen_weights(d, int(g["weight_seed"])))
    for B in (1, 3):
        x = binary_planes(int(g[f"b{B}_input_seed"]), (B, args[1] * args[2] * args[3]))
        if args[12] == "alphazero":
            p, l, v = net.forward_az(x)
            assert np.abs(p - g[f"b{B}_policy"]).max() <= TOL
            assert np.abs(l - g[f"b{B}_policy_logit"]).max() <= TOL
            assert np.abs(v - g[f"b{B}_value"]).max() <= TOL
        else:
            p, l, v, h = net.initial(x)
            assert np.abs(p - g[f"b{B}_init_policy"]).max() <= TOL and np.abs(l - g[f"b{B}_init_policy_logit"]).max() <= TOL
            assert np.abs(v - g[f"b{B}_init_value"]).max() <= TOL and np.abs(h - g[f"b{B}_init_hidden_state"]).max() <= TOL
            act = np.zeros((B, args[5] * args[6]), np.float32)
            for b in range(B):
                act[b, (7 * b + 3) % (args[5] * args[6])] = 1.0
            p, l, v, r, h2 = net.recurrent(g[f"b{B}_init_hidden_state"], act)
            assert np.abs(p - g[f"b{B}_rec_policy"]).max() <= TOL and np.abs(l - g[f"b{B}_rec_policy_logit"]).max() <= TOL
            assert np.abs(v - g[f"b{B}_rec_value"]).max() <= TOL and np.abs(h2 - g[f"b{B}_rec_hidden_state"]).max() <= TOL
            assert np.all(h2 >= 0) and np.all(h2 <= 1) and np.all(r == 0)


@pytest.mark.parametrize("name", sorted(ATARI_CFG))
def test_oracle_atari_network_matches_reference_python(oracle, name):
    """muzero_atari (ref network/py/muzero_atari_network.py): strided stem, pooled residual stages, 601-bin heads"""
    args = ATARI_CFG[name]
    g = np.load(os.path.join(GOLD, f"nn_{name}.npz"))
    d = oracle.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
    net = oracle.OracleNet(d, oracle.gen_weights(d, int(g["weight_seed"])))
    for B in (1, 2):
        x = counter_u01(int(g[f"b{B}_input_seed"]), B * 32 * 96 * 96).reshape(B, -1).astype(np.float32)
        p, l, v, h = net.initial(x)
        assert np.abs(p - g[f"b{B}_init_policy"]).max() <= TOL and np.abs(l - g[f"b{B}_init_policy_logit"]).max() <= TOL
        assert np.abs(h - g[f"b{B}_init_hidden_state"]).max() <= TOL
        # value = invertValue(expectation of the 601-bin softmax) (ref muzero_network.h:157-163, utils.h:102-108)
        assert np.abs(v - net.invert(g[f"b{B}_init_value"])).max() <= 5e-4  # f32 index-ordered sum of 601 terms x |i-300| (as the reference does) vs an f64 sum
        act = np.zeros((B, 18, 36), np.float32)
        for b in range(B):
            act[b, (7 * b + 3) % 18] = 1.0
        p, l, v, r, h2 = net.recurrent(g[f"b{B}_init_hidden_state"], act.reshape(B, -1))
        assert np.abs(p - g[f"b{B}_rec_policy"]).max() <= TOL and np.abs(h2 - g[f"b{B}_rec_hidden_state"]).max() <= TOL
        assert np.abs(v - net.invert(g[f"b{B}_rec_value"])).max() <= 5e-4 and np.abs(r - net.invert(g[f"b{B}_rec_reward"])).max() <= 5e-4


def test_param_counts_match_survey(oracle):
    # SURVEY.md §8a a20 parameter counts (+ BN running stats: 2 per BN channel)
    for desc, params, bn_ch in ((oracle.desc_c1(), 12977, 16 * 5 + 1 + 1), (oracle.desc_c2(), 490048, 64 * 13 + 2 + 1),
                                (oracle.desc_c3(), 472651, 64 * 13 + 2 + 1), (oracle.desc_c4(), 972352, 64 * 26 + 2 + 1),
                                (oracle.desc_c5(), 1524245, 32 * 3 + 64 * 30 + 17 + 1 + 17)):
        assert oracle.lib().mzo_net_param_count(C.byref(desc)) == params + 2 * bn_ch


def test_weight_generator_twins(oracle, mz):
    """the same SplitMix64 stream in oracle/o_nn.cpp, minizero_amd/csrc/weights.cpp and numpy"""
    for d_o, d_m in ((oracle.desc_c1(), mz.DESCS["c1"]()), (oracle.desc_c4(), mz.DESCS["c4"]())):
        for seed in (0, 12345):
            a, b = oracle.gen_weights(d_o, seed), mz.generate_weights(d_m, seed)
            assert same_bits(a, b)
    d = oracle.desc_c1()
    w = oracle.gen_weights(d, 0)
    u = counter_u01(0, w.size)
    bound = np.float32(1.0) / np.sqrt(np.float32(36))  # first tensor: stem conv weight, fan_in = 4*3*3
    assert same_bits(w[:16 * 36], (-bound + (bound - (-bound)) * u[:16 * 36]).astype(np.float32))


def test_deterministic_exp_tanh_accuracy(oracle):
    """The range a softmax of ordinary logits uses.  tests/test_sharp_regime.py test_primitives_against_float64 checks the wider input set (every float around
    the cut to 0 and around tanh's cut and saturation, the clamp at 88, subnormals, infinities), tests/test_gpu_sharp.py the device copy on the same set."""
    x = np.concatenate([np.linspace(-87, 0, 20001), np.linspace(0, 5, 2001)]).astype(np.float32)
    y = np.empty_like(x)
    oracle.lib().mzo_expf(oracle.fptr(x), x.size, oracle.fptr(y))
    ref = np.exp(x.astype(np.float64))
    assert np.max(np.abs(y - ref) / ref) < 2.5e-7
    x = np.linspace(-12, 12, 40001).astype(np.float32)
    y = np.empty_like(x)
    oracle.lib().mzo_tanhf(oracle.fptr(x), x.size, oracle.fptr(y))
    assert np.max(np.abs(y - np.tanh(x.astype(np.float64)))) < 2e-7


# ---------------------------------------------------------------------------------------------
def _ref_fixture():
    with open(os.path.join(GOLD, "ref_rng_rotation_config.json")) as f:
        return json.load(f)


def test_rng_matches_reference_random_h(oracle):
    fx = _ref_fixture()
    for case in fx["rng"]:
        n = len(case["values"])
        buf = (C.c_double * n)()
        oracle.lib().mzo_rng_vector(case["seed"], case["kind"], n, case["k"], case["alpha"], buf)
        got = [float.hex(v) for v in buf]
        assert got == case["values"], f"RNG kind {case['kind']} k={case['k']} seed {case['seed']} differs from the reference"


def test_rotation_matches_reference_rotation_h(oracle):
    fx = _ref_fixture()
    L = oracle.lib()
    assert [L.mzo_reversed_rotation(r) for r in range(8)] == fx["reversed_rotation"]
    for n, table in fx["rotation"].items():
        n = int(n)
        for r in range(8):
            assert [L.mzo_rotate(r, p, n) for p in range(n * n + 1)] == table[r]


def test_config_matches_reference_configuration_cpp(oracle):
    fx = _ref_fixture()
    L = oracle.lib()
    for case in fx["config"]:
        buf = C.create_string_buffer(1 << 16)
        rc = L.mzo_config_dump(case["conf"].encode(), buf, len(buf))
        assert (rc < 0) == case["rc_negative"], case["conf"]
        if rc >= 0:
            assert buf.value.decode() == case["dump"], case["conf"]


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libmzref.so")), reason="oracle/_ref not built")
def test_live_reference_build_agrees(oracle):
    """oracle/_ref (the reference's own sources) against the oracle on fresh seeds, beyond the committed fixture"""
    R = C.CDLL(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libmzref.so"))
    R.mzref_rng_vector.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_double)]
    L = oracle.lib()
    for seed in (3, 99, 123456):
        for kind, k, alpha in ((0, 0, 0.0), (1, 0, 0.0), (2, 30, 0.03), (3, 20, 0.0)):
            n = 200
            a, b = (C.c_double * n)(), (C.c_double * n)()
            R.mzref_rng_vector(seed, kind, n, k, alpha, a)
            L.mzo_rng_vector(seed, kind, n, k, alpha, b)
            assert list(a) == list(b)
    for n in (5, 7, 13):
        for r in range(8):
            for p in range(n * n + 1):
                assert R.mzref_rotate(r, p, n) == L.mzo_rotate(r, p, n)


def _sgf_fixture():
    with open(os.path.join(HERE, "golden", "ref_sgf_vectormap.json")) as f:
        return json.load(f)


def test_record_state_machine_matches_reference_sgf_loader(oracle):
    """oracle RecordLoader (the state machine base_env.h:150-205 shares with utils/sgf_loader.cpp:26-83) against the reference's own SGFLoader"""
    L = oracle.lib()
    fx = _sgf_fixture()
    assert len(fx["sgf"]) >= 40
    buf = C.create_string_buffer(1 << 16)
    for e in fx["sgf"]:
        L.mzo_sgf_parse(e["in"].encode(), buf, len(buf))
        assert buf.value.decode(errors="replace") == e["out"], e["in"]
    for e in fx["coords"]:
        o = (C.c_int * 2)()
        L.mzo_sgf_coords(0, e["n"], e["coord"].encode(), e["sgf"].encode(), o)
        assert [o[0], o[1]] == e["out"], e
    for e in fx["strings"]:
        L.mzo_sgf_strings(e["action"], e["n"], buf, len(buf))
        assert buf.value.decode() == e["out"], e


def test_tag_map_matches_reference_vector_map(oracle):
    """oracle TagMap against the reference's utils/vector_map.h: operator[] finds-or-appends, insert keeps an existing value, order = insertion"""
    L = oracle.lib()
    fx = _sgf_fixture()
    buf = C.create_string_buffer(1 << 16)
    for e in fx["tagmap"]:
        L.mzo_tagmap_apply(e["ops"].encode(), buf, len(buf))
        assert buf.value.decode() == e["out"], e["ops"]
    assert fx["go_unit"] == {"kMaxGoBoardSize": 19, "kGoNumPlayer": 2, "sizeof_GoHashKey": 8, "GoBitboard_bits": 361, "kGoName_len": 2}


def test_register_blocked_convolution_is_the_scalar_chain(oracle):
    """oracle/o_nn.cpp convChains keeps the (tap, channel)-ordered fmaf chains of 4 pixels x 16 output channels in AVX2 registers; every output bit must equal the scalar
    loop that defines the contract (conv3x3sScalar) — channel counts off the blocks of 16, pixel counts off the blocks of 4, strides, with and without the skip input,
    zeros and denormal-sized values in the data."""
    L = oracle.lib()
    L.mzo_conv_selftest.restype = C.c_int
    L.mzo_conv_selftest.argtypes = [C.c_int] * 6 + [C.c_uint64]
    cases = [(1, 1, 1, 1, 1), (3, 5, 2, 3, 1), (18, 64, 9, 9, 1), (20, 33, 7, 5, 1), (64, 64, 8, 8, 1), (32, 32, 11, 13, 2), (17, 48, 6, 6, 2), (96, 96, 13, 13, 1), (4, 256, 3, 3, 1), (40, 17, 25, 4, 1)]
    for seed, (cin, cout, H, W, stride) in enumerate(cases):
        for skip in (0, 1):
            assert L.mzo_conv_selftest(cin, cout, H, W, stride, skip, seed + 1) == 0, (cin, cout, H, W, stride, skip)
