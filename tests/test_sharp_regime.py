"""The regime of a TRAINED network on the CPU oracle: logits tens apart, priors that underflow to subnormals and to exact zeros, tied priors, values that
saturate, searches that run down one line to the end of the game.  The synthetic networks of generate_weights put out none of this (logits within +-0.4,
priors near uniform, |v| < 0.3), so everything the other tests claim about exp, tanh, the softmax and the search rests on that narrow range.

tests/test_gpu_sharp.py compares the HIP side with the oracle bit for bit on the inputs of this file (tests/helpers.py: sharp_primitive_inputs, sharp_logits,
SHARP_SHAPES, SHARP_GAINS, SHARP_SEARCHES); this file checks the oracle itself against float64 on them, and that each input still reaches what it is there for,
so that the GPU tests cannot pass on a regime that degenerated."""
import ctypes as C

import numpy as np
import pytest

from helpers import (SHARP_GAINS, SHARP_SEARCHES, SHARP_SHAPES, blob_manifest, probe_heads, sharp_inputs, sharp_logits, sharp_primitive_inputs, sharpen,
                     total_params)

FLT_MIN = 2.0 ** -126
DENORM = 2.0 ** -149
EXP_REL = 2.5e-7          # tests/test_oracle_pinning.py test_deterministic_exp_tanh_accuracy
TANH_ABS = 2e-7           # the same
EXP_FLUSH_UNITS = 8388582  # measured 8388581.99: see test_primitives_against_float64
SOFTMAX_FLUSH_UNITS = 2611589  # measured 2611588.5 (9x9 Go rows): see test_probe_softmax_against_float64


def _desc(oracle, args):
    return oracle.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])


def test_manifest_mirror_counts_every_parameter(oracle):
    """helpers.blob_manifest (the Python mirror of the blob manifest of weights.cpp / o_nn.cpp) against param_count, for all three network types; the heads'
    last layers have the sizes sharpen / probe_heads rely on."""
    shapes = dict(SHARP_SHAPES, c4=("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82, 256, 1, "muzero"), c5=("atari_ms_pacman", 32, 96, 96, 64, 6, 6, 18, 6, 18, 256, 601, "muzero_atari"))
    for name, args in shapes.items():
        d = _desc(oracle, args)
        assert total_params(d) == oracle.lib().mzo_net_param_count(C.byref(d)), name
        sizes = {n: s for n, _, s in blob_manifest(d)}
        assert sizes["policy_fc.b"] == args[9] and sizes["value_fc.b"] == args[11]
        assert (args[12] == "muzero_atari") == ("reward_fc.b" in sizes)


def test_primitives_against_float64(oracle):
    """mzo_expf / mzo_tanhf on sharp_primitive_inputs (1.22 M floats) against float64 exp / tanh.
      * exp, true result >= FLT_MIN (the input clamped at 88 as the function does): relative error <= 2.5e-7.  Measured 7.98e-8.
      * exp, true result < FLT_MIN: the function returns 0 below the first float whose exp is a normal number (-87.3365402), so the error is the true value
        itself: at most 8388581.99 units of 2^-149 (measured; FLT_MIN is 2^23 = 8388608 units), asserted <= 8388582.
      * tanh: absolute error <= 2e-7 everywhere.  Measured 8.92e-8.  Below FLT_MIN (the inputs +-1e-40, +-0) the result is +-0: 71362 units of 2^-149 = 1e-40
        itself, covered by the absolute bound.
    (Before this test the cut stood at -87.0, 0.34 above the underflow: exp(x) for x in (-87.3365, -87) came out 0 where the true result is a normal number.)"""
    x = sharp_primitive_inputs()
    assert not np.any(np.isnan(x)) and x.size > 1_000_000
    e, t = np.empty_like(x), np.empty_like(x)
    oracle.lib().mzo_expf(oracle.fptr(x), x.size, oracle.fptr(e))
    oracle.lib().mzo_tanhf(oracle.fptr(x), x.size, oracle.fptr(t))
    ref = np.exp(np.minimum(x.astype(np.float64), 88.0))
    normal = ref >= FLT_MIN
    rel = np.max(np.abs(e[normal].astype(np.float64) - ref[normal]) / ref[normal])
    flush = np.max(np.abs(e[~normal].astype(np.float64) - ref[~normal])) / DENORM
    tref = np.tanh(x.astype(np.float64))
    tabs = np.max(np.abs(t.astype(np.float64) - tref))
    print(f"exp: relative error {rel:.3g} on {normal.sum()} normal results, {flush:.2f} units of 2^-149 on {(~normal).sum()} results below FLT_MIN; tanh: absolute {tabs:.3g}")
    assert rel <= EXP_REL
    assert flush <= EXP_FLUSH_UNITS
    assert tabs <= TANH_ABS
    assert np.all(e >= 0) and np.all(np.abs(t) <= 1) and np.all(np.signbit(t) == np.signbit(x))
    # the branches the inputs are there for: the cut to 0, normal results right above it, the clamp, both tanh cuts
    assert np.any((e == 0) & (x > -88)) and np.any((e > 0) & (e < 2 * FLT_MIN)) and not np.any((e > 0) & (e < FLT_MIN))
    assert np.isfinite(e[x == np.inf][0]) and e[x == np.inf][0] == e[x == np.float32(3e38)][0] and e[x == -np.inf][0] == 0
    assert np.any((np.abs(t) == 1) & (np.abs(x) < 10)) and np.any((np.abs(t) < 1) & (np.abs(x) > 8.6))


def _row_stats(row):
    nz = row[row > 0]
    _, c = np.unique(nz, return_counts=True)
    return int(((row > 0) & (row < FLT_MIN)).sum()), int((row == 0).sum()), int(c[c > 1].sum())


def _forward(oracle, args, net, x):
    return net.forward_az(x)[:3] if args[12] == "alphazero" else net.initial(x)[:3]


@pytest.mark.parametrize("name", sorted(SHARP_SHAPES))
def test_probe_softmax_against_float64(oracle, name):
    """The oracle's softmax on the ladder sharp_logits(A) (policy FC weight 0, bias = the ladder) against a float64 softmax, for every shape of the GPU probes.
      * the logits come out as the ladder's values (-0.0 as +0.0: the FC's chain starts from +0);
      * true prior >= FLT_MIN: relative error <= 2.5e-7 (the exp's bound; the sum of at most 82 non-negative terms and one division add 82 * 2^-24 at most — measured 5.2e-8);
      * true prior < FLT_MIN: absolute error <= 2611589 units of 2^-149.  Measured 2611588.5 on the 82-action rows (1823099 .. 2597064 on the shorter ones, < 1 where
        no exp is cut): the exp returns 0 below ln FLT_MIN, so the error is the largest true prior whose exp is cut, FLT_MIN / sum = 2^23 / 3.21 units;
      * the row holds what it is there for: >= 1 subnormal prior, >= 2 tied non-zero priors and, where the row has room (A >= 26), >= 10 exact zeros (a row of 5,
        9 or 18 actions keeps the two maxima, one subnormal and at least one zero).
    Measured (subnormal, zero, tied): A = 82: (30, 43, 8); 65: (23, 33, 8); 50: (17, 24, 8); 26: (7, 10, 8); 18: (4, 5, 8); 9: (1, 1, 6); 5: (1, 1, 2)."""
    args = SHARP_SHAPES[name]
    d, A = _desc(oracle, args), args[9]
    lg = sharp_logits(A)
    net = oracle.OracleNet(d, probe_heads(d, oracle.gen_weights(d, 0), logits=lg))
    p, l, v = _forward(oracle, args, net, sharp_inputs(args, 3))
    for b in range(3):
        assert np.array_equal(l[b], lg + np.float32(0)) and not np.any(np.signbit(l[b][lg == 0]))
        assert np.array_equal(p[b].view(np.uint32), p[0].view(np.uint32))
    l64 = lg.astype(np.float64)
    ref = np.exp(l64 - l64.max())
    ref /= ref.sum()
    err = np.abs(p[0].astype(np.float64) - ref)
    normal = ref >= FLT_MIN
    sub, zeros, ties = _row_stats(p[0])
    flush = np.max(err[~normal]) / DENORM
    print(f"{name}: A = {A}: {sub} subnormal, {zeros} zero, {ties} tied priors; relative error {np.max(err[normal] / ref[normal]):.3g}, below FLT_MIN {flush:.1f} units")
    assert np.max(err[normal] / ref[normal]) <= EXP_REL
    assert flush <= SOFTMAX_FLUSH_UNITS
    assert sub >= 1 and ties >= 2 and zeros >= (10 if A >= 26 else 1)
    assert abs(float(p[0].sum(dtype=np.float64)) - 1) < 1e-6


def test_bin_ladders_of_the_atari_heads(oracle):
    """The 601-bin value / reward heads on the ladder with its peak at an end bin and at the middle: the decoded scalars are finite, ordered as the peaks are and
    the two heads read their own ladder (the second maximum stays at bin 1: the rows are bimodal, -1401.9 / -328.2 / 14.2 for the peak at bin 0 / 300 / 600)."""
    args = SHARP_SHAPES["atari_1bx32"]
    d = _desc(oracle, args)
    w, x = oracle.gen_weights(d, 0), sharp_inputs(args, 2)
    act = np.zeros((2, 18, 36), np.float32)
    act[0, 3] = act[1, 10] = 1.0
    out = {}
    for vp, rp in ((0, 600), (600, 300), (300, 0)):
        net = oracle.OracleNet(d, probe_heads(d, w, logits=sharp_logits(18), value_bins=sharp_logits(601, peak=vp), reward_bins=sharp_logits(601, peak=rp)))
        p, l, v, h = net.initial(x)
        p2, l2, v2, r2, h2 = net.recurrent(h, act.reshape(2, -1))
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(r2)) and np.array_equal(v, v2) and v[0] == v[1] and r2[0] == r2[1]
        out[vp] = float(v[0])
        out[("r", rp)] = float(r2[0])
    print(out)
    assert out[0] < out[300] < out[600] and out[("r", 0)] == out[0] and out[("r", 600)] == out[600]


def test_gains_reach_their_regimes(oracle):
    """sharpen at the gains of the GPU forwards, batch 64 of the GPU test's inputs.  (64, 16): logits tens apart but no prior underflows to 0, and the tanh values
    saturate (|v| > 0.99 on 9x9 Go 1 x 8, 2x2 Go and TicTacToe).  (512, 4): exact zeros beside live priors.  (4096, 0): nearly one-hot rows (> 75 % of all priors
    exactly 0) and every tanh value exactly 0.
    Measured share of zero priors at (512, 4) / (4096, 0): go9_1bx8 0.66 / 0.98, go9_6bx64 0.29 / 0.97, go7_2bx32 0.76 / 0.98, go9_1bx256 0.87 / 0.98,
    go5_3bx24 0.37 / 0.92, go2_1bx4 0.69 / 0.80, ttt_2bx16 0.72 / 0.88, oth_6bx64 0.55 / 0.97, go7_1bx40_mz 0.59 / 0.97, atari_1bx32 0.56 / 0.83."""
    assert SHARP_GAINS == [(64, 16), (512, 4), (4096, 0)]
    saturated = []
    for name, args in sorted(SHARP_SHAPES.items()):
        d = _desc(oracle, args)
        w, x = oracle.gen_weights(d, 0), sharp_inputs(args, 64)
        for gain in SHARP_GAINS:
            p, l, v = _forward(oracle, args, oracle.OracleNet(d, sharpen(d, w, *gain)), x)
            zero = float((p == 0).mean())
            print(f"{name} {gain}: {zero:.3f} of the priors are 0, logits {l.min():.4g} .. {l.max():.4g}, |v| {np.abs(v).min():.4g} .. {np.abs(v).max():.6g}")
            assert np.all(np.isfinite(p)) and np.all(np.isfinite(l)) and np.all(np.isfinite(v))
            if gain == (64, 16):
                assert zero == 0 and l.max() - l.min() > 15
                if args[12] != "muzero_atari" and np.abs(v).max() > 0.99:
                    saturated.append(name)
            elif gain == (512, 4):
                assert 0.25 < zero < 0.9
            else:
                assert zero > 0.75 and (args[12] == "muzero_atari" or np.all(v == 0))
    assert {"go9_1bx8", "go2_1bx4", "ttt_2bx16"} <= set(saturated)


# what each search of SHARP_SEARCHES has to reach on the oracle: (longest path at least, simulations deeper than 128 levels at least, terminal leaves at least,
# finished games at least).  Measured: see the docstring below.
SEARCH_REACHES = {
    "go9_1bx8_p4096_v0": (164, 300, 200, 0),
    "go9_1bx8_p1024_v8": (164, 200, 100, 0),
    "go9_6bx64_p1024_v8": (60, 0, 500, 0),
    "go7_1bx32_p4096_v0": (100, 0, 50, 0),
    "oth_1bx8_p4096_v0": (60, 0, 200, 0),
    "oth_1bx8_p64_v16": (60, 0, 200, 0),
    "ttt_2bx16_p512_v4": (10, 0, 2000, 8),
    "go9_1bx8_resign_p64_v16": (8, 0, 0, 8),
    "go9_1bx8_mz_puct_p1024_v8": (40, 0, 0, 0),
    "go9_1bx8_mz_gumbel_p1024_v8": (12, 0, 0, 0),
    "atari_1bx32_p512_v4": (2, 0, 0, 0),
}


@pytest.mark.parametrize("name", sorted(SHARP_SEARCHES))
def test_searches_reach_their_depths(oracle, name):
    """The oracle's trace of every search the GPU test runs: `S` lines give the path of each simulation, `E ... cand=` with an empty list a terminal leaf.
    Measured (longest path, simulations deeper than 128 levels, terminal leaves of all simulations, finished games; oracle time):
      go9_1bx8_p4096_v0           164 (the 2 * 81 move cap + root + leaf), 586, 414 of 1604, 0; 0.5 s      go9_1bx8_p1024_v8   164, 436, 261 of 1604, 0; 0.4 s
      go9_6bx64_p1024_v8          73, 0, 954 of 3584, 0; 4.7 s                                             go7_1bx32_p4096_v0  100 (the 2 * 49 move cap), 0, 101 of 804, 0; 0.1 s
      oth_1bx8_p4096_v0           67, 0, 395 of 1212, 0; 0.4 s                                             oth_1bx8_p64_v16    64, 0, 412 of 1212, 0; 0.4 s
      ttt_2bx16_p512_v4           10, 0, 3456 of 4080, 8; 0.1 s                                            go9_1bx8_resign_p64_v16  14, 0, 0 of 816, 18 (every game resigned); 0.1 s
      go9_1bx8_mz_puct_p1024_v8   51, 0, 0, 0; 0.1 s      go9_1bx8_mz_gumbel_p1024_v8  16, 0, 0, 0; 0.1 s      atari_1bx32_p512_v4  2 (n = 4 over 4 sampled actions), 0, 0, 0; 0.1 s
    No case takes the oracle more than 5 s.  With the synthetic weights as they are the longest path of the first case is 59 and no leaf is terminal."""
    conf, args, gain, games, chunks, wseed, _ = SHARP_SEARCHES[name]
    d = _desc(oracle, args)
    og = oracle.OracleGroup(conf + ":program_seed=1:nn_file_name=x.pt:zero_num_threads=1", d, sharpen(d, oracle.gen_weights(d, wseed), *gain))
    og.set_trace(True)
    og.cycles(sum(chunks) + 1)  # the leaf of cycle c is looked at in cycle c + 1
    tr = og.trace()
    plen = np.array([len(l.split("path=")[1].split(",")) for l in tr if l.startswith("S ")])
    ev = [l.split(" ") for l in tr if l.startswith("E ")]
    terminal = sum(1 for f in ev if f[3] == "cand=")
    lines = og.lines()
    print(f"{name}: longest path {plen.max()}, {(plen > 128).sum()} simulations deeper than 128, {terminal} of {len(ev)} leaves terminal, {len(lines)} finished games")
    longest, deep, term, finished = SEARCH_REACHES[name]
    assert plen.max() >= longest and (plen > 128).sum() >= deep and terminal >= term and len(lines) >= finished
    if "resign" in name:  # resigned, not played out: one move long, nobody passed twice
        assert all(l.split(" ")[2] in ("1", "2", "3") for l in lines)
