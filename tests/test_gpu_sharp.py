"""The HIP side at the output ranges of a TRAINED network, bit for bit against the CPU oracle: the deterministic exp / tanh on the device, every heads
implementation on logit ladders with subnormal, zero and tied priors and on saturating values, gain-scaled forwards, and whole searches on sharpened networks
(paths to the move cap, hundreds of terminal leaves, candidate lists of tied zero priors, resignation by the search's own value) on every execution plan.
tests/test_sharp_regime.py checks on the CPU that the oracle is right on these inputs (against float64) and that each input reaches what it is here for.

The synthetic networks of generate_weights, which every other GPU parity test uses, keep the logits within +-0.4 and |v| below 0.3."""
import functools

import numpy as np
import pytest

from helpers import (SHARP_GAINS, SHARP_SEARCHES, SHARP_SHAPES, SHARP_VALUE_PRE, bits, probe_heads, same_bits, sharp_inputs, sharp_logits,
                     sharp_primitive_inputs, sharpen)

pytestmark = pytest.mark.gpu


def _descs(mz, oracle, args):
    kw = dict(vh=args[10], dv=args[11], type_name=args[12])
    return mz.make_desc(*args[:10], **kw), oracle.make_desc(*args[:10], **kw)


def _where(a, b):
    bad = np.nonzero(bits(a).reshape(-1) != bits(b).reshape(-1))[0]
    return f"{bad.size} of {a.size} differ, first at {bad[:4]}: {np.asarray(a).reshape(-1)[bad[:4]]} != {np.asarray(b).reshape(-1)[bad[:4]]}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# a. the two primitives
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_device_exp_tanh_equal_the_oracle(mz, oracle):
    """mz_expf / mz_tanhf of net_dev.h, as every head and every softmax loop calls them, through mz_exp_tanh_device against mzo_expf / mzo_tanhf on
    sharp_primitive_inputs: every float around the cut to 0 (-88 .. -86) and around tanh's cut at 10 and its saturation point near 8.66 (both signs), dense
    sweeps of -104 .. 89 and -12 .. 12, the range of the synthetic networks, zeros, subnormals, infinities, +-3e38.
    NaN is left out: the functions convert rintf(x * log2 e) with static_cast<int>, which is undefined for NaN on the host, so host and device need not agree;
    a NaN logit is outside the contract (no finite weights and planes produce one)."""
    x = sharp_primitive_inputs()
    e, t = mz.exp_tanh_device(x)
    oe, ot = np.empty_like(x), np.empty_like(x)
    oracle.lib().mzo_expf(oracle.fptr(x), x.size, oracle.fptr(oe))
    oracle.lib().mzo_tanhf(oracle.fptr(x), x.size, oracle.fptr(ot))
    assert same_bits(e, oe), "exp: " + _where(e, oe)
    assert same_bits(t, ot), "tanh: " + _where(t, ot)
    with pytest.raises(mz.MzError):
        mz.exp_tanh_device(x[:4], device=99)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# b. the heads on chosen pre-activations, c. on gain-scaled weights
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _actions(args, B):
    P = args[5] * args[6]
    if args[12] == "muzero_atari":
        act = np.zeros((B, 18, P), np.float32)
        for b in range(B):
            act[b, (7 * b + 3) % 18] = 1.0
    else:
        act = np.zeros((B, P), np.float32)
        for b in range(B):
            act[b, (7 * b + 3) % P] = 1.0
    return act.reshape(B, -1)


def _both(args, net, onet, x):
    """every output of the network on both sides: [(name, hip, oracle)]"""
    if args[12] == "alphazero":
        return list(zip(("policy", "logit", "value"), net.forward(x), onet.forward_az(x)))
    a, b = net.initial_inference(x), onet.initial(x)
    out = list(zip(("policy", "logit", "value", "hidden"), a, b))
    act = _actions(args, x.shape[0])
    out += list(zip(("rec policy", "rec logit", "rec value", "reward", "rec hidden"), net.recurrent_inference(b[3], act), onet.recurrent(b[3], act)))
    return out


def _assert_equal(outs, what):
    for name, a, b in outs:
        assert same_bits(a, b), f"{what}: {name}: " + _where(a, b)


@pytest.mark.parametrize("name", sorted(SHARP_SHAPES))
def test_head_probes(mz, oracle, name):
    """Each heads implementation on chosen pre-activations (probe_heads: last layer's weight 0, bias = the vector): the policy head on the ladder sharp_logits (two
    maxima, ties, subnormal and zero priors, logits below the exp's cut), the tanh value on {0, 1e-30, 0.3, 8.6, 8.7, 10, nextafter(10), -11, 3e38} (one reload each),
    the 601-bin value and reward heads of muzero_atari on the ladder with its peak at an end bin and at the middle, the decoded scalars compared as well.
    Batch 3; policy, logits, value (reward, hidden state) bit for bit against the oracle."""
    args = SHARP_SHAPES[name]
    d, od = _descs(mz, oracle, args)
    w, x = mz.generate_weights(d, 0), sharp_inputs(args, 3)
    lg = sharp_logits(args[9])
    if args[12] == "muzero_atari":
        probes = [dict(logits=lg, value_bins=sharp_logits(601, peak=vp), reward_bins=sharp_logits(601, peak=rp)) for vp, rp in ((0, 600), (600, 300), (300, 0))]
    else:
        probes = [dict(logits=lg, value_pre=v) for v in SHARP_VALUE_PRE]
    net = None
    for kw in probes:
        pw = probe_heads(d, w, **kw)
        if net is None:
            net = mz.Net(d, pw)
        else:
            net.reload(pw)
        outs = _both(args, net, oracle.OracleNet(od, pw), x)
        _assert_equal(outs, f"{name} {({k: v for k, v in kw.items() if k == 'value_pre'})}")
        policy = outs[0][1]
        assert np.any((policy > 0) & (policy < 2.0 ** -126)) and np.any(policy == 0), "the ladder no longer reaches subnormal and zero priors"
    if args[12] != "muzero_atari":  # the last probe: tanh(3e38)
        assert np.all(outs[2][1] == 1.0)


@pytest.mark.parametrize("gain", SHARP_GAINS, ids=lambda g: f"p{g[0]}_v{g[1]}")
@pytest.mark.parametrize("name", sorted(SHARP_SHAPES))
def test_gain_scaled_forwards(mz, oracle, name, gain):
    """sharpen(policy gain, value gain) on the synthetic weights: logits tens to thousands apart from real activations (no two rows alike), batch 64 against the
    oracle bit for bit; samples 0, 13 and 63 alone equal their rows of the batch."""
    args = SHARP_SHAPES[name]
    d, od = _descs(mz, oracle, args)
    w = sharpen(d, mz.generate_weights(d, 0), *gain)
    x = sharp_inputs(args, 64)
    net = mz.Net(d, w)
    outs = _both(args, net, oracle.OracleNet(od, w), x)
    _assert_equal(outs, f"{name} {gain}")
    idx = [0, 13, 63]
    if args[12] == "alphazero":
        alone, batch = net.forward(x[idx]), [o[1] for o in outs]
    else:
        alone, batch = net.initial_inference(x[idx]), [o[1] for o in outs[:4]]
    for a, b in zip(alone, batch):
        assert same_bits(a, b[idx]), "a sample alone differs from its row of the batch: " + _where(a, b[idx])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# d. searches
# ---------------------------------------------------------------------------------------------------------------------------------------------------
SEED = ":program_seed=1:nn_file_name=x.pt"


@functools.lru_cache(maxsize=None)
def _oracle_search(name):
    import oracle_lib as O
    conf, args, gain, games, chunks, wseed, _ = SHARP_SEARCHES[name]
    od = O.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
    w = sharpen(od, O.gen_weights(od, wseed), *gain)
    og = O.OracleGroup(conf + SEED + ":zero_num_threads=1", od, w)
    og.cycles(sum(chunks))
    return tuple(og.lines()), tuple(og.peek_records(games)), og.leaf_evals()


SEARCH_RUNS = [(name, variant) for name in sorted(SHARP_SEARCHES) for variant in ("",) + SHARP_SEARCHES[name][6]]


@pytest.mark.parametrize("name,variant", SEARCH_RUNS, ids=lambda v: v.strip(":").replace("=", "_") or "default")
def test_sharp_searches_equal_the_oracle(mz, oracle, name, variant):
    """SHARP_SEARCHES on the default execution plan (the per-game simulation kernel of the shape: asserted to have run), on the lock-step kernels
    (mz_sim_kernel=false) and, for 9x9 Go, with the host rules (mz_device_env=false): finished lines and the records as they stand against the oracle's.
    What the cases reach (tests/test_sharp_regime.py asserts it on the oracle): paths of 164 levels with hundreds of simulations deeper than the 128 remembered
    levels, up to 85 % terminal leaves, priors of which 96 % are exactly 0 (candidate lists of tied zeros), values of exactly 0 and of 0.99.., games resigned by
    the search's own value, MuZero with a PUCT and with a Gumbel root (whole moves per call), and the Gumbel rounds of muzero_atari with sharpened reward bins."""
    conf, args, gain, games, chunks, wseed, _ = SHARP_SEARCHES[name]
    d, _od = _descs(mz, oracle, args)
    w = sharpen(d, mz.generate_weights(d, wseed), *gain)
    olines, orecs, oevals = _oracle_search(name)
    wk = mz.Worker(conf + SEED + ":zero_num_threads=2" + variant, d, w)
    wk.command("start")
    for c in chunks:
        assert wk.run_cycles(c) == c
    st = wk.stats()
    lines, recs = wk.pop_lines(), wk.peek_records(games)
    wk.close()
    assert (st["sim_launches"] > 0) == (variant == ""), (variant, st)
    assert st["leaf_evals"] == oevals
    for i, (a, b) in enumerate(zip(lines, olines)):
        assert a == b, f"line {i} differs:\n  hip   : {a[:400]}\n  oracle: {b[:400]}"
    assert len(lines) == len(olines)
    for g in range(games):
        assert recs[g] == orecs[g], f"game {g}: the record as it stands differs:\n  hip   : {recs[g][:400]}\n  oracle: {orecs[g][:400]}"


@pytest.mark.parametrize("game", ["hex", "gomoku"])
def test_sharp_searches_without_an_oracle(mz, game):
    """Hex 11x11 and Gomoku 15x15 (1 block x 32 channels, sim_kernel_wide) have no oracle: at gain (1024, 8) the three execution paths must write the same lines
    and records, and every finished record must replay legally on the rules model with the right result (the helpers of game_paths.py, test_gpu_hex.py and
    test_gpu_gomoku.py)."""
    import test_gpu_gomoku as TG
    import test_gpu_hex as TH
    from game_paths import run_paths
    sims, games, seed = 16, 8, 1
    if game == "hex":
        n, d, conf = 11, TH._desc(mz, 11, 32, 1), TH._conf(11, True)
    else:
        n, d, conf = 15, TG._desc(mz, 15, 32, 1), TG._conf(15, "standard", True)
    w = sharpen(d, mz.generate_weights(d, seed), 1024, 8)
    conf = f"{conf}:actor_num_simulation={sims}:zero_num_parallel_games={games}:program_seed={seed}:nn_file_name=x.pt:zero_num_threads=2"
    cycles = (sims + 1) * (125 if game == "hex" else 230)  # longer than any game
    lines, recs = run_paths(mz, conf, d, w, games, cycles)
    assert len(lines) >= games
    if game == "hex":
        TH._check_records(lines, n, True)
    else:
        TG._check_records(lines, n, "standard", True)
