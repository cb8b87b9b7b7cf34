"""GPU tests of the opt-in `bf16x3` tower for 128 and 256 hidden channels (9x9 Go AlphaZero; net_bf16_wide_body.h: one LDS tile, layers in place) — the
stand-alone forward against the f32 HIP path and the CPU oracle at the north star's 1e-3, and the worker: the per-game simulation kernel
(sim_kernel_wide_bf16) must write byte for byte the records of the lock-step mode on the same tower.  Not bit-exact against the oracle by design (the
summation order inside a K = 32 MFMA cannot be mirrored on the CPU); the default stays f32.  (Where nothing rounds the order does not matter:
tests/test_gpu_bf16_exact.py checks both bf16x3 bodies bit for bit on exactly representable networks.)"""
import functools
import re

import numpy as np
import pytest

from helpers import SHARP_GAINS, binary_planes, sharpen

pytestmark = pytest.mark.gpu
TOL = 1e-3  # BASELINE.json north_star: "network outputs within 1e-3 fp32" (tests/test_gpu_bf16.py)
# Raw logits, max |bf16x3 - f32| over the batch below, measured on one MI355X: (128, 1) 5.364e-7, (128, 2) 4.061e-7, (256, 1) 4.098e-7, (256, 2) 2.801e-6
# (the logits themselves are within +-0.4).  The difference comes from a summation order that varies with the weights, and four nets are a small sample:
# the bound is 4 x the largest measured value.
LOGIT_TOL = 4 * 2.801e-6
NETS = [(128, 1), (128, 2), (256, 1), (256, 2)]
GO = "env_game=go:env_board_size=9:actor_num_simulation={sims}:zero_num_parallel_games={games}"


def _args(c, blocks, type_name="alphazero"):
    return ("go_9x9", 18, 9, 9, c, 9, 9, 1, blocks, 82, 64, 1, type_name)


def _desc(m, args):
    return m.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])


def _batch():
    """three samples: random 0 / 1 planes, all-zero planes, all-one planes (the largest border and corner sums); three catch a wrong per-sample offset"""
    x = binary_planes(321, (3, 18 * 81))
    x[1] = 0.0
    x[2] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def _forwards(c, blocks):
    """(f32, bf16x3, f32 again, oracle) outputs of one network on _batch(): computed once, shared by the tests"""
    import minizero_amd as mz
    import oracle_lib as O
    d = _desc(mz, _args(c, blocks))
    w = mz.generate_weights(d, 10 + blocks)
    x = _batch()
    net = mz.Net(d, w)
    f32 = net.forward(x)
    net.set_precision("bf16x3")  # without the feature: refused here
    b16 = net.forward(x)
    net.set_precision("f32")
    back = net.forward(x)
    ora = O.OracleNet(_desc(O, _args(c, blocks)), w).forward_az(x)
    return f32, b16, back, ora


@pytest.mark.parametrize("c,blocks", NETS)
def test_forward_within_tolerance(mz, oracle, c, blocks):
    """One and two blocks: the stem, a block's first conv (no skip) and its second (skip), both directions of the in-place hand-over."""
    (p32, l32, v32), (p16, l16, v16), (_, l32b, v32b), (op, ol, ov) = _forwards(c, blocks)
    dl = float(np.max(np.abs(l16 - l32)))
    print(f"{c} channels x {blocks} blocks: max |dpolicy| {np.max(np.abs(p16 - p32)):.2e}, max |dvalue| {np.max(np.abs(v16 - v32)):.2e}, max |dlogit| {dl:.3e}; "
          f"vs oracle: policy {np.max(np.abs(p16 - op)):.2e}, value {np.max(np.abs(v16 - ov)):.2e}")
    assert np.array_equal(l32.view(np.uint32), l32b.view(np.uint32)) and np.array_equal(v32.view(np.uint32), v32b.view(np.uint32)), "switching back restores the f32 bits"
    assert not np.array_equal(l16.view(np.uint32), l32.view(np.uint32)), "the bf16x3 path is a different arithmetic: identical bits mean it did not run"
    for name, a, b in (("policy vs f32", p16, p32), ("value vs f32", v16, v32), ("policy vs oracle", p16, op), ("value vs oracle", v16, ov)):
        err = float(np.max(np.abs(a - b)))
        assert err <= TOL, f"{c} x {blocks}: {name} differs by {err:.3e}"
    assert dl <= LOGIT_TOL, f"{c} x {blocks}: logits differ from the f32 path by {dl:.3e}"
    for s in range(3):  # every sample on its own: a wrong per-sample offset shows as one sample far off
        assert float(np.max(np.abs(p16[s] - p32[s]))) <= TOL


def test_sharp_regime(mz, oracle):
    """The heads of a trained network amplify what the tower leaves: the (128, 1) net with its head weights scaled by the first of SHARP_GAINS (policy FC x 64,
    value FC x 16: logits tens apart, values near saturation — the ranges of tests/test_sharp_regime.py), the same 1e-3 on policy and value.  (The larger gains
    of that list put logits thousands apart: there 1e-3 on the policy needs bit-equal logits, which no reordered sum gives; they are for the bit-exact f32 path.)"""
    gain = SHARP_GAINS[0]
    d, od = _desc(mz, _args(128, 1)), _desc(oracle, _args(128, 1))
    w = sharpen(d, mz.generate_weights(d, 11), *gain)
    x = _batch()
    net = mz.Net(d, w)
    p32, l32, v32 = net.forward(x)
    net.set_precision("bf16x3")
    p16, l16, v16 = net.forward(x)
    op, ol, ov = oracle.OracleNet(od, w).forward_az(x)
    print(f"gain {gain}: logit range {l32.min():.1f} .. {l32.max():.1f}, max |v| {np.max(np.abs(v32)):.3f}; max |dlogit| {np.max(np.abs(l16 - l32)):.2e}, "
          f"max |dpolicy| {np.max(np.abs(p16 - p32)):.2e}, max |dvalue| {np.max(np.abs(v16 - v32)):.2e}")
    assert float(l32.max() - l32.min()) > 10.0, "the gain no longer reaches the sharp regime"
    for name, a, b in (("policy vs f32", p16, p32), ("value vs f32", v16, v32), ("policy vs oracle", p16, op), ("value vs oracle", v16, ov)):
        err = float(np.max(np.abs(a - b)))
        assert err <= TOL, f"sharp {gain}: {name} differs by {err:.3e}"


@pytest.mark.parametrize("c", [128, 256])
def test_reload_rebuilds_the_fragments(mz, c):
    d = _desc(mz, _args(c, 1))
    w1, w2 = mz.generate_weights(d, 1), mz.generate_weights(d, 2)
    x = _batch()
    net = mz.Net(d, w1)
    net.set_precision("bf16x3")
    first = net.forward(x)
    net.reload(w2)
    after = net.forward(x)
    fresh = mz.Net(d, w2)
    fresh.set_precision("bf16x3")
    want = fresh.forward(x)
    for a, b in zip(after, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "stale fragments after reload"
    assert not np.array_equal(first[1].view(np.uint32), after[1].view(np.uint32))


def _play(mz, c, blocks, extra, sims=12, games=4, moves=3):
    d = _desc(mz, _args(c, blocks))
    conf = GO.format(sims=sims, games=games) + f":program_seed=5:nn_file_name=x.pt:zero_num_threads=2:mz_nn_precision=bf16x3{extra}"
    wk = mz.Worker(conf, d, mz.generate_weights(d, 3))
    wk.command("start")
    cycles = (sims + 1) * moves + 2  # (a move's record is written a cycle behind its last simulation)
    assert wk.run_cycles(cycles) == cycles
    st = wk.stats()
    out = (wk.pop_lines(), wk.peek_records(games), st)
    wk.close()
    return out


def _replay(mz, rec):
    env = mz.Env("env_game=go:env_board_size=9")
    env.reset()
    moves = re.findall(r";([BW])\[(\d+)\]", rec)
    assert moves
    for colour, a in moves:
        assert env.turn() == (1 if colour == "B" else 2)
        assert env.legal_mask()[int(a)] and env.act(int(a)), f"illegal move {colour}[{a}] in {rec[:200]}"
    return len(moves)


GUMBEL = ":actor_use_gumbel=true:actor_use_dirichlet_noise=false:actor_gumbel_sample_size=8"


@pytest.mark.parametrize("root", ["", GUMBEL], ids=["puct", "gumbel"])
@pytest.mark.parametrize("c,blocks", [(128, 2), (256, 1)])
def test_simulation_kernel_equals_lock_step(mz, c, blocks, root):
    """Both plans run the same tower body in the same order: lines and records byte for byte, no tolerance.  This is the check that the tower inside
    sim_kernel_wide_bf16 is the stand-alone one."""
    la, ra, sa = _play(mz, c, blocks, root)
    lb, rb, sb = _play(mz, c, blocks, root + ":mz_sim_kernel=false")
    assert sa["sim_launches"] > 0, "the per-game simulation kernel did not run on the default plan"
    assert sb["sim_launches"] == 0
    assert sa["leaf_evals"] == sb["leaf_evals"] == (13 * 3 + 2) * 4
    assert la == lb
    for g, (a, b) in enumerate(zip(ra, rb)):
        assert a == b, f"game {g}: records differ:\n  sim kernel: {a[:400]}\n  lock-step : {b[:400]}"
    assert len(ra) == 4 and all(_replay(mz, r) >= 3 for r in ra)


def test_plan_at_400_simulations(mz):
    """The 256-channel tile is 128 KB: at the reference's search size the plan gives up optional LDS blocks, or the worker comes up in lock-step mode on
    the bf16x3 tower — either way it is created and finishes a move; no error at the first launch."""
    d = _desc(mz, _args(256, 1))
    wk = mz.Worker(GO.format(sims=400, games=2) + ":program_seed=1:nn_file_name=x.pt:zero_num_threads=2:mz_nn_precision=bf16x3", d, mz.generate_weights(d, 0))
    wk.command("start")
    assert wk.run_cycles(401 + 2) == 403
    st = wk.stats()
    print(f"256 channels, n = 400: sim_launches {st['sim_launches']}")
    assert st["moves"] == 2 and st["leaf_evals"] == 403 * 2
    assert all(_replay(mz, r) >= 1 for r in wk.peek_records(2))


REFUSED = [("go_9x9", 18, 9, 9, 32, 9, 9, 1, 1, 82, 64, 1, "alphazero"), ("go_7x7", 18, 7, 7, 128, 7, 7, 1, 1, 50, 64, 1, "alphazero"),
           ("go_19x19", 18, 19, 19, 64, 19, 19, 1, 1, 362, 64, 1, "alphazero"), ("othello_8x8", 4, 8, 8, 256, 8, 8, 1, 1, 65, 64, 1, "alphazero"),
           _args(128, 1, "muzero")]


@pytest.mark.parametrize("args", REFUSED, ids=lambda a: f"{a[0]}_{a[4]}_{a[12]}")
def test_still_refused_by_name(mz, args):
    d = _desc(mz, args)
    net = mz.Net(d, mz.generate_weights(d, 0))
    with pytest.raises(mz.MzError, match="128 / 256 hidden channels on 9x9"):
        net.set_precision("bf16x3")


def test_worker_refuses_muzero(mz):
    d = _desc(mz, _args(128, 1, "muzero"))
    conf = "env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=8:zero_num_parallel_games=2:program_seed=1:mz_nn_precision=bf16x3"
    with pytest.raises(mz.MzError, match="bf16x3"):
        mz.Worker(conf, d, mz.generate_weights(d, 0))
