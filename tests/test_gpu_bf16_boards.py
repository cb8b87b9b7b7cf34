"""GPU tests of the opt-in `bf16x3` tower for 64 hidden channels on 11x11 and 15x15 boards — Gomoku, Hex, Havannah edge size 8 (net_bf16_wide_body.h with two
pixel groups; sim_kernel_wide_bf16 in sim_wide_k / _l / _m.hip).  11x11 is the even split of the pixel tiles without a corner tile, 15x15 the uneven one
(8 + 7) with one.  As tests/test_gpu_bf16_exact.py does for 9x9: on the exactly representable networks of tests/exact_nets_boards.py (whose conditions
tests/test_exact_nets_boards.py asserts without a GPU) the towers equal a float64 reference bit for bit and the worker's records under bf16x3 equal the f32
mode's byte for byte — in the per-game simulation kernel and in the lock-step mode; on ordinary networks the outputs are within the 1e-3 that config.h states,
and within a bound derived from the reference at trained-network ranges.  The f32 side of the worker is held to the search model by
tests/test_gpu_search_model_games.py; no model run is needed here."""
import functools
import re

import numpy as np
import pytest

import exact_nets as E
import exact_nets_boards as B
from helpers import blob_manifest

pytestmark = pytest.mark.gpu
TOL = 1e-3  # BASELINE.json north_star: "network outputs within 1e-3 fp32" (config.h mz_nn_precision)


def _desc(lib, args):
    return lib.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])


def _first_difference(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    s, c, p = (int(v) for v in bad[0])
    per_sample = [int(np.count_nonzero(got[i].view(np.uint32) != want[i].view(np.uint32))) for i in range(got.shape[0])]
    return (f"{len(bad)} of {got.size} values differ (per sample {per_sample}); first at sample {s}, channel {c}, position {p}: got {got[s, c, p]!r}, "
            f"want {want[s, c, p]!r}, difference {float(got[s, c, p]) - float(want[s, c, p]):.0f}")


# ---------------------------------------------------------------------------------------------
# the tower and the forward on dense exact nets
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_run(shape, kind):
    """everything the dense-net tests look at, from ONE Net object: towers and forwards at both precisions, and — after a reload of a generate_weights blob on
    the same object — its logits at both precisions"""
    import minizero_amd as mz
    net = B.dense_net(shape, kind)
    d = _desc(mz, net.args)
    x = E.batch(net.args)
    n = mz.Net(d, net.blob(heads_from=mz.generate_weights(d, 3)))
    t32, f32 = n.tower(x), n.forward(x)
    n.set_precision("bf16x3")  # without the feature: refused here
    t16, f16 = n.tower(x), n.forward(x)
    # (seed 2: these shapes have ONE policy-conv plane, and on some seeds — 4 and 7 among them, in float64 — its ReLU passes nothing, the logits are the FC's
    # bias at any precision and say nothing about the tower; at seed 2 the plane is alive on every shape with one block and with two)
    n.reload(mz.generate_weights(d, 2))
    g16 = n.forward(x)[1]
    n.set_precision("f32")
    g32 = n.forward(x)[1]
    n.close()
    return net.reference(x), t32, t16, f32, f16, g32, g16


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape,kind", B.DENSE_CASES)
def test_tower_equals_the_float64_reference(mz, shape, kind, precision):
    """wide_stem: lo_w in the stem, then hi_w * lo_a in both tower layers; wide_conv1: lo_w * hi_a in a tower layer, then hi_w * lo_a with the skip; narrow2:
    the hand-over of x between two blocks and the fragments' ring (two taps per round at 64 channels) across four tower layers.  Compared as uint32, every
    sample alone: a pixel tile given to the wrong group, the corner tile's taps, or a ring slot holding another tap's fragments are whole-number errors."""
    ref, t32, t16 = _dense_run(shape, kind)[:3]
    got = t32 if precision == "f32" else t16
    assert got.shape == ref.shape and got.dtype == np.float32
    for s in range(ref.shape[0]):
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), f"{shape} {kind} {precision}, sample {s}: " + _first_difference(got, ref)


@pytest.mark.parametrize("shape,kind", B.DENSE_CASES)
def test_forward_bits_are_those_of_the_f32_path(mz, shape, kind):
    _, _, _, f32, f16, g32, g16 = _dense_run(shape, kind)
    for name, a, b in zip(("policy", "logit", "value"), f16, f32):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{shape} {kind}: {name} bits differ between bf16x3 and f32 on an exact network"
    assert np.all(np.isfinite(f32[1])) and np.all(np.isfinite(f32[2]))
    # ... and not because the switch did nothing: on an ordinary network the same object's bf16x3 logits are another arithmetic's
    assert not np.array_equal(g16.view(np.uint32), g32.view(np.uint32)), "identical bits on a generate_weights network: the bf16x3 tower did not run"


# ---------------------------------------------------------------------------------------------
# ordinary networks: the 1e-3 of config.h, a derived bound at trained-network ranges, reload
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(B.SHAPES))
def test_forward_within_tolerance(mz, shape):
    """generate_weights, two blocks: policy and value within 1e-3 of the f32 path, every sample on its own; switching back restores the f32 bits"""
    args = B.args_of(shape, 2)
    d = _desc(mz, args)
    x = E.batch(args)
    net = mz.Net(d, mz.generate_weights(d, 12))
    p32, l32, v32 = net.forward(x)
    net.set_precision("bf16x3")
    p16, l16, v16 = net.forward(x)
    net.set_precision("f32")
    _, l32b, v32b = net.forward(x)
    net.close()
    print(f"{shape}: max |dpolicy| {np.max(np.abs(p16 - p32)):.2e}, max |dvalue| {np.max(np.abs(v16 - v32)):.2e}, max |dlogit| {np.max(np.abs(l16 - l32)):.3e}")
    assert np.array_equal(l32.view(np.uint32), l32b.view(np.uint32)) and np.array_equal(v32.view(np.uint32), v32b.view(np.uint32)), "switching back restores the f32 bits"
    assert not np.array_equal(l16.view(np.uint32), l32.view(np.uint32)), "the bf16x3 path is a different arithmetic: identical bits mean it did not run"
    for s in range(3):
        assert float(np.max(np.abs(p16[s] - p32[s]))) <= TOL and float(np.max(np.abs(v16[s] - v32[s]))) <= TOL, f"{shape}, sample {s}"


# (shape, blocks, weight seed, factor on every tower layer's bn_g): the factors bring the last activations' maximum to 1e2 .. 1e3 (asserted on the reference)
RANGED = [("gomoku15x64", 2, 12, 6.0), ("hex11x64", 2, 12, 6.0), ("havannah15x64", 2, 12, 6.0)]


@pytest.mark.parametrize("shape,blocks,seed,gain", RANGED)
def test_bf16x3_error_within_the_derived_bound(mz, shape, blocks, seed, gain):
    """As tests/test_gpu_bf16_exact.py: |bf16x3 tower - float64 reference| <= E elementwise, E from the reference alone (exact_nets.bf16x3_error_bound; no
    measured constant), on generate_weights networks with the tower's bn_g raised until the activations reach a trained network's 1e2 .. 1e3."""
    args = B.args_of(shape, blocks)
    d = _desc(mz, args)
    w = mz.generate_weights(d, seed)
    for name, off, n in blob_manifest(E.manifest_desc(args)):
        if name.startswith("repr.") and name.endswith(".bn_g"):
            w[off:off + n] *= np.float32(gain)
    x = E.batch(args)
    ref, bound = E.bf16x3_error_bound(E.fold(args, w), x, args[5], args[6])
    assert 1e2 <= ref.max() <= 1e3, f"the activations' maximum {ref.max():.1f} has left 1e2 .. 1e3"
    n = mz.Net(d, w)
    t32 = n.tower(x).astype(np.float64)
    n.set_precision("bf16x3")
    t16 = n.tower(x).astype(np.float64)
    n.close()
    e16, e32 = np.abs(t16 - ref), np.abs(t32 - ref)
    live = bound > 0
    print(f"{shape} x {blocks}: activations up to {ref.max():.1f}; bf16x3: max error {e16.max():.3e}, largest error / bound {np.max(e16[live] / bound[live]):.3e}; "
          f"f32 path: max error {e32.max():.3e}; bound up to {bound.max():.3e}")
    assert np.all(e16 <= bound), f"{shape} x {blocks}: error above the bound at {np.argwhere(e16 > bound)[0]}, {e16.max():.3e}"


@pytest.mark.parametrize("shape", list(B.SHAPES))
def test_reload_rebuilds_the_fragments(mz, shape):
    args = B.args_of(shape, 1)
    d = _desc(mz, args)
    w1, w2 = mz.generate_weights(d, 1), mz.generate_weights(d, 2)
    x = E.batch(args)
    net = mz.Net(d, w1)
    net.set_precision("bf16x3")
    first = net.forward(x)
    net.reload(w2)
    after = net.forward(x)
    net.close()
    fresh = mz.Net(d, w2)
    fresh.set_precision("bf16x3")
    want = fresh.forward(x)
    fresh.close()
    for a, b in zip(after, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "stale fragments after reload"
    assert not np.array_equal(first[1].view(np.uint32), after[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------
# the worker, on networks that are exact for every position
# ---------------------------------------------------------------------------------------------
# (no resignation: on some of these nets the value head of generate_weights saturates and the games would end before their first move)
COMMON = ":actor_num_simulation=12:zero_num_parallel_games=4:program_seed=5:nn_file_name=x.pt:actor_resign_threshold=-2:zero_num_threads=2"
GAMES = {
    "gomoku15x64": "env_game=gomoku:env_board_size=15:env_gomoku_rule=standard:env_gomoku_exactly_five_stones=true",
    "hex11x64": "env_game=hex:env_board_size=11:env_hex_use_swap_rule=true",
    "havannah15x64": "env_game=havannah:env_board_size=8:env_havannah_use_swap_rule=true",
}
GUMBEL = ":actor_use_gumbel=true:actor_use_dirichlet_noise=false:actor_gumbel_sample_size=8"
ROOTS = {"puct": "", "gumbel": GUMBEL}
CYCLES = 13 * 3 + 2  # 12 simulations, 3 moves (a move's record is written a cycle behind its last simulation)


@functools.lru_cache(maxsize=None)
def _play(shape, kind, shift, root, precision, lock_step):
    import minizero_amd as mz
    net = B.certified_net(shape, kind, shift)
    d = _desc(mz, net.args)
    w = net.blob(heads_from=mz.generate_weights(d, 3))
    conf = GAMES[shape] + COMMON + ROOTS[root] + f":mz_nn_precision={precision}" + (":mz_sim_kernel=false" if lock_step else "")
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    assert wk.run_cycles(CYCLES) == CYCLES
    st = wk.stats()
    out = (wk.pop_lines(), wk.peek_records(4), st["sim_launches"], st["leaf_evals"])
    wk.close()
    return out


@pytest.mark.parametrize("lock_step", [False, True], ids=["sim_kernel", "lock_step"])
@pytest.mark.parametrize("root", list(ROOTS))
@pytest.mark.parametrize("shape,kind,shift", B.CERTIFIED_CASES)
def test_worker_records_equal_the_f32_mode(mz, shape, kind, shift, root, lock_step):
    """Certified nets (exact for every 0 / 1 input), last tower layer times 2^-shift, heads of generate_weights: the towers put out the same bits at both
    precisions for every leaf, the heads and the search are shared code, so lines and records are equal byte for byte — in the per-game simulation kernels
    (sim_kernel_wide_bf16 against sim_kernel_wide) and in the lock-step mode.  Hex plays with the swap rule on."""
    la, ra, sa, ea = _play(shape, kind, shift, root, "bf16x3", lock_step)
    lb, rb, sb, eb = _play(shape, kind, shift, root, "f32", lock_step)
    if lock_step:
        assert sa == 0 and sb == 0
    else:
        assert sa > 0 and sb > 0, "the per-game simulation kernel did not run on the default plan"
    assert ea == eb and ea > 0
    assert la == lb
    assert len(ra) == 4 and all(len(re.findall(r";[BW]\[\d+\]", r)) >= 3 for r in ra), ra[0][:300]
    for g, (a, b) in enumerate(zip(ra, rb)):
        assert a == b, f"{shape} {kind} {root}, game {g}: records differ:\n  bf16x3: {a[:400]}\n  f32   : {b[:400]}"


# ---------------------------------------------------------------------------------------------
# what stays refused
# ---------------------------------------------------------------------------------------------
REFUSED = [("havannah4x4", 20, 7, 7, 32, 7, 7, 1, 1, 49, 32, 1, "alphazero"), ("go_13x13", 18, 13, 13, 64, 13, 13, 1, 1, 170, 64, 1, "alphazero"),
           ("gomoku_15x15", 4, 15, 15, 32, 15, 15, 1, 1, 225, 32, 1, "alphazero"), ("gomoku_15x15", 4, 15, 15, 64, 15, 15, 1, 1, 225, 32, 1, "muzero")]


@pytest.mark.parametrize("args", REFUSED, ids=lambda a: f"{a[0]}_{a[4]}_{a[12]}")
def test_still_refused_by_name(mz, args):
    """(19x19 x 64: tests/test_gpu_bf16_wide.py)"""
    d = _desc(mz, args)
    net = mz.Net(d, mz.generate_weights(d, 0))
    with pytest.raises(mz.MzError, match="bf16x3"):
        net.set_precision("bf16x3")
    net.close()
