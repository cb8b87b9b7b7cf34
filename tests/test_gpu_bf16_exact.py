"""Bit-exact GPU tests of the towers — the f32 paths and the opt-in bf16x3 bodies (net_bf16_body.h: 64 channels; net_bf16_wide_body.h, sim_wide_bf16.inc: 128 /
256 channels) — on the exactly representable networks of tests/exact_nets.py.  The design note that a CPU cannot mirror the summation order inside a K = 32 MFMA
does not bite where every product and every partial sum is representable: then any order gives the same bits, the towers must equal a float64 reference bit
for bit, and an operand taken from the wrong tap or k-block, or one of the three products dropped, is a whole-number error.  (tests/test_exact_nets.py asserts,
without a GPU, that the networks used here meet the conditions.)  What the heads blur is looked at directly: Net.tower() (mz_net_tower_az).

Tried once on scratch builds: with the hi_w * lo_a MFMAs removed from the tower layers of wideLayerBf16, every bf16x3 tower, forward and worker test of this file
at 128 / 256 channels fails; with the lo_w * hi_a MFMAs removed, those on the wide_conv1 nets (the only ones with lo_w in a tower layer) fail."""
import functools
import re

import numpy as np
import pytest

import exact_nets as E
from helpers import blob_manifest

pytestmark = pytest.mark.gpu


def _desc(lib, args):
    return lib.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])


def _first_difference(got, want):
    """(text) the first differing (sample, channel, position) and the difference there; the networks' values are whole numbers, so is the difference"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    s, c, p = (int(v) for v in bad[0])
    per_sample = [int(np.count_nonzero(got[i].view(np.uint32) != want[i].view(np.uint32))) for i in range(got.shape[0])]
    return (f"{len(bad)} of {got.size} values differ (per sample {per_sample}); first at sample {s}, channel {c}, position {p}: got {got[s, c, p]!r}, "
            f"want {want[s, c, p]!r}, difference {float(got[s, c, p]) - float(want[s, c, p]):.0f}")


@functools.lru_cache(maxsize=None)
def _dense_run(shape, kind):
    """everything the dense-net tests look at, from ONE Net object: towers and forwards at both precisions, and — after a reload of a generate_weights blob on
    the same object — its logits at both precisions"""
    import minizero_amd as mz
    net = E.dense_net(shape, kind)
    d = _desc(mz, net.args)
    x = E.batch(net.args)
    n = mz.Net(d, net.blob(heads_from=mz.generate_weights(d, 3)))
    t32, f32 = n.tower(x), n.forward(x)
    n.set_precision("bf16x3")
    t16, f16 = n.tower(x), n.forward(x)
    n.reload(mz.generate_weights(d, 4))
    g16 = n.forward(x)[1]
    n.set_precision("f32")
    g32 = n.forward(x)[1]
    n.close()
    return net.reference(x), t32, t16, f32, f16, g32, g16


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("shape,kind", E.DENSE_CASES)
def test_tower_equals_the_float64_reference(mz, shape, kind, precision):
    """wide_stem: lo_w in the stem (which has no lo input), then hi_w * lo_a in both tower layers; wide_conv1: lo_w * hi_a in a tower layer, then hi_w * lo_a
    with the skip; narrow2: the hand-over of x between two blocks and the fragments' ring across four tower layers.  Compared as uint32, every sample alone."""
    ref, t32, t16 = _dense_run(shape, kind)[:3]
    got = t32 if precision == "f32" else t16
    assert got.shape == ref.shape and got.dtype == np.float32
    for s in range(ref.shape[0]):
        assert np.array_equal(got[s].view(np.uint32), ref[s].view(np.uint32)), f"{shape} {kind} {precision}, sample {s}: " + _first_difference(got, ref)


@pytest.mark.parametrize("shape,kind", E.DENSE_CASES)
def test_forward_bits_are_those_of_the_f32_path(mz, shape, kind):
    _, _, _, f32, f16, g32, g16 = _dense_run(shape, kind)
    for name, a, b in zip(("policy", "logit", "value"), f16, f32):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{shape} {kind}: {name} bits differ between bf16x3 and f32 on an exact network"
    assert np.all(np.isfinite(f32[1])) and np.all(np.isfinite(f32[2]))
    # ... and not because the switch did nothing: on an ordinary network the same object's bf16x3 logits are another arithmetic's
    assert not np.array_equal(g16.view(np.uint32), g32.view(np.uint32)), "identical bits on a generate_weights network: the bf16x3 tower did not run"


# ---------------------------------------------------------------------------------------------
# the worker, on networks that are exact for every position
# ---------------------------------------------------------------------------------------------
# (no resignation: on some of these nets the value head of generate_weights saturates at -1 and the games would end before their first move)
GO = "env_game=go:env_board_size=9:actor_num_simulation=12:zero_num_parallel_games=4:program_seed=5:nn_file_name=x.pt:actor_resign_threshold=-2"
GUMBEL = ":actor_use_gumbel=true:actor_use_dirichlet_noise=false:actor_gumbel_sample_size=8"
ROOTS = {"puct": "", "gumbel": GUMBEL}
CYCLES = 13 * 3 + 2  # 12 simulations, 3 moves (a move's record is written a cycle behind its last simulation)


def _certified_blob(mz, shape, kind, shift):
    net = E.certified_net(shape, kind, shift)
    d = _desc(mz, net.args)
    return net, d, net.blob(heads_from=mz.generate_weights(d, 3))


@functools.lru_cache(maxsize=None)
def _play(shape, kind, shift, root, precision, lock_step):
    import minizero_amd as mz
    net, d, w = _certified_blob(mz, shape, kind, shift)
    conf = GO + ROOTS[root] + f":zero_num_threads=2:mz_nn_precision={precision}" + (":mz_sim_kernel=false" if lock_step else "")
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    assert wk.run_cycles(CYCLES) == CYCLES
    st = wk.stats()
    out = (wk.pop_lines(), wk.peek_records(4), st["sim_launches"], st["leaf_evals"])
    wk.close()
    return out


@pytest.mark.parametrize("lock_step", [False, True], ids=["sim_kernel", "lock_step"])
@pytest.mark.parametrize("root", list(ROOTS))
@pytest.mark.parametrize("shape,kind,shift", E.CERTIFIED_CASES)
def test_worker_records_equal_the_f32_mode(mz, shape, kind, shift, root, lock_step):
    """Certified nets (exact for every 0 / 1 input), last tower layer times 2^-shift, heads of generate_weights: the towers put out the same bits at both precisions
    for every leaf, the heads and the search are shared code, so lines and records are equal byte for byte — in the per-game simulation kernels (sim_kernel
    <..., BF = true> at 64 channels, which takes networks of any depth; sim_kernel_wide_bf16 at 128 / 256) and in the lock-step mode."""
    la, ra, sa, ea = _play(shape, kind, shift, root, "bf16x3", lock_step)
    lb, rb, sb, eb = _play(shape, kind, shift, root, "f32", lock_step)
    if lock_step:
        assert sa == 0 and sb == 0
    else:
        assert sa > 0 and sb > 0, "the per-game simulation kernel did not run on the default plan"
    assert ea == eb == CYCLES * 4
    assert la == lb
    assert len(ra) == 4 and all(len(re.findall(r";[BW]\[\d+\]", r)) >= 3 for r in ra)
    for g, (a, b) in enumerate(zip(ra, rb)):
        assert a == b, f"{shape} {kind} {root}, game {g}: records differ:\n  bf16x3: {a[:400]}\n  f32   : {b[:400]}"


@pytest.mark.parametrize("root", list(ROOTS))
@pytest.mark.parametrize("shape", ["go9x64", "go9x128"])
def test_worker_records_equal_the_oracle(mz, oracle, shape, root):
    """The first oracle parity a bf16x3 simulation kernel can have: on the certified one-block wide-conv1 nets the records under mz_nn_precision=bf16x3 are the
    CPU oracle's."""
    kind, shift = next((k, s) for sh, k, s in E.CERTIFIED_CASES if sh == shape and k == "wide_conv1")
    net, d, w = _certified_blob(mz, shape, kind, shift)
    lines, recs, sims, evals = _play(shape, kind, shift, root, "bf16x3", False)
    og = oracle.OracleGroup(GO + ROOTS[root] + ":zero_num_threads=1", _desc(oracle, net.args), w)
    og.cycles(CYCLES)
    assert sims > 0 and evals == og.leaf_evals()
    assert lines == og.lines()
    for g, (a, b) in enumerate(zip(recs, og.peek_records(4))):
        assert a == b, f"{shape} {root}, game {g}: records differ:\n  bf16x3: {a[:400]}\n  oracle: {b[:400]}"


# ---------------------------------------------------------------------------------------------
# a derived bound at trained-network ranges
# ---------------------------------------------------------------------------------------------
# (shape, blocks, weight seed, factor on every tower layer's bn_g): the factors bring the last activations' maximum to 1e2 .. 1e3 (asserted on the reference)
RANGED = [("go9x128", 2, 12, 6.0), ("go9x256", 1, 11, 8.0), ("go9x64", 2, 12, 6.0)]


@pytest.mark.parametrize("shape,blocks,seed,gain", RANGED)
def test_bf16x3_error_within_the_derived_bound(mz, shape, blocks, seed, gain):
    """generate_weights networks with the tower's bn_g raised until the activations reach 1e2 .. 1e3 (a trained network's range; generate_weights alone gives
    O(1)): |bf16x3 tower - float64 reference| <= E elementwise, E from the reference alone (exact_nets.bf16x3_error_bound; no measured constant).  E is a
    worst-case bound (|W| through every layer), far above what random signs leave.  Largest error / bound ratios seen on one MI355X, for the record (no gate):
    go9x128 x 2: 7.0e-7 (max error 6.7e-3 at activations up to 372), go9x256 x 1: 1.7e-4 (1.8e-3, 243), go9x64 x 2: 3.9e-6 (6.0e-3, 480)."""
    args = E.args_of(shape, blocks)
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
