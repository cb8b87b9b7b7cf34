"""The networks of tests/exact_nets_boards.py (Gomoku 15x15, Hex 11x11, Havannah 15x15, 64 channels), checked without a GPU as tests/test_exact_nets.py
checks the 9x9 ones: for every network that tests/test_gpu_bf16_boards.py runs, the validity conditions (under which the f32 path, the bf16x3 path and a
float64 sum must agree bit for bit) and the coverage conditions (under which a lost or misplaced partial product of any fragment cannot hide) hold.  The
numbers asserted are the caps of tests/test_exact_nets.py, set beforehand, not measurements of a kernel."""
import functools

import numpy as np
import pytest

import exact_nets as E
import exact_nets_boards as B


def test_shapes_are_the_games():
    """planes and actions of the three games (game_kind.h kGameTable: Gomoku and Hex 4 planes, Havannah 20; no pass action; Havannah's edge size 8 plays on a
    15x15 array), 64 hidden channels, the three variants of exact_nets"""
    got = {k: (v[1], v[2], v[3], v[4], v[9]) for k, v in B.SHAPES.items()}
    assert got == {"gomoku15x64": (4, 15, 15, 64, 225), "hex11x64": (4, 11, 11, 64, 121), "havannah15x64": (20, 15, 15, 64, 225)}
    assert set(B.KINDS) == {"wide_stem", "wide_conv1", "narrow2"}
    assert len(B.DENSE_CASES) == 9 and len(B.CERTIFIED_CASES) == 6


@functools.lru_cache(maxsize=None)
def _report(shape, kind):
    net = B.dense_net(shape, kind)
    return net, E.validity(net, E.batch(net.args))


@pytest.mark.parametrize("shape,kind", B.DENSE_CASES)
def test_dense_net_is_valid_and_covers(shape, kind):
    net, r = _report(shape, kind)
    print(f"{net.name}: largest layer input {r['max_in']:.0f}, largest sum |w||a| {r['max_abs_sum']:.3g}, lo fractions {np.round(r['lo_frac'], 3)}, "
          f"ReLU survival {np.round(r['relu_frac'], 2)}, non-zero output channels {r['nonzero_channels']:.3f}")
    assert len(net.ints) == 1 + 2 * B.KINDS[kind] and net.wide == [(kind, l) in (("wide_stem", 0), ("wide_conv1", 1)) for l in range(len(net.ints))]
    assert net.ints[0][0].shape == (64, net.args[1], 9) and all(w.shape == (64, 64, 9) for w, b in net.ints[1:])
    assert r["ok"] and r["max_lolo"] == 0.0 and r["max_abs_sum"] < 2 ** 24
    for l, ((w, b), wide) in enumerate(zip(net.ints, net.wide)):
        assert E.fragment_coverage(w.astype(np.float64), wide) == 1.0, f"layer {l}: a fragment without a non-zero hi" + (" and lo" if wide else "")
        assert (E.split(w.astype(np.float64))[1] != 0).any() == wide
        assert set(np.unique(b)) <= {0, 1, 2}
    for l in E.lo_layers(kind):
        assert r["lo_frac"][l] >= 0.05, f"layer {l}: only {r['lo_frac'][l]:.3f} of the input activations have a lo"
    assert r["nonzero_channels"] >= 0.95
    assert all(0.4 <= f <= 0.6 for f in r["relu_frac"]), r["relu_frac"]


@pytest.mark.parametrize("shape,kind", B.DENSE_CASES)
def test_blob_folds_back_to_the_integers(shape, kind):
    net = B.dense_net(shape, kind)
    blob = net.blob()
    assert blob.dtype == np.float32 and np.all(np.isfinite(blob))
    for (w, b), (fw, fb) in zip(net.layers(), E.fold(net.args, blob)):
        assert np.array_equal(w, fw) and np.array_equal(b, fb)


@pytest.mark.parametrize("shape,kind,shift", B.CERTIFIED_CASES)
def test_certified_net_is_valid_for_every_input(shape, kind, shift):
    net = B.certified_net(shape, kind, shift)
    ok, bounds, worst = E.certificate(net)
    print(f"{net.name}: worst-case layer inputs {bounds}, worst sum {worst:.4g} grid units (2^{np.log2(worst):.2f})")
    assert ok and worst < 2 ** 24 and max(bounds) <= 2 ** 17
    for l, ((w, b), wide) in enumerate(zip(net.ints, net.wide)):
        assert int(np.count_nonzero(w.reshape(w.shape[0], -1), axis=1).max()) <= E.CERT_NNZ
        assert E.fragment_coverage(w.astype(np.float64), wide) >= 0.75
        if wide:
            assert bounds[l] <= 256, "a wide layer's inputs must all be bf16 (lo_w * lo_a is what the kernel leaves out)"
    x = E.batch(net.args)
    r = E.validity(net, x)
    assert r["ok"] and r["max_in"] <= max(bounds) and r["max_abs_sum"] <= worst
    for (w, b), (fw, fb) in zip(net.layers(), E.fold(net.args, net.blob())):
        assert np.array_equal(w, fw) and np.array_equal(b, fb)
    assert 2.0 ** -5 <= float(r["out"].mean()) <= 2.0 ** 5, "what the heads read is no longer O(1)"


def test_a_broken_net_is_noticed():
    """the checkers bite on these shapes too: a wide weight behind activations that need a lo, and a sum past 2^24"""
    net = B.dense_net("hex11x64", "wide_stem")
    w, b = net.ints[1]
    w2 = w.copy()
    w2[w2 != 0] = 257
    bad = E.ExactNet("bad", net.args, [net.ints[0], (w2, b), net.ints[2]], [True, True, False])
    r = E.validity(bad, E.batch(net.args))
    assert not r["ok"] and r["max_lolo"] > 0
    cert = B.certified_net("gomoku15x64", "narrow2", 7)
    big = E.ExactNet("big", cert.args, [(w * 64, b) for w, b in cert.ints], cert.wide, 7)
    assert not E.certificate(big)[0]
