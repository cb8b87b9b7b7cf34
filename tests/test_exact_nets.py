"""The constructions of tests/exact_nets.py, checked without a GPU: for every network that tests/test_gpu_bf16_exact.py runs, the validity conditions (under
which the f32 path, the bf16x3 path, the oracle and a float64 sum must agree bit for bit) and the coverage conditions (under which a lost or misplaced partial
product of any fragment cannot hide) hold.  The coverage numbers are caps set beforehand, not measurements of a kernel."""
import functools

import numpy as np
import pytest

import exact_nets as E


def test_number_facts_the_constructions_rest_on():
    one = np.float32(1.0)
    assert E.BN_V_ONE + np.float32(1e-5) == one and one / np.sqrt(E.BN_V_ONE + np.float32(1e-5), dtype=np.float32) == one
    v4 = np.float32(4.0 - 1e-5)
    assert one / np.sqrt(v4 + np.float32(1e-5), dtype=np.float32) == np.float32(0.5)
    n = np.arange(-2 ** 17, 2 ** 17 + 1, dtype=np.float64)
    hi, lo, exact = E.split(n)
    assert exact, "every integer of magnitude <= 2^17 is hi + lo"
    assert not lo[np.abs(n) <= 256].any(), "every integer of magnitude <= 256 is a bf16"
    assert not E.split(np.array([2.0 ** 17 + 257]))[2], "(and the checker does notice a value that is not)"
    assert not E.split(E.NARROW)[1].any() and E.split(E.WIDE)[1].all() and E.split(E.WIDE)[2] and len(E.WIDE) >= 4
    # the rounding is to nearest, ties to even (bf16_split.h bf16Rne): 257 -> 256, 259 -> 260 (tie), 383 -> 384 (tie), 385 -> 384 (tie)
    assert list(E.bf16_rne(np.array([257, 259, 383, 385, -259], np.float32))) == [256, 260, 384, 384, -260]


def test_reference_conv_against_plain_loops():
    H, W, cin, cout = 4, 5, 3, 2
    a = (np.arange(2 * cin * H * W) % 7 - 3).astype(np.float64).reshape(2, cin, H * W)
    w = (np.arange(cout * cin * 9) % 5 - 2).astype(np.float64).reshape(cout, cin, 9)
    want = np.zeros((2, cout, H * W))
    for b in range(2):
        for o in range(cout):
            for y in range(H):
                for x in range(W):
                    for c in range(cin):
                        for ky in range(3):
                            for kx in range(3):
                                yy, xx = y + ky - 1, x + kx - 1
                                if 0 <= yy < H and 0 <= xx < W:
                                    want[b, o, y * W + x] += w[o, c, 3 * ky + kx] * a[b, c, yy * W + xx]
    assert np.array_equal(E.conv3x3(a, w, H, W), want)


@functools.lru_cache(maxsize=None)
def _report(shape, kind):
    net = E.dense_net(shape, kind)
    return net, E.validity(net, E.batch(net.args))


@pytest.mark.parametrize("shape,kind", E.DENSE_CASES)
def test_dense_net_is_valid_and_covers(shape, kind):
    net, r = _report(shape, kind)
    print(f"{net.name}: largest layer input {r['max_in']:.0f}, largest sum |w||a| {r['max_abs_sum']:.3g}, lo fractions {np.round(r['lo_frac'], 3)}, "
          f"ReLU survival {np.round(r['relu_frac'], 2)}, non-zero output channels {r['nonzero_channels']:.3f}")
    assert len(net.ints) == 1 + 2 * E.KINDS[kind] and net.wide == [(kind, l) in (("wide_stem", 0), ("wide_conv1", 1)) for l in range(len(net.ints))]
    assert r["ok"] and r["max_lolo"] == 0.0 and r["max_abs_sum"] < 2 ** 24
    for l, ((w, b), wide) in enumerate(zip(net.ints, net.wide)):
        assert E.fragment_coverage(w.astype(np.float64), wide) == 1.0, f"layer {l}: a fragment without a non-zero hi" + (" and lo" if wide else "")
        assert (E.split(w.astype(np.float64))[1] != 0).any() == wide
        assert set(np.unique(b)) <= {0, 1, 2}
    for l in E.lo_layers(kind):
        assert r["lo_frac"][l] >= 0.05, f"layer {l}: only {r['lo_frac'][l]:.3f} of the input activations have a lo"
    assert r["nonzero_channels"] >= 0.95
    assert all(0.4 <= f <= 0.6 for f in r["relu_frac"]), r["relu_frac"]


@pytest.mark.parametrize("shape,kind", E.DENSE_CASES)
def test_blob_folds_back_to_the_integers(shape, kind):
    """the blob (helpers.blob_manifest order, BatchNorm that folds to 1) gives back exactly the integer layers when folded as weights.cpp folds it"""
    net = E.dense_net(shape, kind)
    blob = net.blob()
    assert blob.dtype == np.float32 and np.all(np.isfinite(blob))
    for (w, b), (fw, fb) in zip(net.layers(), E.fold(net.args, blob)):
        assert np.array_equal(w, fw) and np.array_equal(b, fb)


@pytest.mark.parametrize("shape,kind,shift", E.CERTIFIED_CASES)
def test_certified_net_is_valid_for_every_input(shape, kind, shift):
    net = E.certified_net(shape, kind, shift)
    ok, bounds, worst = E.certificate(net)
    print(f"{net.name}: worst-case layer inputs {bounds}, worst sum {worst:.4g} grid units (2^{np.log2(worst):.2f})")
    assert ok and worst < 2 ** 24 and max(bounds) <= 2 ** 17
    for l, ((w, b), wide) in enumerate(zip(net.ints, net.wide)):
        assert int(np.count_nonzero(w.reshape(w.shape[0], -1), axis=1).max()) <= E.CERT_NNZ
        assert E.fragment_coverage(w.astype(np.float64), wide) >= 0.75
        if wide:
            assert bounds[l] <= 256, "a wide layer's inputs must all be bf16 (lo_w * lo_a is what the kernel leaves out)"
    # the bound is a bound: a batch with the all-ones and the all-zeros planes stays below it, and is valid by the batch check too
    x = E.batch(net.args)
    r = E.validity(net, x)
    assert r["ok"] and r["max_in"] <= max(bounds) and r["max_abs_sum"] <= worst
    for (w, b), (fw, fb) in zip(net.layers(), E.fold(net.args, net.blob())):
        assert np.array_equal(w, fw) and np.array_equal(b, fb)
    # what the heads read: within 2^5 of 1 on average (in the two-block nets the last block's unscaled skip, tens, is most of it: the shift cannot remove it)
    assert 2.0 ** -5 <= float(r["out"].mean()) <= 2.0 ** 5, "what the heads read is no longer O(1)"


def test_a_broken_net_is_noticed():
    """the checkers are not vacuous: a wide weight behind activations that need a lo, and a sum past 2^24, are both refused"""
    net = E.dense_net("go9x64", "wide_stem")
    w, b = net.ints[1]
    w2 = w.copy()
    w2[w2 != 0] = 257
    bad = E.ExactNet("bad", net.args, [net.ints[0], (w2, b), net.ints[2]], [True, True, False])
    r = E.validity(bad, E.batch(net.args))
    assert not r["ok"] and r["max_lolo"] > 0
    cert = E.certified_net("go9x64", "narrow2", 7)
    big = E.ExactNet("big", cert.args, [(w * 64, b) for w, b in cert.ints], cert.wide, 7)
    assert not E.certificate(big)[0]
