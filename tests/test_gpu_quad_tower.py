"""The tower of a simulation on four workgroups of one XCD (sim_help.h towerBodyQuad) against the pair tower, the solo tower and the oracle, through
mz_tail_towers_device: 8 towers, i.e. 32 workgroups in quad mode, four per XCD.

Every member computes its oc-tiles with the layer function of the solo tower, so the activations must be the same BITS whoever computed them; the exchange
carries its phase in the sign bit of the ReLU outputs, so exact zeros and the all-zero / all-one boards are among the inputs.

The oracle has no entry point that returns a tower's activations as they are.  What tests/test_gpu_net.py compares is the hidden state of a MuZero network's
initial inference: the representation tower's output, min-max scaled (o_nn.cpp scaleHidden: (h - min) / (max - min), f32).  The same is done here with the
BASELINE configs[3] network (the same 18 -> 6 blocks x 64 tower shape): the solo tower's output, scaled the same way in f32, must be the oracle's hidden state
bit for bit.  The AlphaZero weights the issue names (generate_weights(desc_c2, 0), one `sharpen`ed set — which changes the heads only — and a second seed) are
compared between the three modes."""
import numpy as np
import pytest

from helpers import binary_planes, same_bits, frac_bit_equal, sharpen

pytestmark = pytest.mark.gpu

T, CH, P, W32 = 8, 18, 81, 3


def _planes():
    x = np.zeros((T, CH, P), np.float32)
    x[1] = 1.0                                             # a full board in every plane
    x[2:] = binary_planes(1201, (T - 2, CH, P))            # six random positions
    x[3, :, :] *= (np.arange(P) % 9 != 8)[None, :]         # ... one with the last column (the corner tile's pixel among it) empty
    return x


def _pack(x):
    b = np.zeros((T, CH, W32), np.uint32)
    for p in range(P):
        b[:, :, p >> 5] |= (x[:, :, p] != 0).astype(np.uint32) << np.uint32(p & 31)
    return b.reshape(T, CH * W32)


def _modes(mz, net, bits):
    res = {}
    for members in (1, 2, 4):
        out, xcc, err, status = mz.tail_towers(net, bits, members)
        if status != 0:
            pytest.skip(f"members on different XCDs ({members} per tower): XCC_ID + 1 by member and tower:\n{xcc}")
        assert err == 0, f"{members} members per tower: error flag {err} (a wait of the exchange timed out)"
        assert xcc.min() >= 1 and all(np.array_equal(xcc[m], xcc[0]) for m in range(members))
        res[members] = out
    return res


def _scale_hidden(h):
    h = h.reshape(h.shape[0], -1).astype(np.float32)
    mn, mx = h.min(axis=1, keepdims=True), h.max(axis=1, keepdims=True)
    scale = (mx - mn).astype(np.float32)
    scale = np.where(scale < np.float32(1e-5), scale + np.float32(1e-5), scale).astype(np.float32)
    return ((h - mn) / scale).astype(np.float32)


@pytest.mark.parametrize("weights", ["seed0", "sharpened", "seed1"])
def test_quad_equals_pair_equals_solo(mz, weights):
    d = mz.DESCS["c2"]()
    w = mz.generate_weights(d, 1 if weights == "seed1" else 0)
    if weights == "sharpened":
        w = sharpen(d, w, 40.0, 25.0)
    net = mz.Net(d, w)
    r = _modes(mz, net, _pack(_planes()))
    solo, pair, quad = r[1], r[2], r[4]
    assert np.isfinite(solo).all() and (solo >= 0).all() and (solo == 0).any() and (solo > 0).any()
    assert len({solo[t].tobytes() for t in range(T)}) == T, "the towers' inputs must give different outputs"
    for t in range(T):
        assert same_bits(pair[t], solo[t]), f"tower {t}: pair differs from solo ({frac_bit_equal(pair[t], solo[t]):.4f} of the words equal)"
        assert same_bits(quad[t], solo[t]), f"tower {t}: quad differs from solo ({frac_bit_equal(quad[t], solo[t]):.4f} of the words equal)"


def test_solo_pair_quad_equal_the_oracle(mz, oracle):
    args = ("go_9x9", 18, 9, 9, 64, 9, 9, 1, 6, 82)
    kw = dict(vh=256, dv=1, type_name="muzero")
    d, od = mz.make_desc(*args, **kw), oracle.make_desc(*args, **kw)
    w = mz.generate_weights(d, 0)
    net, onet = mz.Net(d, w), oracle.OracleNet(od, w)
    x = _planes()
    oh = onet.initial(x.reshape(T, -1))[3]
    r = _modes(mz, net, _pack(x))
    for members, name in ((1, "solo"), (2, "pair"), (4, "quad")):
        h = _scale_hidden(r[members])
        assert same_bits(h, oh), f"{name}: scaled tower output differs from the oracle's hidden state ({frac_bit_equal(h, oh):.4f} of the words equal)"
