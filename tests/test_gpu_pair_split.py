"""The split chain of the pair tower (sim_help.h towerBodyPair): the accumulator of pixel tile 2 is brought up to tap 6 by one wave, handed to a wave of
another SIMD through LDS, and finished there (taps 6 .. 8 and the epilogue).  Through mz_tail_towers_device as in test_gpu_quad_tower.py: 8 towers, i.e. 16
workgroups in pair mode, two per XCD.

Every output is still the solo tower's tap-major, k-ordered chain, so members = 2 must give the solo tower's BITS.  What a broken hand-over would do — lose the
first wave's part, add it twice, start the second part at +0 — cancels in no output of the handed tile when only ONE tap of every trunk conv is alive: with
tap t < 6 alive the whole sum lies in front of the cut, with t >= 6 behind it.  So beside generate_weights(desc_c2, 0) there are nine networks made from it
with all taps but tap t zeroed in every trunk conv (the cut is between two taps, kPairCut = 6: no network cut inside a tap is needed).

Boards: those of test_gpu_quad_tower._planes, one with stones only on the 16 pixels of the handed tile and one with stones everywhere else; the pixels are read
from the library's tile map (mz_tail_tower_tile), not computed here."""
import numpy as np
import pytest

from helpers import blob_manifest, same_bits, frac_bit_equal
from test_gpu_quad_tower import T, CH, P, _pack, _planes

pytestmark = pytest.mark.gpu

HANDED_TILE = 2
NETWORKS = ["all_taps"] + [f"tap{t}" for t in range(9)]


def _one_tap(desc, w, t):
    """The blob with taps != t of every 3x3 conv of the trunk (stem and residual convs, weights [cout][cin][3][3]) set to zero."""
    w = np.array(w, np.float32)
    convs = [(name, off, n) for name, off, n in blob_manifest(desc) if name.startswith("repr.") and name.endswith(".w")]
    assert len(convs) == 1 + 2 * desc.num_blocks
    for _, off, n in convs:
        k = w[off:off + n].reshape(-1, 9)
        keep = k[:, t].copy()
        k[:] = 0.0
        k[:, t] = keep
    return w


@pytest.fixture(scope="module")
def handed_pixels(mz):
    q = mz.tail_tower_tile(HANDED_TILE)
    assert q.shape == (16,) and (q >= 0).all() and (q < P).all() and len(set(q.tolist())) == 16, f"tile {HANDED_TILE} of the tile map: {q}"
    return q


@pytest.fixture(scope="module")
def boards(handed_pixels):
    """Two batches of T boards: _planes(), and the two boards about the handed tile followed by _planes()[2:] again (a multiple of 8 towers keeps pairs on one XCD)."""
    a = _planes()
    b = a.copy()
    on_tile = np.zeros(P, np.float32)
    on_tile[handed_pixels] = 1.0
    b[0] = on_tile[None, :]
    b[1] = (1.0 - on_tile)[None, :]
    return a, b


def _solo_and_pair(mz, net, x):
    res = {}
    for members in (1, 2):
        out, xcc, err, status = mz.tail_towers(net, _pack(x), members)
        if status != 0:
            pytest.skip(f"members on different XCDs ({members} per tower): XCC_ID + 1 by member and tower:\n{xcc}")
        assert err == 0, f"{members} members per tower: error flag {err} (95: an exchange, 101: the hand-over of the split chain timed out)"
        assert xcc.min() >= 1 and all(np.array_equal(xcc[m], xcc[0]) for m in range(members))
        res[members] = out
    return res[1], res[2]


@pytest.mark.parametrize("network", NETWORKS)
def test_pair_split_equals_solo(mz, network, boards, handed_pixels):
    d = mz.DESCS["c2"]()
    w = mz.generate_weights(d, 0)
    if network != "all_taps":
        w = _one_tap(d, w, int(network[3:]))
    net = mz.Net(d, w)
    distinct = {}
    for name, x in zip(("planes", "tile"), boards):
        assert x.shape == (T, CH, P)
        solo, pair = _solo_and_pair(mz, net, x)
        assert np.isfinite(solo).all() and (solo >= 0).all()
        for t in range(T):
            assert same_bits(pair[t], solo[t]), f"{network}, {name} board {t}: pair differs from solo ({frac_bit_equal(pair[t], solo[t]):.4f} of the words equal)"
            distinct[x[t].tobytes()] = solo[t].tobytes()
        # a condition on the inputs, checked on the solo result: the handed tile has outputs that are not zero, so a lost or doubled accumulator would show
        handed = solo[:, :, handed_pixels]
        print(f"{network}, {name}: {int((handed != 0).sum())} of {handed.size} outputs of the handed tile are non-zero")
        assert (handed != 0).any(), f"{network}, {name}: every output of the handed tile is zero"
    assert len(distinct) == T + 2, "ten different boards"
    assert len(set(distinct.values())) == len(distinct), f"{network}: different boards must give different outputs"
