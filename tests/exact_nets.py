"""Exactly representable networks for the bf16x3 towers (net_bf16_body.h, net_bf16_wide_body.h) and a float64 reference of the residual tower.
Pure numpy; no reference code.

The bf16x3 towers carry a value v as hi = bf16(v), lo = bf16(v - hi) and form a product from hi_w * lo_a, lo_w * hi_a and hi_w * hi_a in one f32 accumulator.
When every weight and every activation IS hi + lo, no term has lo_w and lo_a both non-zero, and every partial sum of a layer is a multiple of one power of
two (its grid) and below 2^24 of it, then nothing rounds in any summation order: the f32 HIP path, the CPU oracle, the bf16x3 path and a float64 sum agree
bit for bit, and a lost or misplaced partial product is a whole-number error.  The networks here are built to meet these conditions, and `validity()` /
`certificate()` check them in float64: BatchNorm folds to exactly 1 (bn_g = 1, bn_b = bn_m = 0, bn_v = float32(1 - 1e-5): v + 1e-5f rounds to 1.0f), conv
weights and biases are small integers.

  * narrow weights: +-1, +-2 (lo = 0); wide weights: +-(256 m + e), m in {1, 2}, e in {+-1, +-3}, those whose lo is non-zero
  * dense nets: random sparse weights, valid for one input batch (the one the caller checks them on)
  * certified nets: at most 8 non-zeros per output channel, valid for every 0 / 1 input by a worst-case bound (for the worker, whose leaves nobody chooses)
Variants: "wide_stem" (1 block; lo_w in the stem, then hi_w * lo_a in both tower layers), "wide_conv1" (1 block; lo_w * hi_a in a tower layer, then
hi_w * lo_a with the skip), "narrow2" (2 blocks, narrow throughout: the hand-over of x between blocks, lo_a != 0 from conv3 on)."""
import functools
import types

import numpy as np

from helpers import binary_planes, blob_manifest, counter_u01

SHAPES = {  # argument order of make_desc, without the block count
    "go9x64": ("go_9x9", 18, 9, 9, 64, 9, 9, 1, None, 82, 64, 1, "alphazero"),
    "oth8x64": ("othello_8x8", 4, 8, 8, 64, 8, 8, 1, None, 65, 64, 1, "alphazero"),
    "go9x128": ("go_9x9", 18, 9, 9, 128, 9, 9, 1, None, 82, 64, 1, "alphazero"),
    "go9x256": ("go_9x9", 18, 9, 9, 256, 9, 9, 1, None, 82, 64, 1, "alphazero"),
}
KINDS = {"wide_stem": 1, "wide_conv1": 1, "narrow2": 2}  # variant -> blocks
BN_V_ONE = np.float32(1.0 - 1e-5)                        # g / sqrtf(v + 1e-5f) == g exactly
NARROW = np.array([1, 2], np.int64)


def bf16_rne(v):
    """f32 -> bf16 (round to nearest, ties to even) -> f32: bf16_split.h bf16Rne on finite values"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def split(v):
    """(hi, lo, exact): bf16_split.h bf16Split in f32, and whether v == hi + lo (v itself an f32) for every element"""
    v64 = np.asarray(v, np.float64)
    v32 = v64.astype(np.float32)
    hi = bf16_rne(v32)
    lo = bf16_rne(v32 - hi)
    exact = bool(np.all(v32.astype(np.float64) == v64) and np.all(hi.astype(np.float64) + lo.astype(np.float64) == v64))
    return hi.astype(np.float64), lo.astype(np.float64), exact


def _wide_values():
    c = np.array([256 * m + e for m in (1, 2) for e in (-3, -1, 1, 3)], np.int64)
    _, lo, exact = split(c)
    assert exact
    return c[lo != 0]


WIDE = _wide_values()


def args_of(shape, blocks):
    a = SHAPES[shape]
    return a[:8] + (blocks,) + a[9:]


def manifest_desc(args):
    """what helpers.blob_manifest reads of a descriptor"""
    return types.SimpleNamespace(num_input_channels=args[1], input_channel_height=args[2], input_channel_width=args[3], num_hidden_channels=args[4],
                                 hidden_channel_height=args[5], hidden_channel_width=args[6], num_action_feature_channels=args[7], num_blocks=args[8],
                                 action_size=args[9], num_value_hidden_channels=args[10], discrete_value_size=args[11], type=0)


def tower_names(blocks):
    return ["repr.stem"] + [f"repr.conv{b}" for b in range(2 * blocks)]


# ---------------------------------------------------------------------------------------------
# float64 reference: conv3x3 with zero padding + bias (+ skip), ReLU; block structure of network_unit (t = relu(conv1(x)); x = relu(conv2(t) + x))
# ---------------------------------------------------------------------------------------------
def conv3x3(a, w, H, W):
    """a [B][cin][H * W], w [cout][cin][9] (tap = 3 * ky + kx reads (y + ky - 1, x + kx - 1)) -> [B][cout][H * W], float64"""
    B, cin = a.shape[0], a.shape[1]
    pad = np.zeros((B, cin, H + 2, W + 2), np.float64)
    pad[:, :, 1:H + 1, 1:W + 1] = a.reshape(B, cin, H, W)
    out = np.zeros((B, w.shape[0], H * W), np.float64)
    for t in range(9):
        out += np.matmul(w[:, :, t], pad[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W].reshape(B, cin, H * W))
    return out


def tower_reference(layers, x, H, W):
    """layers: [(w [cout][cin][9], b [cout])] folded, float64; x [B][cin * H * W] -> (inputs of every layer, skip of every layer or None, last activations)"""
    a = np.asarray(x, np.float64).reshape(x.shape[0], -1, H * W)
    ins, skips = [a], [None]
    cur = np.maximum(conv3x3(a, layers[0][0], H, W) + layers[0][1][None, :, None], 0.0)
    for l in range(1, len(layers), 2):
        ins.append(cur)
        skips.append(None)
        t = np.maximum(conv3x3(cur, layers[l][0], H, W) + layers[l][1][None, :, None], 0.0)
        ins.append(t)
        skips.append(cur)
        cur = np.maximum(conv3x3(t, layers[l + 1][0], H, W) + layers[l + 1][1][None, :, None] + cur, 0.0)
    return ins, skips, cur


def fold(args, blob):
    """the tower's folded layers of any blob, in f32 as weights.cpp takeConvBN folds them (s = g / sqrtf(v + 1e-5f); w * s; (b - m) * s + beta), as float64"""
    blob = np.asarray(blob, np.float32)
    s = {name: blob[off:off + n] for name, off, n in blob_manifest(manifest_desc(args))}
    out = []
    for name in tower_names(args[8]):
        cout = s[name + ".b"].size
        sc = s[name + ".bn_g"] / np.sqrt(s[name + ".bn_v"] + np.float32(1e-5), dtype=np.float32)
        w = s[name + ".w"].reshape(cout, -1) * sc[:, None]
        b = (s[name + ".b"] - s[name + ".bn_m"]) * sc + s[name + ".bn_b"]
        assert w.dtype == np.float32 and b.dtype == np.float32
        out.append((w.reshape(cout, -1, 9).astype(np.float64), b.astype(np.float64)))
    return out


# ---------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------
class ExactNet:
    """args: make_desc arguments; ints: [(w int64 [cout][cin][9], b int64 [cout])]; wide: per layer, does it hold wide weights; shift: the last layer is
    scaled by 2^-shift through its bn_g"""

    def __init__(self, name, args, ints, wide, shift=0):
        self.name, self.args, self.ints, self.wide, self.shift = name, args, ints, wide, shift
        self.H, self.W = args[5], args[6]

    def scale(self, l):
        return 2.0 ** -self.shift if l + 1 == len(self.ints) else 1.0

    def layers(self):
        """folded layers as float64 (what fold() gives for blob())"""
        return [(w.astype(np.float64) * self.scale(l), b.astype(np.float64) * self.scale(l)) for l, (w, b) in enumerate(self.ints)]

    def blob(self, heads_from=None):
        """the weight blob; the heads (everything behind the tower) from `heads_from` (a blob of the same shape), else small deterministic values"""
        man = blob_manifest(manifest_desc(self.args))
        total = man[-1][1] + man[-1][2]
        blob = np.zeros(total, np.float32)
        at = {name: slice(off, off + n) for name, off, n in man}
        tower = tower_names(self.args[8])
        first_head = at["policy_conv.w"].start
        if heads_from is not None:
            assert heads_from.size == total
            blob[first_head:] = np.asarray(heads_from, np.float32)[first_head:]
        else:
            bn = {"bn_g": 1.0, "bn_v": BN_V_ONE, "bn_b": 0.0, "bn_m": 0.0}
            for name, off, n in man:
                if off >= first_head:
                    kind = name.rsplit(".", 1)[1]
                    blob[off:off + n] = bn[kind] if kind in bn else (counter_u01(7 + off, n) - np.float32(0.5)) * np.float32(0.25)
        for l, (name, (w, b)) in enumerate(zip(tower, self.ints)):
            blob[at[name + ".w"]] = w.reshape(-1)
            blob[at[name + ".b"]] = b
            blob[at[name + ".bn_g"]] = self.scale(l)
            blob[at[name + ".bn_v"]] = BN_V_ONE
        return blob

    def reference(self, x):
        """last activations [B][C][H * W] as f32 (exact: the validity conditions make every value an f32)"""
        out = tower_reference(self.layers(), x, self.H, self.W)[2]
        o32 = out.astype(np.float32)
        assert np.array_equal(o32.astype(np.float64), out)
        return o32


def _uniform(seed, n):
    return counter_u01(seed, n).astype(np.float64)


def _random_layer(seed, cout, cin, density, values):
    """random sparse weights, random signs, biases in {0, 1, 2}; every (tap, 32-channel k-block, 16-channel oc-tile) fragment gets at least one non-zero"""
    n = cout * cin * 9
    u, uv, us = _uniform(seed, n), _uniform(seed + 1, n), _uniform(seed + 2, n)
    val = values[np.minimum((uv * len(values)).astype(np.int64), len(values) - 1)] * np.where(us < 0.5, -1, 1)
    w = np.where(u < density, val, 0).reshape(cout, cin, 9)
    val = val.reshape(cout, cin, 9)
    pick = _uniform(seed + 3, 9 * ((cin + 31) // 32) * (cout // 16))
    i = 0
    for t in range(9):
        for kb in range((cin + 31) // 32):
            for ot in range(cout // 16):
                c0, c1 = 32 * kb, min(cin, 32 * kb + 32)
                if not w[16 * ot:16 * ot + 16, c0:c1, t].any():
                    k = int(pick[i] * 16 * (c1 - c0))
                    oc, c = 16 * ot + k % 16, c0 + k // 16
                    w[oc, c, t] = val[oc, c, t]
                i += 1
    b = np.minimum((_uniform(seed + 4, cout) * 3).astype(np.int64), 2)
    return w.astype(np.int64), b


# dense nets: (stem density, first conv density, other convs' density) per (channels, variant); all meet validity() and coverage() on batch() — asserted by
# tests/test_exact_nets.py, which is where a change of these numbers shows
DENSE = {
    (64, "wide_stem"): (0.4, 0.08, 0.05), (64, "wide_conv1"): (0.4, 0.08, 0.05), (64, "narrow2"): (0.5, 0.1, 0.05),
    (128, "wide_stem"): (0.4, 0.05, 0.03), (128, "wide_conv1"): (0.4, 0.05, 0.03), (128, "narrow2"): (0.5, 0.06, 0.03),
    (256, "wide_stem"): (0.4, 0.03, 0.02), (256, "wide_conv1"): (0.4, 0.03, 0.02), (256, "narrow2"): (0.5, 0.04, 0.02),
}


def _values(kind, l):
    return WIDE if (kind == "wide_stem" and l == 0) or (kind == "wide_conv1" and l == 1) else NARROW


@functools.lru_cache(maxsize=None)
def dense_net(shape, kind, seed=1):
    blocks = KINDS[kind]
    args = args_of(shape, blocks)
    C, cin = args[4], args[1]
    ds, d1, dr = DENSE[(C, kind)]
    ints, wide = [], []
    for l in range(1 + 2 * blocks):
        vals = _values(kind, l)
        ints.append(_random_layer(1000 * seed + 10 * l, C, cin if l == 0 else C, ds if l == 0 else d1 if l == 1 else dr, vals))
        wide.append(vals is WIDE)
    return ExactNet(f"{shape}-{kind}", args, ints, wide)


def batch(args):
    """three samples: random 0 / 1 planes (30 %), all zeros, all ones (tests/test_gpu_bf16_wide.py _batch)"""
    x = binary_planes(321, (3, args[1] * args[2] * args[3]))
    x[1] = 0.0
    x[2] = 1.0
    return x


CERT_NNZ = 8


def _certified_layer(seed, cout, cin, values):
    """at most CERT_NNZ non-zeros per output channel; the 128 non-zeros of an oc-tile go round its (tap, k-block) fragments in turn"""
    KB = (cin + 31) // 32
    w = np.zeros((cout, cin, 9), np.int64)
    n = cout * CERT_NNZ
    uc, uv, us, uo = _uniform(seed, n), _uniform(seed + 1, n), _uniform(seed + 2, n), _uniform(seed + 3, cout // 16)
    i = 0
    for ot in range(cout // 16):
        start = int(uo[ot] * 9 * KB)
        for k in range(16 * CERT_NNZ):
            f = (start + k) % (9 * KB)
            t, kb = f // KB, f % KB
            c0, c1 = 32 * kb, min(cin, 32 * kb + 32)
            c = c0 + min(int(uc[i] * (c1 - c0)), c1 - c0 - 1)
            w[16 * ot + k % 16, c, t] = values[min(int(uv[i] * len(values)), len(values) - 1)] * (-1 if us[i] < 0.5 else 1)
            i += 1
    assert int(np.count_nonzero(w.reshape(cout, -1), axis=1).max()) <= CERT_NNZ
    b = np.minimum((_uniform(seed + 4, cout) * 3).astype(np.int64), 2)
    return w, b


@functools.lru_cache(maxsize=None)
def certified_net(shape, kind, shift, seed=1):
    blocks = KINDS[kind]
    args = args_of(shape, blocks)
    C, cin = args[4], args[1]
    ints, wide = [], []
    for l in range(1 + 2 * blocks):
        vals = _values(kind, l)
        ints.append(_certified_layer(5000 * seed + 10 * l, C, cin if l == 0 else C, vals))
        wide.append(vals is WIDE)
    return ExactNet(f"{shape}-{kind}-certified", args, ints, wide, shift)


# the networks the GPU tests run (tests/test_gpu_bf16_exact.py); tests/test_exact_nets.py asserts the conditions for every one of them without a GPU
DENSE_CASES = [(shape, kind) for shape in SHAPES for kind in KINDS]
# (shape, variant, shift): the last layer times 2^-shift brings what the heads read to O(1) (mean about 1, largest values in the tens); the shifts are within
# what certificate() allows (the unscaled skip must stay on the scaled layer's grid below 2^24 of it)
CERTIFIED_CASES = [(shape, kind, 11 if kind == "wide_conv1" else 7) for shape in ("go9x64", "go9x128", "go9x256") for kind in ("wide_conv1", "narrow2")]


# ---------------------------------------------------------------------------------------------
# the conditions
# ---------------------------------------------------------------------------------------------
LIMIT = 2.0 ** 24


def validity(net, x):
    """The validity conditions of `net` on the batch x, in float64.  Returns a report; `ok` says that all hold:
    every layer's weights and input activations are hi + lo exactly, sum |lo_w| |lo_a| = 0, and sum |w| |a| + |b| + |skip| < 2^24 grid at every output,
    where grid is the power of two that every term of the layer is a multiple of (1 for the integer layers, 2^-shift for a scaled last layer)."""
    layers = net.layers()
    ins, skips, out = tower_reference(layers, x, net.H, net.W)
    rep = {"ok": True, "max_in": 0.0, "max_abs_sum": 0.0, "max_lolo": 0.0, "lo_frac": [], "relu_frac": [], "out": out}
    for l, ((w, b), a, sk) in enumerate(zip(layers, ins, skips)):
        grid = net.scale(l)
        whi, wlo, wex = split(w)
        ahi, alo, aex = split(a)
        lolo = float(conv3x3(np.abs(alo), np.abs(wlo), net.H, net.W).max())
        tot = conv3x3(np.abs(a), np.abs(w), net.H, net.W) + np.abs(b)[None, :, None] + (0.0 if sk is None else np.abs(sk))
        on_grid = bool(np.all(np.mod(w / grid, 1.0) == 0) and np.all(np.mod(b / grid, 1.0) == 0) and np.all(np.mod(a, 1.0) == 0))
        rep["ok"] = rep["ok"] and wex and aex and lolo == 0.0 and on_grid and float(tot.max()) < LIMIT * grid
        rep["max_in"] = max(rep["max_in"], float(np.abs(a).max()))
        rep["max_abs_sum"] = max(rep["max_abs_sum"], float(tot.max()) / grid)
        rep["max_lolo"] = max(rep["max_lolo"], lolo)
        rep["lo_frac"].append(float(np.mean(alo != 0)))
        pre = conv3x3(a, w, net.H, net.W) + b[None, :, None] + (0.0 if sk is None else sk)
        rep["relu_frac"].append(float(np.mean(pre > 0)))
    rep["nonzero_channels"] = float(np.mean(out.max(axis=(0, 2)) > 0))
    return rep


def fragment_coverage(w, wide):
    """fraction of the (tap, 32-channel k-block, 16-channel oc-tile) fragments of a layer that hold a non-zero hi, and — for a wide layer — a non-zero lo too"""
    cout, cin = w.shape[0], w.shape[1]
    hi, lo, _ = split(w)
    got = total = 0
    for kb in range((cin + 31) // 32):
        for ot in range(cout // 16):
            fh = hi[16 * ot:16 * ot + 16, 32 * kb:32 * kb + 32, :].reshape(-1, 9)
            fl = lo[16 * ot:16 * ot + 16, 32 * kb:32 * kb + 32, :].reshape(-1, 9)
            ok = fh.any(axis=0) & (fl.any(axis=0) if wide else True)
            got += int(np.count_nonzero(ok))
            total += 9
    return got / total


def lo_layers(kind):
    """the layers meant to exercise hi_w * lo_a (their input activations need a lo)"""
    return {"wide_stem": (1, 2), "wide_conv1": (2,), "narrow2": (3, 4)}[kind]


def certificate(net):
    """Validity of a certified net for EVERY 0 / 1 input, from the worst-case bound bound_l = max_oc (sum |w| bound_{l-1} + |b|) + bound_skip.  Returns
    (ok, bounds of every layer's input, largest sum |w| |a| + |b| + |skip| in units of the layer's grid).  Uses: every integer of magnitude <= 2^17 is hi + lo
    exactly and every one <= 256 is a bf16 (both asserted by tests/test_exact_nets.py)."""
    ok, bound_in, bounds, worst = True, 1.0, [], 0.0
    x_bound = None  # the block input kept for the skip
    for l, (w, b) in enumerate(net.ints):
        grid = net.scale(l)
        _, wlo, wex = split(w.astype(np.float64))
        s = np.abs(w).reshape(w.shape[0], -1).sum(axis=1).astype(np.float64)
        skip = x_bound if (l >= 2 and l % 2 == 0) else 0.0
        tot = float((s * bound_in + np.abs(b)).max()) * grid + skip
        ok = ok and wex and bound_in <= 2.0 ** 17 and (not wlo.any() or bound_in <= 256.0) and tot < LIMIT * grid
        bounds.append(bound_in)
        worst = max(worst, tot / grid)
        if l % 2 == 0:
            x_bound = tot
        bound_in = tot
    return ok, bounds, worst


# ---------------------------------------------------------------------------------------------
# a forward error bound of the bf16x3 tower on ANY network, from the float64 reference alone
# ---------------------------------------------------------------------------------------------
def bf16x3_error_bound(layers, x, H, W):
    """E_l = |W_l| (*) E_{l-1} (+ E_skip) + (2^-15 + K_l 2^-24) (|W_l| (*) |a_{l-1}|), E of the 0 / 1 planes = 0; K_l = 9 cin terms per output.
    2^-15: two split residuals of 2^-17 relative (bf16_split.h: 2^-16 per operand, halved by the rounding to nearest) and the dropped lo * lo, 2^-18 ... all
    below 2^-15 together; K_l 2^-24: the f32 accumulation.  (ReLU does not increase an error.)  Returns (reference output, bound), float64."""
    ins, skips, out = tower_reference(layers, x, H, W)
    E = [np.zeros_like(ins[0])]
    e_x = None
    for l, ((w, b), a) in enumerate(zip(layers, ins)):
        K = 9 * w.shape[1]
        e = conv3x3(E[l], np.abs(w), H, W) + (2.0 ** -15 + K * 2.0 ** -24) * conv3x3(np.abs(a), np.abs(w), H, W)
        if skips[l] is not None:
            e = e + e_x
        if l % 2 == 0:
            e_x = e
        E.append(e)
    return out, E[-1]
