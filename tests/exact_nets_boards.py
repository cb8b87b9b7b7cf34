"""The exactly representable networks of tests/exact_nets.py for the 64-channel shapes of the larger boards that the one-tile bf16x3 tower serves
(net_bf16_wide_body.h, two pixel groups): Gomoku 15x15 and Hex 11x11 (4 planes), Havannah edge size 8 on its 15x15 array (20 planes).  Same layer
constructions (exact_nets._random_layer / _certified_layer), same conditions (exact_nets.validity / certificate / fragment_coverage); the density table and
the shifts are this file's own.  11x11 is the even split of the pixel tiles (4 + 4, no corner tile), 15x15 the uneven one (8 + 7, the last the corner tile).
Pure numpy; tests/test_exact_nets_boards.py asserts the conditions for every network here without a GPU."""
import functools

import exact_nets as E

SHAPES = {  # argument order of make_desc, without the block count
    "gomoku15x64": ("gomoku_15x15", 4, 15, 15, 64, 15, 15, 1, None, 225, 32, 1, "alphazero"),
    "hex11x64": ("hex_11x11", 4, 11, 11, 64, 11, 11, 1, None, 121, 32, 1, "alphazero"),
    "havannah15x64": ("havannah8x8", 20, 15, 15, 64, 15, 15, 1, None, 225, 32, 1, "alphazero"),
}
KINDS = E.KINDS


def args_of(shape, blocks):
    a = SHAPES[shape]
    return a[:8] + (blocks,) + a[9:]


# dense nets: (stem density, first conv density, other convs' density) per (input planes, variant).  A 4-plane stem has 36 weights per output channel, a
# 20-plane one 180: the stems' densities differ so that the stem's sums do, and what follows stays within the conditions on exact_nets.batch().
DENSE = {
    (4, "wide_stem"): (0.6, 0.08, 0.05), (4, "wide_conv1"): (0.6, 0.08, 0.05), (4, "narrow2"): (0.6, 0.1, 0.05),
    (20, "wide_stem"): (0.5, 0.08, 0.05), (20, "wide_conv1"): (0.5, 0.08, 0.05), (20, "narrow2"): (0.5, 0.1, 0.05),
}


@functools.lru_cache(maxsize=None)
def dense_net(shape, kind, seed=1):
    blocks = KINDS[kind]
    args = args_of(shape, blocks)
    C, cin = args[4], args[1]
    ds, d1, dr = DENSE[(cin, kind)]
    ints, wide = [], []
    for l in range(1 + 2 * blocks):
        vals = E._values(kind, l)
        ints.append(E._random_layer(1000 * seed + 10 * l, C, cin if l == 0 else C, ds if l == 0 else d1 if l == 1 else dr, vals))
        wide.append(vals is E.WIDE)
    return E.ExactNet(f"{shape}-{kind}", args, ints, wide)


@functools.lru_cache(maxsize=None)
def certified_net(shape, kind, shift, seed=1):
    blocks = KINDS[kind]
    args = args_of(shape, blocks)
    C, cin = args[4], args[1]
    ints, wide = [], []
    for l in range(1 + 2 * blocks):
        vals = E._values(kind, l)
        ints.append(E._certified_layer(5000 * seed + 10 * l, C, cin if l == 0 else C, vals))
        wide.append(vals is E.WIDE)
    return E.ExactNet(f"{shape}-{kind}-certified", args, ints, wide, shift)


# the networks the GPU tests run (tests/test_gpu_bf16_boards.py)
DENSE_CASES = [(shape, kind) for shape in SHAPES for kind in KINDS]
# (shape, variant, shift): the last layer times 2^-shift brings what the heads read to O(1), within what certificate() allows
SHIFTS = {"wide_conv1": 11, "narrow2": 7}
CERTIFIED_CASES = [(shape, kind, SHIFTS[kind]) for shape in SHAPES for kind in ("wide_conv1", "narrow2")]
