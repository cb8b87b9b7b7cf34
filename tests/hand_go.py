"""Hand-built Go sequences whose last move decides something: a chain across every 64-bit word of the 19x19 board captured whole, one stone capturing
four blocks, a snapback, a positional-superko cycle longer than a ko, and the position where the two ko rules differ.  Points are row * n + column, the
pass is n * n.  tests/test_go_model.py and tests/test_gpu_go_model.py let the model (tests/go_rules.py) confirm that each is what it claims before an
engine is compared.  This file imports neither the oracle nor the product."""


def _neighbours(p, n):
    x, y = p % n, p // n
    return [q for q, ok in ((p - n, y > 0), (p + n, y < n - 1), (p - 1, x > 0), (p + 1, x < n - 1)) if ok]


def _interleave(black, white, n):
    """Black's stones in order, White's in between; White passes when it has none left (Black never passes, so no two passes are consecutive)"""
    seq = []
    for i, b in enumerate(black):
        seq.append(b)
        if i + 1 < len(black):
            seq.append(white[i] if i < len(white) else n * n)
    return seq


# ---- a chain that winds across every word boundary of 19x19 -----------------------------------------------------------------------------------------
# White: column 9 from top to bottom, with arms along row 3 and row 10 to the left edge and along row 6 and row 13 to the right edge — 55 stones in
# all six 64-bit words of the 361 points, stepping over each of the boundaries 63|64, 127|128, 191|192, 255|256, 319|320.  Black: every neighbour of the
# chain.  Black's last stone takes the last liberty.
CHAIN_N = 19


def winding_chain():
    """(actions, the chain's points): White's stones in an order in which each joins the chain, Black's around them, Black's last move captures all"""
    n = CHAIN_N
    chain = [r * n + 9 for r in range(n)]
    for row, cols in ((3, range(8, -1, -1)), (6, range(10, n)), (10, range(8, -1, -1)), (13, range(10, n))):
        chain += [row * n + c for c in cols]
    inside = set(chain)
    around = sorted({q for p in chain for q in _neighbours(p, n)} - inside)
    assert len(around) > len(chain)
    return _interleave(around, chain, n), chain


# ---- one stone capturing four blocks ----------------------------------------------------------------------------------------------------------------
# 9x9, the centre of the cross is point 65 (row 7, column 2), just past the first 64-bit word: the four White stones lie in both words (56 | 64, 66, 74)
# and one of them on the edge row.
FOUR_N, FOUR_CENTRE = 9, 65


def four_blocks():
    n, c = FOUR_N, FOUR_CENTRE
    white = _neighbours(c, n)
    black = sorted({q for p in white for q in _neighbours(p, n)} - {c})
    return _interleave(black + [c], white, n), white


# ---- a snapback -------------------------------------------------------------------------------------------------------------------------------------
# 7x7, (column, row):   row 2   . B B B . . .        White's block W has two liberties, a = (2, 0) and b = (3, 0).  Black throws in at a (one liberty: b),
#                       row 1   B W W W B . .        White captures it at b, and the block, now with b, is left with the one liberty a: Black plays a again
#                       row 0   B W a b B . .        and captures five stones.  The position is new, so no ko rule objects.
SNAP_N, SNAP_A, SNAP_B = 7, 2, 3


def snapback():
    """(actions up to and including Black's throw-in, White's capture, Black's recapture)"""
    n = SNAP_N
    at = lambda x, y: y * n + x
    white = [at(1, 0), at(1, 1), at(2, 1), at(3, 1)]
    black = [at(0, 0), at(0, 1), at(1, 2), at(2, 2), at(3, 2), at(4, 1), at(4, 0)]
    return _interleave(black + [SNAP_A], white, n), SNAP_B, SNAP_A


# ---- a superko cycle longer than a ko ---------------------------------------------------------------------------------------------------------------
# 3x3 without a pass, thirteen stones, every one from the 7th on a capture; now White at 1 would capture and leave the board as it was
# eight plies ago, with the same side to move: refused by both rules.  (Found by a random search over the model's games, not by hand; the model
# confirms it where it is used.)
CYCLE_N, CYCLE, CYCLE_POINT, CYCLE_AGE = 3, [6, 7, 0, 1, 4, 5, 8, 3, 2, 7, 0, 5, 6], 1, 8

# ---- where the two ko rules differ ------------------------------------------------------------------------------------------------------------------
# 3x3: Black 1, White 3, Black 5, White 4, Black 0, White 2 captures the two stones at 0 and 1.  Black at 1 would capture the stone at 2 and recreate
# the stones after White's second move, three plies ago — then with Black to move, now with White to move.  Positional superko refuses it, situational
# superko allows it.
DIFFER_N, KO_RULES_DIFFER, DIFFER_POINT, DIFFER_AGE = 3, [1, 3, 5, 4, 0, 2], 1, 3
