"""Havannah as the reference plays it (environment/havannah), restated in plain Python from the rule list — not from the C++ engines it is the yardstick of.

Edge size N plays on an E x E array, E = 2N - 1; cell (i, j) has id i * E + j and is on the board iff N - 1 <= i + j <= 3N - 3.  A cell's neighbours are
(i-1, j) (i-1, j+1) (i, j-1) (i, j+1) (i+1, j-1) (i+1, j).  E * E actions, no pass, Black first, strictly alternating.  Swap rule: every on-board cell is legal
on the second action, and taking the occupied one makes it White's where it is — while Black's bit stays in the feature bitboards, so the cell shows in both
history planes from then on (the reference's quirk, kept).  Only the mover's group through the new stone is tested for a win: bridge (>= 2 of the 6 corners),
fork (>= 3 of the 6 sides; corners belong to no side) or ring.  A winner never goes away.

Cells are a dict, the group is found by graph search, and the ring's hole test exists twice: `hole_bbox` (the reference's flood over the group's bounding
box plus a one-cell frame) and `hole_rim` (some cell of the array outside the group that the array's rim cannot reach); the tests hold them to each other."""
import numpy as np

NEIGHBOURS = ((-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0))


class Havannah:
    def __init__(self, N=8, swap=True):
        self.N, self.E, self.swap = N, 2 * N - 1, swap
        E = self.E
        self.P = E * E
        self.valid = {(i, j) for i in range(E) for j in range(E) if N - 1 <= i + j <= 3 * N - 3}
        self.corners = {(0, N - 1), (0, E - 1), (N - 1, 0), (N - 1, E - 1), (E - 1, 0), (E - 1, N - 1)}
        # a side: the N - 2 cells strictly between two corners
        lines = (lambda i, j: i == 0, lambda i, j: i + j == N - 1, lambda i, j: j == 0, lambda i, j: i == E - 1, lambda i, j: i + j == 3 * N - 3, lambda i, j: j == E - 1)
        self.sides = [{c for c in self.valid if on(*c) and c not in self.corners} for on in lines]
        assert all(len(s) == N - 2 for s in self.sides) and len(self.valid) == 3 * N * (N - 1) + 1
        self.reset()

    def reset(self):
        self.owner = {c: 0 for c in self.valid}           # 0 empty, 1 black, 2 white
        self.fb = (set(), set())                          # the two feature bitboards: black never loses the bit of a swapped stone
        self.history = [(frozenset(), frozenset())]      # the positions so far, the empty one first
        self.actions, self.turn, self.winner = [], 1, 0
        self.last = {}                                    # what the last action's win test saw (kind, group, gates): for the tests

    def cell(self, a): return divmod(a, self.E)
    def ident(self, c): return c[0] * self.E + c[1]
    def neighbours(self, c): return [(c[0] + di, c[1] + dj) for di, dj in NEIGHBOURS if (c[0] + di, c[1] + dj) in self.valid]
    def swappable(self): return self.swap and len(self.actions) == 1

    def is_legal(self, a):
        if not 0 <= a < self.P or self.cell(a) not in self.valid:
            return False
        return self.swappable() or self.owner[self.cell(a)] == 0

    def legal_mask(self):
        return np.array([self.is_legal(a) for a in range(self.P)], np.uint8)

    def group(self, c):
        colour, seen, todo = self.owner[c], {c}, [c]
        while todo:
            for q in self.neighbours(todo.pop()):
                if self.owner[q] == colour and q not in seen:
                    seen.add(q)
                    todo.append(q)
        return seen

    def own_neighbours(self, c, colour):
        return sum(self.owner[q] == colour for q in self.neighbours(c))

    # ---- the ring's hole test, twice
    def hole_bbox(self, grp):
        """The reference's detectHole: the group's bounding box plus a frame of one cell; everything that is not the group is background, the frame's mark
        spreads through the background by the six-neighbour adjacency; a background cell it does not reach is a hole."""
        imin, imax = min(i for i, _ in grp), max(i for i, _ in grp)
        jmin, jmax = min(j for _, j in grp), max(j for _, j in grp)
        di, dj = imax - imin + 3, jmax - jmin + 3
        obj = {(i - imin + 1, j - jmin + 1) for i, j in grp}
        frame = {(i, j) for i in range(di) for j in range(dj) if i in (0, di - 1) or j in (0, dj - 1)}
        reached, todo = set(frame), list(frame)
        while todo:
            i, j = todo.pop()
            for a, b in NEIGHBOURS:
                q = (i + a, j + b)
                if 0 <= q[0] < di and 0 <= q[1] < dj and q not in obj and q not in reached:
                    reached.add(q)
                    todo.append(q)
        return any((i, j) not in obj and (i, j) not in reached for i in range(di) for j in range(dj))

    def hole_rim(self, grp):
        """Some cell of the E x E array outside the group — a stone, empty or off the board — that is not connected to the array's rim through such cells."""
        E = self.E
        rim = [(i, j) for i in range(E) for j in range(E) if (i in (0, E - 1) or j in (0, E - 1)) and (i, j) not in grp]
        reached, todo = set(rim), list(rim)
        while todo:
            i, j = todo.pop()
            for a, b in NEIGHBOURS:
                q = (i + a, j + b)
                if 0 <= q[0] < E and 0 <= q[1] < E and q not in grp and q not in reached:
                    reached.add(q)
                    todo.append(q)
        return any((i, j) not in grp and (i, j) not in reached for i in range(E) for j in range(E))

    def win_kind(self, c, colour):
        """bridge / fork / ring / None for the group through the new stone `c`, in the reference's order; self.last keeps what was looked at."""
        grp = self.group(c)
        self.last = {"group": grp, "gates": False, "shortcut": False, "flooded": False}
        if len(grp & self.corners) >= 2:
            return "bridge"
        if sum(bool(grp & s) for s in self.sides) >= 3:
            return "fork"
        if len(grp) < 6 or self.own_neighbours(c, colour) < 2:
            return None
        self.last["gates"] = True
        if any(self.own_neighbours(q, colour) == 6 for q in self.neighbours(c)):  # a neighbour of any colour, empty or not
            self.last["shortcut"] = True
            return "ring"
        self.last["flooded"] = True
        return "ring" if self.hole_bbox(grp) else None

    def act(self, a):
        if not self.is_legal(a):
            return False
        c, colour = self.cell(a), self.turn
        self.owner[c] = colour  # a swap: the cell becomes White's in the same place
        self.actions.append(a)
        self.turn = 3 - colour
        kind = self.win_kind(c, colour)
        self.last["kind"] = kind
        if self.winner == 0 and kind:
            self.winner = colour
        self.fb[colour - 1].add(c)  # only ever set
        self.history.append((frozenset(self.fb[0]), frozenset(self.fb[1])))
        return True

    def is_terminal(self):
        return self.winner != 0 or all(v != 0 for v in self.owner.values())

    def eval_score(self, resign=False):
        w = 3 - self.turn if resign else self.winner
        return 1.0 if w == 1 else (-1.0 if w == 2 else 0.0)

    def features(self):
        """20 planes of E * E: 2k / 2k+1 own / opponent feature bitboards k positions ago, 16 the board, 17 swappable, 18 / 19 black / white to move."""
        E, P = self.E, self.P
        f = np.zeros((20, P), np.float32)
        for k in range(min(8, len(self.history))):
            pos = self.history[-1 - k]
            for c in pos[self.turn - 1]:
                f[2 * k, self.ident(c)] = 1
            for c in pos[2 - self.turn]:
                f[2 * k + 1, self.ident(c)] = 1
        for c in self.valid:
            f[16, self.ident(c)] = 1
        f[17] = 1.0 if self.swappable() else 0.0
        f[18] = 1.0 if self.turn == 1 else 0.0
        f[19] = 1.0 if self.turn == 2 else 0.0
        return f.reshape(-1)

    def feature_bits(self):
        f = self.features().reshape(20, self.P)
        W32 = (self.P + 31) // 32
        out = np.zeros((20, W32), np.uint32)
        for ch in range(20):
            for p in np.nonzero(f[ch])[0]:
                out[ch, p >> 5] |= np.uint32(1 << (int(p) & 31))
        return out.reshape(-1)

    def console(self, a):
        """Console coordinates on the E x E array: column letter (I skipped), row number from 1."""
        i, j = self.cell(a)
        return "ABCDEFGHJKLMNOPQRSTUVWXYZ"[j] + str(i + 1)


# ---- positions by hand: `a` are the stones of the player whose stone comes last (the deciding one last), `b` stones of the other player that matter (played
# first, in order), `avoid` cells that must stay empty.  expect: what the LAST stone's win test finds; winner: 'a', 'b' or None after it.
RING6 = [(2, 3), (2, 4), (3, 4), (4, 3), (4, 2), (3, 2)]                       # around (3, 3), N = 4
RING8 = [(2, 3), (2, 4), (3, 2), (3, 5), (4, 2), (4, 3), (4, 4), (2, 5)]       # around (3, 3) and (3, 4), N = 4; (2, 5) closes it with two own neighbours
ROW1 = [(1, 2), (1, 3), (1, 5), (1, 6)]
# (flooded: the complement flood decides; shortcut: a neighbour of the last stone has six own neighbours — the centre of a ring of six does, empty or not, so
#  the smallest rings never reach the flood)
HAND = {
    "bridge": dict(N=4, a=[(0, 3), (3, 0), (2, 1), (1, 2)], expect="bridge", winner="a"),
    "near_bridge_one_corner_and_the_cell_next_to_another": dict(N=4, a=[(0, 3), (2, 1), (1, 2)], avoid=[(3, 0)], expect=None, winner=None),
    "fork_over_three_sides": dict(N=4, a=ROW1 + [(0, 4), (1, 4)], expect="fork", winner="a"),
    "two_sides_and_a_corner_is_no_fork": dict(N=4, a=ROW1 + [(0, 3), (1, 4)], avoid=[(0, 4), (0, 5), (0, 6), (2, 6)], expect=None, winner=None, flooded=True),
    "ring_of_six_around_an_empty_cell": dict(N=4, a=RING6, avoid=[(3, 3)], expect="ring", winner="a", shortcut=True),
    "ring_around_an_opponent_stone": dict(N=4, a=RING6, b=[(3, 3)], expect="ring", winner="a", shortcut=True),
    "ring_around_two_cells": dict(N=4, a=RING8, avoid=[(3, 3), (3, 4)], expect="ring", winner="a", flooded=True),
    "filled_seven_blob_wins_by_the_shortcut": dict(N=4, a=RING6[1:] + [(3, 3), (2, 3)], expect="ring", winner="a", shortcut=True, no_hole=True),
    "five_cell_c_not_closed": dict(N=4, a=[(2, 3), (2, 4), (3, 4), (4, 3), (4, 2)], avoid=[(3, 3), (3, 2)], expect=None, winner=None),
    "loop_closed_by_a_stone_with_two_own_neighbours": dict(N=4, a=RING8[1:] + [(2, 3)], avoid=[(3, 3), (3, 4)], expect="ring", winner="a", flooded=True, closing_neighbours=2),
    # rings around two cells whose groups lie in two 64-bit words of the bitboards (ids 48 .. 67 at E = 9, 50 .. 81 at E = 15)
    "ring_across_two_words_n5": dict(N=5, a=[(5, 3), (5, 4), (5, 5), (6, 2), (6, 5), (7, 2), (7, 3), (7, 4)], avoid=[(6, 3), (6, 4)], expect="ring", winner="a", flooded=True),
    "ring_across_two_words_n8": dict(N=8, a=[(3, 5), (3, 6), (3, 7), (4, 4), (4, 7), (5, 4), (5, 5), (5, 6)], avoid=[(4, 5), (4, 6)], expect="ring", winner="a", flooded=True),
    # the other player's bridge comes first; the ring that closes afterwards would win too, and does not
    "a_winner_never_goes_away": dict(N=4, a=RING6, b=[(0, 3), (3, 0), (2, 1), (1, 2)], avoid=[(3, 3)], expect="ring", winner="b", shortcut=True),
}
# the swap of a corner cell, as actions (White is the mover by the nature of the rule): afterwards the cell is in both planes and White's, and White's
# bridge runs through it
SWAP_CORNER = dict(N=4, actions=[(0, 3), (0, 3), (6, 0), (1, 2), (6, 1), (2, 1), (5, 0), (3, 0)], expect="bridge", winner=2)


def hand_sequence(name, mover):
    """The actions of HAND[name] with `mover` (1 Black, 2 White) placing the `a` stones, the deciding one last.  The other player places `b`, then filler
    stones: cells that touch no other stone of the filler's colour, none of `a`, `b` or `avoid`, so that they form nothing."""
    h = HAND[name]
    m = Havannah(h["N"])
    a, b = list(h["a"]), list(h.get("b", []))
    need = len(a) - 1 if mover == 1 else len(a)
    taken = set(a) | set(b) | set(h.get("avoid", []))
    others = list(b)
    for c in sorted(m.valid, reverse=True):  # from the far end of the array: the hand positions live near its beginning
        if len(others) >= need:
            break
        if c in taken or c in m.corners or any(q in others for q in m.neighbours(c)):
            continue
        others.append(c)
    assert len(others) >= need, name
    others = others[:need] if len(b) <= need else others
    seq, ai, bi = [], 0, 0
    for ply in range(len(a) + len(others)):
        if (ply % 2) + 1 == mover and ai < len(a):
            seq.append(m.ident(a[ai])); ai += 1
        else:
            seq.append(m.ident(others[bi])); bi += 1
    assert ai == len(a) and bi == len(others) and seq[-1] == m.ident(a[-1]), name
    return h["N"], seq


def play(N, actions, swap=True):
    m = Havannah(N, swap)
    for a in actions:
        assert m.act(a), (N, actions, a)
    return m


# A whole game at N = 4 that fills the 37 cells without a winner: the draw (result 0).  Found by a randomised search while the tests were written (a random
# colouring with 19 black and 18 white cells in which no group holds two corners, meets three sides or surrounds a cell, played in a random order).
DRAW_N4 = [35, 30, 13, 31, 42, 10, 12, 17, 16, 43, 5, 21, 44, 6, 29, 36, 4, 33, 11, 45, 26, 18, 38, 22, 9, 25, 24, 20, 32, 28, 37, 39, 27, 3, 23, 19, 15]


def random_game(N, swap, seed, take_swap=None):
    """A whole game of uniformly random legal actions on the model, from numpy's default_rng(seed).  take_swap (rule on): True = the second action
    repeats the first, False = it does not, None = as drawn.  Returns the model at the end; model.kinds lists (kind, colour) of every action whose win
    test found something (the first one is the game's deciding stone)."""
    rng = np.random.default_rng(seed)
    m = Havannah(N, swap)
    m.kinds = []
    while not m.is_terminal():
        legal = np.nonzero(m.legal_mask())[0]
        if len(m.actions) == 1 and swap and take_swap is not None:
            a = m.actions[0] if take_swap else int(rng.choice([x for x in legal if x != m.actions[0]]))
        else:
            a = int(rng.choice(legal))
        colour = m.turn
        assert m.act(a)
        if m.last["kind"]:
            m.kinds.append((m.last["kind"], colour))
    return m


def replay_record(record, swap):
    """Replay one record `(;GM[..]RE[..]SZ[N]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from Black, every action legal when played,
    no action after the game ended.  Returns (model, RE value, GM name); model.swapped: the second action took the first stone over."""
    import re
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    N = int(re.search(r"SZ\[(\d+)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = Havannah(N, swap)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"action {i} played after the game ended"
        assert colour == ("B" if g.turn == 1 else "W"), f"action {i}: {colour} out of turn"
        assert g.act(int(a)), f"action {i}: {a} is illegal"
    g.swapped = len(g.actions) >= 2 and g.actions[0] == g.actions[1]
    return g, re_value, gm
