"""NoGo's rules restated from the rule text (ref environment/nogo/nogo.h:25-76 over GoEnv, go.cpp:132-190,280-308), in plain Python and with none of
env.cpp's data structures: a list of colours per point and a flood fill per block that returns its stones and its liberties as sets.  There is no oracle for this game: the host engine,
the device engine and the worker's records are checked against this model.

The rules: the board and the actions are Go's (P points + the pass slot, which is never legal).  An empty point p is legal for player c iff no
orthogonally adjacent enemy block has exactly one liberty (that liberty is p: the move would capture) and some neighbour of p is empty or some adjacent
block of c has more than one liberty (else the move is suicide).  A move places a stone; nothing is ever removed.  The game is over when the player to
move has no legal point; the player NOT to move has won (+1 Black, -1 White), resign or not.  The planes are Go's: own / opponent stones of the last 8
positions under the rotation, then black-to-move and white-to-move."""
import numpy as np


def rotate_point(rot, p, n):
    """ref utils/rotation.h: the position `p` under rotation `rot` (float centre arithmetic, truncated)."""
    c = (n - 1) / 2.0
    x, y = p % n - c, p // n - c
    rx, ry = [(x, y), (y, -x), (-x, -y), (-y, x), (x, -y), (-y, -x), (-x, y), (y, x)][rot]
    return int((ry + c) * n + (rx + c))


REVERSED = [0, 3, 2, 1, 4, 5, 6, 7]


class NoGo:
    def __init__(self, n):
        self.n = n
        self.board = [0] * (n * n)  # 0 empty, 1 black, 2 white
        self.turn = 1
        self.actions = []
        self.history = []  # the board after every action

    def neighbours(self, p):
        n, x, y = self.n, p % self.n, p // self.n
        return [q for q, ok in ((p - n, y > 0), (p + n, y < n - 1), (p - 1, x > 0), (p + 1, x < n - 1)) if ok]

    def block(self, p):
        """(stones, liberties) of the block through the stone at p."""
        colour, stones, libs, todo = self.board[p], {p}, set(), [p]
        while todo:
            for q in self.neighbours(todo.pop()):
                if self.board[q] == 0:
                    libs.add(q)
                elif self.board[q] == colour and q not in stones:
                    stones.add(q)
                    todo.append(q)
        return stones, libs

    def is_legal(self, a, player=None):
        player = self.turn if player is None else player
        if a < 0 or a >= self.n * self.n or self.board[a] != 0:
            return False
        alive = False
        for q in self.neighbours(a):
            if self.board[q] == 0:
                alive = True
                continue
            libs = len(self.block(q)[1])
            if self.board[q] == player:
                alive = alive or libs > 1
            elif libs == 1:
                return False  # captures
        return alive

    def legal_mask(self):
        P = self.n * self.n
        return np.array([self.is_legal(a) for a in range(P)] + [False], np.uint8)

    def act(self, a, player=None):
        player = self.turn if player is None else player
        if not self.is_legal(a, player):
            return False
        self.board[a] = player
        self.actions.append(a)
        self.turn = 3 - player
        self.history.append(list(self.board))
        return True

    def undo(self):
        a = self.actions.pop()
        self.history.pop()
        self.turn = self.board[a]
        self.board[a] = 0

    def is_terminal(self):
        return not any(self.is_legal(a) for a in range(self.n * self.n))

    def eval_score(self, resign=False):
        return 1.0 if self.turn == 2 else -1.0

    def features(self, rot=0):
        n, P = self.n, self.n * self.n
        f = np.zeros((18, P), np.float32)
        src = np.array([rotate_point(REVERSED[rot], p, n) for p in range(P)])
        for k in range(min(8, len(self.history))):
            b = np.array(self.history[-1 - k])[src]
            f[2 * k] = b == self.turn
            f[2 * k + 1] = b == 3 - self.turn
        f[16, :] = self.turn == 1
        f[17, :] = self.turn == 2
        return f.reshape(-1)

    def feature_bits(self, rot=0):
        P = self.n * self.n
        W32 = (P + 31) // 32
        f = self.features(rot).reshape(18, P)
        out = np.zeros(18 * W32, np.uint32)
        for c in range(18):
            for p in np.nonzero(f[c])[0]:
                out[c * W32 + p // 32] |= np.uint32(1 << (int(p) % 32))
        return out


def model_legal_moves(n):
    """legal_moves callback of count_tree over the model."""
    def legal(actions):
        g = NoGo(n)
        for a in actions:
            assert g.act(a)
        return [a for a in range(n * n) if g.is_legal(a)]
    return legal


def count_tree(n, depth, legal_moves):
    """The move tree from the empty board, `depth` levels deep, by the rules behind `legal_moves(actions) -> legal actions of the player to move`:
    ([sequences of length 1, of length 2, ...], {(length, winner): finished games}).  Nothing is ever captured, so a position is the two sets of
    stones; positions reached by several move orders are expanded once and counted as often as they are reached."""
    memo = {}

    def walk(actions, left):
        key = (frozenset(actions[0::2]), frozenset(actions[1::2]), left)
        if key not in memo:
            legal = legal_moves(actions)
            counts, ended = [0] * left, {}
            if not legal:
                ended[(0, 1 if len(actions) % 2 == 1 else 2)] = 1  # the player who moved last has won
            else:
                counts[0] = len(legal)
                if left > 1:
                    for a in legal:
                        cc, ee = walk(actions + (a,), left - 1)
                        for i, v in enumerate(cc):
                            counts[i + 1] += v
                        for (l, w), v in ee.items():
                            ended[(l + 1, w)] = ended.get((l + 1, w), 0) + v
            memo[key] = (counts, ended)
        return memo[key]
    return walk((), depth)


# ---- positions by hand ------------------------------------------------------------------------------------------------------------------------------
# (mover's stones, enemy's stones, the point in question, is it legal for the mover) on a 9x9 board, (x, y) with y the row; every list is in an order
# in which each stone is legal when it is placed
HAND = {
    "capture": ([(1, 0)], [(0, 0)], (0, 1), False),                                        # the enemy stone (0, 0) has one liberty left: the point
    "single-stone suicide": ([], [(1, 0), (0, 1)], (0, 0), False),
    "multi-stone suicide": ([(0, 0), (2, 0)], [(0, 1), (1, 1), (2, 1), (3, 0)], (1, 0), False),  # both own blocks in atari, no empty neighbour
    "one block with two liberties": ([(0, 0), (2, 0)], [(0, 1), (1, 1), (2, 1)], (1, 0), True),  # ... and (2, 0) keeps (3, 0)
    "safe own block": ([(1, 0)], [(0, 1)], (0, 0), True),                                   # no empty neighbour, legal through (1, 0)
    "shared block": ([(0, 0), (0, 1), (1, 1)], [(0, 2), (1, 2), (2, 1), (2, 0)], (1, 0), False),  # one own block on two sides: the point is ONE liberty
}
FILLERS = [(0, 8), (2, 8), (4, 8), (6, 8), (8, 8), (0, 6), (2, 6), (4, 6), (6, 6), (8, 6)]  # lone stones far from the corner the positions are in


def hand_sequence(name, mover, n=9):
    """The position `name` as alternating actions from Black, after which `mover` (1 black, 2 white) is to move: (actions, point, legal)."""
    mine, theirs, point, legal = HAND[name]
    k_mine = max(len(mine), len(theirs) - (mover == 2))
    k_theirs = k_mine + (mover == 2)
    fill = iter(FILLERS)
    mine = list(mine) + [next(fill) for _ in range(k_mine - len(mine))]
    theirs = list(theirs) + [next(fill) for _ in range(k_theirs - len(theirs))]
    first, second = (mine, theirs) if mover == 1 else (theirs, mine)
    seq = []
    for i in range(len(first)):
        seq.append(first[i])
        if i < len(second):
            seq.append(second[i])
    return [y * n + x for x, y in seq], point[1] * n + point[0], legal


def spiral_chain(n=9):
    """80 alternating actions on 9x9: a Black chain of 40 stones that spirals inward from the corner (over points 63 and 72: both words of the bitboard),
    White on every other point but (0, 1).  White's last stone, at (7, 1), takes the chain's second-to-last liberty: Black is left without a move."""
    black = [(x, 0) for x in range(9)] + [(8, y) for y in range(1, 9)] + [(x, 8) for x in range(7, -1, -1)] + [(0, y) for y in range(7, 1, -1)] \
        + [(x, 2) for x in range(1, 7)] + [(6, y) for y in range(3, 6)]
    corridor = [(x, 1) for x in range(0, 8)] + [(7, y) for y in range(2, 8)] + [(x, 7) for x in range(6, 0, -1)] + [(1, y) for y in range(6, 2, -1)] \
        + [(x, 3) for x in range(2, 6)]
    inner = [(x, y) for y in range(4, 7) for x in range(2, 7) if (x, y) not in black and (x, y) not in corridor]
    white = [p for p in inner[::-1] + corridor[::-1] if p not in ((0, 1), (7, 1))] + [(7, 1)]
    assert len(black) == 40 and len(white) == 40 and len(set(black) | set(white)) == 80
    return [y * n + x for pair in zip(black, white) for x, y in pair]


def replay_record(record, n):
    """Replay one record `(;GM[..]RE[..]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from Black, every action legal when played,
    no action after the game ended.  Returns (model, RE value, GM name)."""
    import re
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = NoGo(n)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"action {i} played after the game ended"
        assert colour == ("B" if g.turn == 1 else "W"), f"action {i}: {colour} out of turn"
        assert g.act(int(a)), f"action {i}: {a} is illegal"
    return g, re_value, gm
