"""Othello's rules restated from the rule text (ref environment/othello/othello.cpp:13-36,103-140,195-255), in plain Python and with none of env.cpp's
or o_env.cpp's data structures: a list of colours per point and a walk along each of the 8 directions that returns the discs it would flip as a list.
It imports neither the oracle nor the product.

The rules.  Boards 4, 6, 8; P = n * n points plus the pass (action P).  The start: Black on the lower-left and upper-right of the four centre points
(point (n/2 - 1) * n + n/2 - 1 and the one diagonally above), White on the other two; Black moves first.  A player may place a disc on an empty point
from which, in at least one of the 8 directions, an unbroken line of enemy discs is followed by an own disc; all such lines are flipped.  The pass is
legal exactly when the player has no placing move.  The game is over after two consecutive passes and not before: a full board still needs them.  The
result is the disc count (+1 Black has more, -1 White, 0 equal), and it is 0 at every position where either side can still place (othello.cpp:225).
After a resignation the side to move has lost.  The 4 planes: own discs, opponent discs through the reversed rotation, black-to-move, white-to-move."""
import re

import numpy as np

from go_rules import _source_points, pack_bits

EMPTY, BLACK, WHITE = 0, 1, 2
DIRECTIONS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


class Othello:
    def __init__(self, n=8):
        assert n in (4, 6, 8), n
        self.n = n
        self.board = [EMPTY] * (n * n)
        h = n // 2
        self.board[(h - 1) * n + h - 1] = self.board[h * n + h] = BLACK
        self.board[(h - 1) * n + h] = self.board[h * n + h - 1] = WHITE
        self.turn = BLACK
        self.actions = []   # (action, player)
        self._undo = []     # (board before, turn before)

    @property
    def P(self):
        return self.n * self.n

    def flips(self, a, player):
        """the enemy discs that `player` turns over by placing on the empty point a"""
        n, out = self.n, []
        for dx, dy in DIRECTIONS:
            x, y, line = a % n + dx, a // n + dy, []
            while 0 <= x < n and 0 <= y < n and self.board[y * n + x] == 3 - player:
                line.append(y * n + x)
                x, y = x + dx, y + dy
            if line and 0 <= x < n and 0 <= y < n and self.board[y * n + x] == player:
                out += line
        return out

    def can_place(self, player):
        return any(self.board[a] == EMPTY and self.flips(a, player) for a in range(self.P))

    def is_legal(self, a, player=None):
        player = self.turn if player is None else player
        if a == self.P:
            return not self.can_place(player)
        return 0 <= a < self.P and self.board[a] == EMPTY and bool(self.flips(a, player))

    def legal_mask(self):
        return np.array([self.is_legal(a) for a in range(self.P + 1)], np.uint8)

    def act(self, a, player=None):
        player = self.turn if player is None else player
        if not self.is_legal(a, player):
            return False
        self._undo.append((list(self.board), self.turn))
        if a != self.P:
            for q in self.flips(a, player) + [a]:
                self.board[q] = player
        self.turn = 3 - player
        self.actions.append((a, player))
        return True

    def undo(self):
        self.actions.pop()
        self.board, self.turn = self._undo.pop()

    def clone(self):
        g = type(self)(self.n)
        g.board, g.turn, g.actions, g._undo = list(self.board), self.turn, list(self.actions), list(self._undo)
        return g

    def is_terminal(self):
        return len(self.actions) >= 2 and self.actions[-1][0] == self.P and self.actions[-2][0] == self.P

    def eval_score(self, resign=False):
        if resign:
            return 1.0 if self.turn == WHITE else -1.0
        if self.can_place(BLACK) or self.can_place(WHITE):
            return 0.0
        b, w = self.board.count(BLACK), self.board.count(WHITE)
        return 1.0 if b > w else -1.0 if b < w else 0.0

    def features(self, rot=0):
        P = self.P
        f = np.zeros((4, P), np.float32)
        b = np.array(self.board)[_source_points(self.n, rot)]
        f[0] = b == self.turn
        f[1] = b == 3 - self.turn
        f[2, :] = self.turn == BLACK
        f[3, :] = self.turn == WHITE
        return f.reshape(-1)

    def feature_bits(self, rot=0):
        return pack_bits(self.features(rot).reshape(4, self.P))


def replay_record(record, n):
    """Replay one record `(;GM[..]RE[..]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from Black, every action legal when played,
    no action after the game ended.  Returns (model, RE value, GM name)."""
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = Othello(n)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"action {i} played after the game ended"
        assert colour == ("B" if g.turn == BLACK else "W"), f"action {i}: {colour} out of turn"
        assert g.act(int(a)), f"action {i}: {a} is illegal"
    return g, re_value, gm
