"""Go's rules restated from the rule text (ref environment/go/go.cpp:45-49,132-308,703-723), in plain Python and with none of env.cpp's or o_env.cpp's
data structures: a list of colours per point, a flood fill per block that returns its stones and its liberties as sets, a flood fill per empty region
that returns its points and the colours it touches.  It imports neither the oracle nor the product: the host engine, the oracle's restatement, the
device engine, the worker's records, the search and the sampler are checked against this model.

The rules.  P = n * n points plus the pass (action P), which is always legal.  An occupied point is illegal.  A stone placed removes every adjacent
enemy block that is left without a liberty; a move after which the mover's own block has no liberty and nothing was removed is suicide and illegal
(a move that captures is never suicide).  Superko: a move is illegal if the position it creates is in the set of positions after every earlier action,
passes included (a pass adds the unchanged position); the empty start is not in the set.  env_go_ko_rule=positional compares the stones only,
situational the stones and the side to move after the action.  The game is over after two consecutive passes, or after more than 2 * n * n actions.
The result is Tromp-Taylor area: stones plus the empty regions that touch one colour only, env_go_komi added to White; an empty region that touches no
stone at all goes to Black (the reference's quirk, go.cpp:713: the test is "nothing around it that is not black"); equal areas are a draw.  After a
resignation the side to move has lost.  The 18 planes: own / opponent stones of the last 8 positions (after each action, passes included) through the
reversed rotation, then black-to-move and white-to-move.

Positions are kept exactly, as tuples.  The product and the oracle keep 64-bit Zobrist keys instead, so they can differ from this model only where two
different positions of one game share a key: a hash collision, of probability about (game length)^2 / 2^65 per game."""
import re

import numpy as np

from nogo_rules import REVERSED, rotate_point

EMPTY, BLACK, WHITE = 0, 1, 2


class Go:
    def __init__(self, n, komi=7.5, ko_rule="positional"):
        assert ko_rule in ("positional", "situational"), ko_rule
        self.n, self.komi, self.ko_rule = n, float(komi), ko_rule
        self.board = [EMPTY] * (n * n)
        self.turn = BLACK
        self.actions = []   # (action, player)
        self.history = []   # the board after every action, as a tuple
        self.seen = set()   # the superko set: the key of the position after every action
        self._undo = []     # what undo() needs: (turn before, key added to `seen` by this action or None)
        self._libs = None   # point -> number of liberties of its block, for the position on the board; None: not counted yet

    # ---- geometry -----------------------------------------------------------------------------------------------------------------------------------
    @property
    def P(self):
        return self.n * self.n

    def neighbours(self, p):
        n, x, y = self.n, p % self.n, p // self.n
        return [q for q, ok in ((p - n, y > 0), (p + n, y < n - 1), (p - 1, x > 0), (p + 1, x < n - 1)) if ok]

    def block(self, p, board=None):
        """(stones, liberties) of the block through the stone at p."""
        board = self.board if board is None else board
        colour, stones, libs, todo = board[p], {p}, set(), [p]
        while todo:
            for q in self.neighbours(todo.pop()):
                if board[q] == EMPTY:
                    libs.add(q)
                elif board[q] == colour and q not in stones:
                    stones.add(q)
                    todo.append(q)
        return stones, libs

    # ---- moves --------------------------------------------------------------------------------------------------------------------------------------
    def place(self, a, player):
        """The board after `player` puts a stone on the empty point a, and the enemy blocks removed (a list of sets); None if the move is suicide.
        No superko here."""
        board = list(self.board)
        board[a] = player
        captured = []
        for q in self.neighbours(a):
            if board[q] == 3 - player:
                stones, libs = self.block(q, board)
                if not libs:
                    captured.append(stones)
                    for s in stones:
                        board[s] = EMPTY
        if not captured and not self.block(a, board)[1]:
            return None, []
        return board, captured

    def _quiet(self, a, player):
        """True if a stone of `player` on the empty point a has an empty neighbour and no adjacent enemy block is down to its last liberty: then the move
        neither captures nor is suicide.  The liberty counts of the blocks on the board are found once per position."""
        if self._libs is None:
            self._libs = {}
            for p in range(self.P):
                if self.board[p] != EMPTY and p not in self._libs:
                    stones, libs = self.block(p)
                    for s in stones:
                        self._libs[s] = len(libs)
        nb = self.neighbours(a)
        return any(self.board[q] == EMPTY for q in nb) and not any(self.board[q] == 3 - player and self._libs[q] == 1 for q in nb)

    def key(self, board, to_move):
        return tuple(board) if self.ko_rule == "positional" else (tuple(board), to_move)

    def refusal(self, a, player=None):
        """Why the point a is illegal for `player`: None (legal), 'occupied', 'suicide', or ('superko', how many plies before the one asked about the repeated position
        was last created: 2 is the simple ko)."""
        player = self.turn if player is None else player
        if a == self.P:
            return None
        if self.board[a] != EMPTY:
            return "occupied"
        if self._quiet(a, player):  # the common case without a flood fill per candidate: the stone stays, nothing is removed
            board = list(self.board)
            board[a] = player
        else:
            board, _ = self.place(a, player)
        if board is None:
            return "suicide"
        k = self.key(board, 3 - player)
        if k in self.seen:
            t = tuple(board)
            age = next(i for i in range(1, len(self.history) + 1) if self.history[-i] == t and (self.ko_rule == "positional" or self.actions[-i][1] == player))
            return ("superko", age)
        return None

    def is_legal(self, a, player=None):
        return 0 <= a <= self.P and self.refusal(a, player) is None

    def legal_mask(self):
        return np.array([self.is_legal(a) for a in range(self.P + 1)], np.uint8)

    def act(self, a, player=None):
        player = self.turn if player is None else player
        if not self.is_legal(a, player):
            return False
        before, self._libs = self.turn, None
        if a != self.P:
            self.board, _ = self.place(a, player)
        self.turn = 3 - player
        self.actions.append((a, player))
        self.history.append(tuple(self.board))
        k = self.key(self.board, self.turn)
        self._undo.append((before, None if k in self.seen else k))
        self.seen.add(k)
        return True

    def undo(self):
        self.actions.pop()
        self.history.pop()
        self._libs = None
        self.turn, k = self._undo.pop()
        if k is not None:
            self.seen.remove(k)
        self.board = list(self.history[-1]) if self.history else [EMPTY] * self.P

    def clone(self):
        g = type(self)(self.n, self.komi, self.ko_rule)
        g.board, g.turn, g.actions, g.history, g.seen, g._undo = list(self.board), self.turn, list(self.actions), list(self.history), set(self.seen), list(self._undo)
        return g

    # ---- ending and result --------------------------------------------------------------------------------------------------------------------------
    def is_terminal(self):
        if len(self.actions) >= 2 and self.actions[-1][0] == self.P and self.actions[-2][0] == self.P:
            return True
        return len(self.actions) > 2 * self.P

    def areas(self):
        """(Black's area, White's area without komi)"""
        area = [0, self.board.count(BLACK), self.board.count(WHITE)]
        done = set()
        for p in range(self.P):
            if self.board[p] != EMPTY or p in done:
                continue
            region, touches, todo = {p}, set(), [p]
            while todo:
                for q in self.neighbours(todo.pop()):
                    if self.board[q] != EMPTY:
                        touches.add(self.board[q])
                    elif q not in region:
                        region.add(q)
                        todo.append(q)
            done |= region
            if WHITE not in touches:   # only Black, or nothing at all: the reference's quirk
                area[BLACK] += len(region)
            elif BLACK not in touches:
                area[WHITE] += len(region)
        return area[BLACK], area[WHITE]

    def eval_score(self, resign=False):
        if resign:
            return 1.0 if self.turn == WHITE else -1.0
        b, w = self.areas()
        w += self.komi
        return 1.0 if b > w else -1.0 if b < w else 0.0

    # ---- planes -------------------------------------------------------------------------------------------------------------------------------------
    def features(self, rot=0):
        n, P = self.n, self.P
        f = np.zeros((18, P), np.float32)
        src = _source_points(n, rot)
        for k in range(min(8, len(self.history))):
            b = np.array(self.history[-1 - k])[src]
            f[2 * k] = b == self.turn
            f[2 * k + 1] = b == 3 - self.turn
        f[16, :] = self.turn == BLACK
        f[17, :] = self.turn == WHITE
        return f.reshape(-1)

    def feature_bits(self, rot=0):
        return pack_bits(self.features(rot).reshape(18, self.P))


_SRC = {}


def _source_points(n, rot):
    """plane point p shows board point rotate_point(REVERSED[rot], p)"""
    if (n, rot) not in _SRC:
        _SRC[n, rot] = np.array([rotate_point(REVERSED[rot], p, n) for p in range(n * n)])
    return _SRC[n, rot]


def pack_bits(planes):
    """(C, P) 0/1 planes -> C * ceil(P / 32) uint32 words, point p of a plane at bit p % 32 of its word p // 32"""
    C, P = planes.shape
    W32 = (P + 31) // 32
    bits = np.zeros((C, W32 * 32), np.uint64)
    bits[:, :P] = planes != 0
    return (bits.reshape(C, W32, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).reshape(-1)


def replay_record(record, n, komi=7.5, ko_rule="positional"):
    """Replay one record `(;GM[..]RE[..]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from Black, every action legal when played,
    no action after the game ended.  Returns (model, RE value, GM name)."""
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = Go(n, komi, ko_rule)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"action {i} played after the game ended"
        assert colour == ("B" if g.turn == BLACK else "W"), f"action {i}: {colour} out of turn"
        assert g.act(int(a)), f"action {i}: {a} is illegal"
    return g, re_value, gm
