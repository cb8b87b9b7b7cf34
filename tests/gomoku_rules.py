"""A short restatement of the reference's Gomoku rules (environment/gomoku/gomoku.cpp), written from the rule text: the stand-in for an oracle on
both sides of tests/test_gomoku_env.py and tests/test_gpu_gomoku.py.

- act (gomoku.cpp:23-32): the stone goes down, the turn passes, and the winner is REPLACED by the result of this move alone;
- a move wins when one of the four lines through its stone (row, column, both diagonals; gomoku.cpp:140-162) holds exactly five of the mover's
  stones (exactly_five, the default), or five or more (freestyle);
- legality (gomoku.cpp:48-58): an empty point; under outer_open the game's first move (no move played yet) is any point of the outer two rings;
- terminal (gomoku.cpp:60-63): a winner, or no empty point left; eval (65-73): +1 black won, -1 white won, 0 otherwise; resigning: the player
  not to move is scored;
- features (75-98): own stones, opponent stones, black to move, white to move, each plane read through the reversed rotation."""
import numpy as np

REVERSED = [0, 3, 2, 1, 4, 5, 6, 7]


def rotate_pos(rot, pos, n):
    """ref utils/rotation.h: float centre arithmetic with truncation."""
    c = (n - 1) / 2.0
    x, y = pos % n - c, pos // n - c
    rx, ry = {0: (x, y), 1: (y, -x), 2: (-x, -y), 3: (-y, x), 4: (x, -y), 5: (-y, -x), 6: (-x, y), 7: (y, x)}[rot]
    return int((ry + c) * n + (rx + c))


class Gomoku:
    def __init__(self, n=15, outer_open=False, exactly_five=True):
        self.n, self.outer_open, self.exactly_five = n, outer_open, exactly_five
        self.reset()

    def reset(self):
        self.board = [0] * (self.n * self.n)
        self.turn = 1
        self.winner = 0
        self.actions = []

    def is_legal(self, a):
        n = self.n
        if not 0 <= a < n * n:
            return False
        if self.outer_open and not self.actions:
            i, j = a // n, a % n
            return i < 2 or i >= n - 2 or j < 2 or j >= n - 2
        return self.board[a] == 0

    def legal_mask(self):
        return np.array([1 if self.is_legal(a) else 0 for a in range(self.n * self.n)], np.uint8)

    def line(self, a, dx, dy):
        n, who = self.n, self.board[a]
        count = 1
        for s in (1, -1):
            x, y = a % n + s * dx, a // n + s * dy
            while 0 <= x < n and 0 <= y < n and self.board[y * n + x] == who:
                count += 1
                x, y = x + s * dx, y + s * dy
        return count

    def wins(self, a):
        for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
            k = self.line(a, dx, dy)
            if (k == 5) if self.exactly_five else (k >= 5):
                return True
        return False

    def act(self, a, player=None):
        player = self.turn if player is None else player
        if not self.is_legal(a):
            return False
        self.board[a] = player
        self.actions.append(a)
        self.turn = 3 - player
        self.winner = player if self.wins(a) else 0
        return True

    def is_terminal(self):
        return self.winner != 0 or 0 not in self.board

    def eval_score(self, resign=False):
        who = (3 - self.turn) if resign else self.winner
        return {1: 1.0, 2: -1.0}.get(who, 0.0)

    def features(self, rot=0):
        n, P = self.n, self.n * self.n
        own, opp = self.turn, 3 - self.turn
        f = np.zeros((4, P), np.float32)
        for p in range(P):
            q = rotate_pos(REVERSED[rot], p, n)
            f[0, p] = self.board[q] == own
            f[1, p] = self.board[q] == opp
        f[2, :] = self.turn == 1
        f[3, :] = self.turn == 2
        return f.reshape(-1)

    def feature_bits(self, rot=0):
        P = self.n * self.n
        W32 = (P + 31) // 32
        f = self.features(rot).reshape(4, P)
        out = np.zeros(4 * W32, np.uint32)
        for c in range(4):
            for p in np.nonzero(f[c])[0]:
                out[c * W32 + p // 32] |= np.uint32(1 << (int(p) % 32))
        return out


def replay_record(record, n, outer_open, exactly_five):
    """Replay one record `(;GM[..]RE[..]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from black, every move legal when played,
    no move after the game ended (the first winning move or the full board ends it).  Returns (model, RE value, GM name)."""
    import re
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = Gomoku(n, outer_open, exactly_five)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"move {i} played after the game ended"
        assert colour == ("B" if g.turn == 1 else "W"), f"move {i}: {colour} out of turn"
        assert g.act(int(a)), f"move {i}: {a} is illegal"
    return g, re_value, gm
