"""A short restatement of the reference's Hex rules (environment/hex/hex.{h,cpp}), written from the rule text: the stand-in for an oracle on both
sides of tests/test_hex_env.py and tests/test_gpu_hex.py.

- board n x n, action a = row * n + col, Black (1) first, the turn passes on every accepted action (the swap included);
- the neighbours of (col x, row y) are (x-1,y-1) (x,y-1) (x-1,y) (x+1,y) (x,y+1) (x+1,y+1) (hex.cpp:319-336); (x+1,y-1) and (x-1,y+1) are NOT adjacent;
- Black connects column 0 with column n-1, White row 0 with row n-1 (hex.cpp:51-61); after a move the mover wins when the mover's connected group
  through the new stone touches both of the mover's edges — found here by a plain breadth-first search, on purpose not the algorithm of either
  product engine (a stack flood on the host, a bitboard dilation on the device) nor the reference's (edge flags propagated recursively);
- a winner never goes away; terminal <=> a winner exists (hex.cpp:101-104); eval +1 / -1 / 0, resigning scores the player not to move (106-116);
- legality (86-99): an empty cell; with the swap rule, exactly one action played makes EVERY cell legal;
- swap (28-47): rule on, one action played, the action equals the first one: that cell is cleared and a stone of the mover goes on
  (n-1-col) * n + (n-1-row) where (row, col) is the first stone; the record keeps the chosen action id;
- features (118-141): own stones, opponent stones, Black to move, White to move; the rotation argument is ignored."""
from collections import deque

import numpy as np

NEIGHBOURS = ((-1, -1), (0, -1), (-1, 0), (1, 0), (0, 1), (1, 1))


class Hex:
    def __init__(self, n=11, swap=True):
        self.n, self.swap = n, swap
        self.reset()

    def reset(self):
        self.board = [0] * (self.n * self.n)
        self.turn = 1
        self.winner = 0
        self.actions = []
        self.swapped = False

    def is_legal(self, a):
        if not 0 <= a < self.n * self.n:
            return False
        return (self.swap and len(self.actions) == 1) or self.board[a] == 0

    def legal_mask(self):
        return np.array([1 if self.is_legal(a) else 0 for a in range(self.n * self.n)], np.uint8)

    def group(self, p):
        n, who = self.n, self.board[p]
        seen, queue = {p}, deque([p])
        while queue:
            q = queue.popleft()
            x, y = q % n, q // n
            for dx, dy in NEIGHBOURS:
                u, v = x + dx, y + dy
                if 0 <= u < n and 0 <= v < n and self.board[v * n + u] == who and v * n + u not in seen:
                    seen.add(v * n + u)
                    queue.append(v * n + u)
        return seen

    def connects(self, p):
        n, who = self.n, self.board[p]
        along = [(q % n if who == 1 else q // n) for q in self.group(p)]
        return 0 in along and n - 1 in along

    def act(self, a, player=None):
        player = self.turn if player is None else player
        if not self.is_legal(a):
            return False
        n, p = self.n, a
        if self.swap and len(self.actions) == 1 and a == self.actions[0]:
            self.board[a] = 0
            p = (n - 1 - a % n) * n + (n - 1 - a // n)
            self.swapped = True
        self.board[p] = player
        self.actions.append(a)
        self.turn = 3 - player
        if self.winner == 0 and self.connects(p):
            self.winner = player
        return True

    def is_terminal(self):
        return self.winner != 0

    def eval_score(self, resign=False):
        who = (3 - self.turn) if resign else self.winner
        return {1: 1.0, 2: -1.0}.get(who, 0.0)

    def features(self, rot=0):
        P = self.n * self.n
        f = np.zeros((4, P), np.float32)
        b = np.array(self.board)
        f[0] = b == self.turn
        f[1] = b == 3 - self.turn
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


def replay_record(record, n, swap):
    """Replay one record `(;GM[..]RE[..]...;B[a]...;W[a]...)` on the model.  Checks: alternating players from Black, every action legal when played,
    no action after the game ended.  Returns (model, RE value, GM name)."""
    import re
    gm = re.search(r"GM\[([^\]]*)\]", record).group(1)
    re_value = float(re.search(r"RE\[([^\]]*)\]", record).group(1))
    moves = re.findall(r";([BW])\[(\d+)\]", record)
    g = Hex(n, swap)
    for i, (colour, a) in enumerate(moves):
        assert not g.is_terminal(), f"action {i} played after the game ended"
        assert colour == ("B" if g.turn == 1 else "W"), f"action {i}: {colour} out of turn"
        assert g.act(int(a)), f"action {i}: {a} is illegal"
    return g, re_value, gm
