"""TicTacToe restated from the rule text (ref environment/tictactoe/tictactoe.cpp), in plain Python, behind the environment interface that
tests/search_model.py plays in.  It imports neither the oracle nor the product."""
import numpy as np

f32 = np.float32


class TicTacToe:
    """environment/tictactoe/tictactoe.cpp: rules, result and the four planes (own, opponent, player 1 to move, player 2 to move)"""
    LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]

    def __init__(self, board=None, to_move=1):
        self.board, self.to_move = list(board or [0] * 9), to_move

    def clone(self): return TicTacToe(self.board, self.to_move)

    def act(self, a, player):
        assert self.board[a] == 0
        self.board[a], self.to_move = player, 3 - player

    def num_players(self): return 2
    def turn(self): return self.to_move
    def legal(self): return [int(b == 0) for b in self.board]

    def winner(self):
        for i, j, k in self.LINES:
            if self.board[i] and self.board[i] == self.board[j] == self.board[k]:
                return self.board[i]
        return 0

    def terminal(self): return self.winner() != 0 or 0 not in self.board
    def eval_score(self): return f32({0: 0.0, 1: 1.0, 2: -1.0}[self.winner()])
    def reward(self): return f32(0)

    def features(self):
        me, you = self.to_move, 3 - self.to_move
        return np.array([b == me for b in self.board] + [b == you for b in self.board] + [me == 1] * 9 + [me == 2] * 9, np.float32)

    def action_features(self, a, player):
        f = np.zeros(9, np.float32)
        f[a] = 1
        return f
