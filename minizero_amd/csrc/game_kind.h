// The board games with a device twin, described once: the value stored in GoDevView::kind, and every fact about a game that code outside its own
// rules (env.cpp: the host class; go_body.h: the leaf body) needs.  Plain header of constexpr facts: host code (g++) and device code (hipcc) both include it.
// Adding a game: INTEGRATION.md "Adding a board game".
#pragma once

namespace mz {

// The values are stored in GoDevView::kind; kNoDeviceGame is what an engine without a device twin reports: the Atari-shaped environment.
enum GameKind : int { kGo = 0, kOthello = 1, kTicTacToe = 2, kGomoku = 3, kHex = 4, kNoGo = 5, kHavannah = 6, kNoDeviceGame = -1 };
constexpr int kNumGameKinds = 7;

// The rules argument of the kernels (their template parameter `int CPL`): for Go the 64-bit words per plane of the board, positive (rulesArg below computes it);
// for the other games a sentinel that selects the leaf body (go_body.h leafBody).  The values are part of the kernels' mangled names.
constexpr int kRulesWordsPerPlane = 1;
constexpr int kRulesOthello = 0, kRulesTicTacToe = -1, kRulesGomoku = -2, kRulesHex = -3, kRulesNoGo = -4, kRulesHavannah = -5;

// One row per game, in enum order: env_game name; feature planes; has a pass action; smallest / default / largest board with a device twin (as env_board_size
// counts them); the rules argument; hex_array: a hexagon of edge size n kept in a (2n - 1) x (2n - 1) array (networkBoard below); variant_of: the kind whose
// network shape and record loader the game shares — itself, unless the game is a RULES VARIANT, which differs from that kind in its rules alone (a host class
// and a leaf body of its own).  NoGo is a variant of Go (ref nogo.h:18 NoGoEnv derives from GoEnv; its boards end at 9x9, nogo.h:12,22; the pass slot is in
// the policy, and never legal).  Havannah: ref havannah.h: assert(board_size >= 4), default 8; edge size 10 is a 19 x 19 array, what kGoMaxW words hold (go_dev.h).
struct GameRow { const char* name; int channels; bool has_pass; int min_board, default_board, max_board; int rules; bool hex_array; GameKind variant_of; };
constexpr GameRow kGameTable[kNumGameKinds] = {
    {"go", 18, true, 2, 9, 19, kRulesWordsPerPlane, false, kGo},
    {"othello", 4, true, 4, 8, 8, kRulesOthello, false, kOthello},
    {"tictactoe", 4, false, 3, 3, 3, kRulesTicTacToe, false, kTicTacToe},
    {"gomoku", 4, false, 2, 15, 19, kRulesGomoku, false, kGomoku},
    {"hex", 4, false, 2, 11, 19, kRulesHex, false, kHex},
    {"nogo", 18, true, 2, 9, 9, kRulesNoGo, false, kGo},
    {"havannah", 20, false, 4, 8, 10, kRulesHavannah, true, kHavannah},
};

constexpr bool isDeviceGame(int k) { return k >= 0 && k < kNumGameKinds; }
constexpr bool isGameVariant(int k) { return isDeviceGame(k) && kGameTable[k].variant_of != k; }
constexpr GameKind gameRow(GameKind k) { return kGameTable[k].variant_of; } // the kind whose network shape and loader a kind uses (itself unless a variant)
constexpr bool gameHasPass(GameKind k) { return kGameTable[k].has_pass; }
constexpr int gameChannels(GameKind k) { return kGameTable[k].channels; }
constexpr int gameMinBoard(GameKind k) { return kGameTable[k].min_board; }
constexpr int gameDefaultBoard(GameKind k) { return kGameTable[k].default_board; }
constexpr int gameMaxBoard(GameKind k) { return kGameTable[k].max_board; }
constexpr const char* gameName(GameKind k) { return kGameTable[k].name; }
// The NETWORK BOARD of a game at env_board_size n: the side of the square array the planes, the policy, the bitboards and the kernels' H and W are made of.
// Havannah's edge size N plays on a (2N - 1) x (2N - 1) array with two corners cut off (ref havannah.h: extended_board_size_); everywhere else it is n.
constexpr int networkBoard(GameKind k, int n) { return kGameTable[k].hex_array ? 2 * n - 1 : n; }

// the game of an env_game string; kNoDeviceGame: not in the table ("atari", or unknown)
inline GameKind gameFromName(const char* env_game)
{
    for (int k = 0; k < kNumGameKinds; ++k) {
        const char* a = gameName(static_cast<GameKind>(k));
        const char* b = env_game;
        while (*a && *a == *b) { ++a; ++b; }
        if (*a == 0 && *b == 0) { return static_cast<GameKind>(k); }
    }
    return kNoDeviceGame;
}

// the rules argument of a kind on a network board of side board_n (a kind without a row is asked about like Go: no kernel instance has its answer)
constexpr int rulesArg(int kind, int board_n)
{
    return isDeviceGame(kind) && kGameTable[kind].rules != kRulesWordsPerPlane ? kGameTable[kind].rules : (board_n * board_n + 63) / 64;
}

} // namespace mz
