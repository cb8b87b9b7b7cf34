// The board games with a device twin, described once: the value stored in GoDevView::kind, and every fact about a game that code outside its own
// rules (env.cpp: the host class; go_body.h: the leaf body) needs.  Plain header of constexpr facts: host code (g++) and device code (hipcc) both include it.
// Adding a game: INTEGRATION.md "Adding a board game".
#pragma once

namespace mz {

// (the values of the five games are stored in GoDevView::kind; kNoDeviceGame is what an engine without a device twin reports: the Atari-shaped environment)
// Values past the table are RULES VARIANTS of a row: a game that is its row's game in everything the table says — planes, pass slot in the policy, network shape,
// record loader — and differs in its rules alone, so it has a host class and a leaf body of its own but no row.  kNoGo: NoGo, a variant of Go (ref nogo.h:18
// NoGoEnv derives from GoEnv); its boards end at 9x9.
enum GameKind : int { kGo = 0, kOthello = 1, kTicTacToe = 2, kGomoku = 3, kHex = 4, kNoGo = 5, kNoDeviceGame = -1 };
constexpr int kNumGameKinds = 5;

// env_game name, feature planes, has a pass action, smallest / default / largest board with a device twin
struct GameRow { const char* name; int channels; bool has_pass; int min_board, default_board, max_board; };
constexpr GameRow kGameTable[kNumGameKinds] = {
    {"go", 18, true, 2, 9, 19},
    {"othello", 4, true, 4, 8, 8},
    {"tictactoe", 4, false, 3, 3, 3},
    {"gomoku", 4, false, 2, 15, 19},
    {"hex", 4, false, 2, 11, 19},
};

constexpr int kNoGoMaxBoard = 9; // ref nogo.h:12,22
constexpr bool isGameVariant(int k) { return k == kNoGo; }
constexpr bool isDeviceGame(int k) { return (k >= 0 && k < kNumGameKinds) || isGameVariant(k); }
constexpr GameKind gameRow(GameKind k) { return k == kNoGo ? kGo : k; } // the row a kind reads its facts from
constexpr bool gameHasPass(GameKind k) { return kGameTable[gameRow(k)].has_pass; } // (NoGo: the slot is in the policy, and never legal)
constexpr int gameChannels(GameKind k) { return kGameTable[gameRow(k)].channels; }
constexpr int gameMinBoard(GameKind k) { return kGameTable[gameRow(k)].min_board; }
constexpr int gameDefaultBoard(GameKind k) { return kGameTable[gameRow(k)].default_board; }
constexpr int gameMaxBoard(GameKind k) { return k == kNoGo ? kNoGoMaxBoard : kGameTable[k].max_board; }
constexpr const char* gameName(GameKind k) { return k == kNoGo ? "nogo" : kGameTable[k].name; }

// the game of an env_game string; kNoDeviceGame: neither of the table nor a variant ("atari", or unknown)
inline GameKind gameFromName(const char* env_game)
{
    {
        const char* a = "nogo";
        const char* b = env_game;
        while (*a && *a == *b) { ++a; ++b; }
        if (*a == 0 && *b == 0) { return kNoGo; }
    }
    for (int k = 0; k < kNumGameKinds; ++k) {
        const char* a = kGameTable[k].name;
        const char* b = env_game;
        while (*a && *a == *b) { ++a; ++b; }
        if (*a == 0 && *b == 0) { return static_cast<GameKind>(k); }
    }
    return kNoDeviceGame;
}

// The rules argument of the kernels (their template parameter `int CPL`): for Go the 64-bit words per plane of the board, positive; for the other games a
// sentinel that selects the leaf body (go_body.h leafBody).  The values are part of the kernels' mangled names.
constexpr int kRulesOthello = 0, kRulesTicTacToe = -1, kRulesGomoku = -2, kRulesHex = -3, kRulesNoGo = -4;
constexpr int rulesArg(int kind, int board_n)
{
    return kind == kNoGo ? kRulesNoGo : kind == kHex ? kRulesHex : kind == kGomoku ? kRulesGomoku : kind == kTicTacToe ? kRulesTicTacToe : kind == kOthello ? kRulesOthello : (board_n * board_n + 63) / 64;
}

} // namespace mz
