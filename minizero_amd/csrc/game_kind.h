// The board games with a device twin, described once: the value stored in GoDevView::kind, and every fact about a game that code outside its own
// rules (env.cpp: the host class; go_body.h: the leaf body) needs.  Plain header of constexpr facts: host code (g++) and device code (hipcc) both include it.
// Adding a game: INTEGRATION.md "Adding a board game".
#pragma once

namespace mz {

// (the values of the five games are stored in GoDevView::kind; kNoDeviceGame is what an engine without a device twin reports: the Atari-shaped environment)
enum GameKind : int { kGo = 0, kOthello = 1, kTicTacToe = 2, kGomoku = 3, kHex = 4, kNoDeviceGame = -1 };
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

constexpr bool isDeviceGame(int k) { return k >= 0 && k < kNumGameKinds; }
constexpr bool gameHasPass(GameKind k) { return kGameTable[k].has_pass; }
constexpr int gameChannels(GameKind k) { return kGameTable[k].channels; }
constexpr int gameMinBoard(GameKind k) { return kGameTable[k].min_board; }
constexpr int gameDefaultBoard(GameKind k) { return kGameTable[k].default_board; }
constexpr int gameMaxBoard(GameKind k) { return kGameTable[k].max_board; }
constexpr const char* gameName(GameKind k) { return kGameTable[k].name; }

// the game of an env_game string; kNoDeviceGame: none of the table ("atari", or unknown)
inline GameKind gameFromName(const char* env_game)
{
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
constexpr int kRulesOthello = 0, kRulesTicTacToe = -1, kRulesGomoku = -2, kRulesHex = -3;
constexpr int rulesArg(int kind, int board_n)
{
    return kind == kHex ? kRulesHex : kind == kGomoku ? kRulesGomoku : kind == kTicTacToe ? kRulesTicTacToe : kind == kOthello ? kRulesOthello : (board_n * board_n + 63) / 64;
}

} // namespace mz
