// The board games with a device twin, described once: the value stored in GoDevView::kind, and every fact about a game that code outside its own
// rules (env.cpp: the host class; go_body.h: the leaf body) needs.  Plain header of constexpr facts: host code (g++) and device code (hipcc) both include it.
// Adding a game: INTEGRATION.md "Adding a board game".
#pragma once

namespace mz {

// (the values of the five games are stored in GoDevView::kind; kNoDeviceGame is what an engine without a device twin reports: the Atari-shaped environment)
// Values past the table are the games of kExtraGames below, of two sorts.  A RULES VARIANT of a row is its row's game in everything the table says — planes,
// pass slot in the policy, network shape, record loader — and differs in its rules alone: a host class and a leaf body of its own, facts read from its row
// (kNoGo: NoGo, a variant of Go, ref nogo.h:18 NoGoEnv derives from GoEnv; its boards end at 9x9).  A game PAST THE ROWS WITH FACTS OF ITS OWN has a row of
// facts in kExtraGames instead (kHavannah: ref havannah.h — 20 planes, no pass, and a network board that is not env_board_size: networkBoard below).
enum GameKind : int { kGo = 0, kOthello = 1, kTicTacToe = 2, kGomoku = 3, kHex = 4, kNoGo = 5, kHavannah = 6, kNoDeviceGame = -1 };
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

// The games past the table, kind kNumGameKinds + i: their facts (boards as env_board_size counts them), the row a variant reads channels / pass / smallest and
// default board from (kNoDeviceGame: none, the facts here are the game's own), and the rules argument of the kernels (below).  A further such game is one line.
constexpr int kNoGoMaxBoard = 9;     // ref nogo.h:12,22
constexpr int kHavannahMaxBoard = 10; // edge size: the array is 19 x 19, what kGoMaxW words hold (go_dev.h)
constexpr int kRulesOthello = 0, kRulesTicTacToe = -1, kRulesGomoku = -2, kRulesHex = -3, kRulesNoGo = -4, kRulesHavannah = -5;
struct ExtraGame { GameRow facts; GameKind row; int rules; bool hex_array; }; // hex_array: a hexagon of edge size n kept in a (2n - 1) x (2n - 1) array (networkBoard)
constexpr int kNumExtraGames = 2;
constexpr ExtraGame kExtraGames[kNumExtraGames] = {
    {{"nogo", 18, true, 2, 9, kNoGoMaxBoard}, kGo, kRulesNoGo, false},
    {{"havannah", 20, false, 4, 8, kHavannahMaxBoard}, kNoDeviceGame, kRulesHavannah, true}, // ref havannah.h: assert(board_size >= 4); default 8
};

constexpr bool isExtraGame(int k) { return k >= kNumGameKinds && k < kNumGameKinds + kNumExtraGames; }
constexpr bool isGameVariant(int k) { return isExtraGame(k) && kExtraGames[k - kNumGameKinds].row != kNoDeviceGame; }
constexpr bool isDeviceGame(int k) { return (k >= 0 && k < kNumGameKinds) || isExtraGame(k); }
constexpr GameKind gameRow(GameKind k) { return isGameVariant(k) ? kExtraGames[k - kNumGameKinds].row : k; } // the row a kind reads its facts from (itself unless a variant)
// the facts of a kind: a row of the table, the row of a variant (with the variant's own name and largest board: the two accessors below), or the game's own
constexpr const GameRow& gameFacts(GameKind k) { return isExtraGame(k) && !isGameVariant(k) ? kExtraGames[k - kNumGameKinds].facts : kGameTable[gameRow(k)]; }
constexpr bool gameHasPass(GameKind k) { return gameFacts(k).has_pass; } // (NoGo: the slot is in the policy, and never legal)
constexpr int gameChannels(GameKind k) { return gameFacts(k).channels; }
constexpr int gameMinBoard(GameKind k) { return gameFacts(k).min_board; }
constexpr int gameDefaultBoard(GameKind k) { return gameFacts(k).default_board; }
constexpr int gameMaxBoard(GameKind k) { return isExtraGame(k) ? kExtraGames[k - kNumGameKinds].facts.max_board : kGameTable[k].max_board; }
constexpr const char* gameName(GameKind k) { return isExtraGame(k) ? kExtraGames[k - kNumGameKinds].facts.name : kGameTable[k].name; }
// The NETWORK BOARD of a game at env_board_size n: the side of the square array the planes, the policy, the bitboards and the kernels' H and W are made of.
// Havannah's edge size N plays on a (2N - 1) x (2N - 1) array with two corners cut off (ref havannah.h: extended_board_size_); everywhere else it is n.
constexpr int networkBoard(GameKind k, int n) { return isExtraGame(k) && kExtraGames[k - kNumGameKinds].hex_array ? 2 * n - 1 : n; }

// the game of an env_game string; kNoDeviceGame: neither of the table nor past it ("atari", or unknown)
inline GameKind gameFromName(const char* env_game)
{
    for (int k = 0; k < kNumGameKinds + kNumExtraGames; ++k) {
        const char* a = gameName(static_cast<GameKind>(k));
        const char* b = env_game;
        while (*a && *a == *b) { ++a; ++b; }
        if (*a == 0 && *b == 0) { return static_cast<GameKind>(k); }
    }
    return kNoDeviceGame;
}

// The rules argument of the kernels (their template parameter `int CPL`): for Go the 64-bit words per plane of the board, positive; for the other games a
// sentinel that selects the leaf body (go_body.h leafBody).  The values are part of the kernels' mangled names.
// (the sentinels are declared above, beside kExtraGames; board_n is the network board)
constexpr int rulesArg(int kind, int board_n)
{
    return isExtraGame(kind) ? kExtraGames[kind - kNumGameKinds].rules : kind == kHex ? kRulesHex : kind == kGomoku ? kRulesGomoku : kind == kTicTacToe ? kRulesTicTacToe : kind == kOthello ? kRulesOthello : (board_n * board_n + 63) / 64;
}

} // namespace mz
