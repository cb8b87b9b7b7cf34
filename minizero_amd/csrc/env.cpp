// Host rules engines of libmzgpu — see env.h.  Not a translation of the reference's data structures:
//   Havannah: two feature bitboards as the reference keeps them + a ring of the last eight, the group of the new stone by a flood, the ring test by a flood of the complement.
//   NoGo    : Go's board and planes, rules of its own (no capture, no suicide, no pass): flat byte board + early-exit flood fills.
//   Go      : flat byte board + on-demand early-exit flood fills for captures (no incremental blocks /
//             liberty bitsets / areas / Benson), one whole-board group pass only when a legal mask is
//             needed, positional-superko set as a small open-addressing table that is copied with the env,
//             8-deep ring of stone bitboards for the history planes.
//   Othello : two 64-bit bitboards, shift-and-mask move generation (8x8 and smaller).
//   TicTacToe: two 9-bit masks.
//   Gomoku  : two bitboards of up to 6 words, the winner from the four lines through the last stone.
//   Hex     : two bitboards of up to 6 words, the winner from an early-exit flood of the mover's group through the last stone.
// All feature planes are written straight into caller memory (the worker's pinned staging buffer).
#include "env.h"
#include "go_dev.h"
#include "common.h"
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>

namespace mz {

// ---------------------------------------------------------------------------------------------
// rotation tables (ref utils/rotation.h:21-29,51-93: float centre arithmetic with truncation)
// ---------------------------------------------------------------------------------------------
static int rotatePos(int rotation, int pos, int n)
{
    if (pos == n * n) { return pos; }
    const float center = (n - 1) / 2.0;
    const float x = pos % n - center, y = pos / n - center;
    float rx = x, ry = y;
    switch (rotation) {
        case 0: rx = x; ry = y; break;
        case 1: rx = y; ry = -x; break;
        case 2: rx = -x; ry = -y; break;
        case 3: rx = -y; ry = x; break;
        case 4: rx = x; ry = -y; break;
        case 5: rx = -y; ry = -x; break;
        case 6: rx = -x; ry = y; break;
        case 7: rx = y; ry = x; break;
    }
    return static_cast<int>((ry + center) * n + (rx + center));
}

void RotationTables::build(int n, int num_actions)
{
    static const int reversed[8] = {0, 3, 2, 1, 4, 5, 6, 7};
    board_size = n;
    for (int r = 0; r < 8; ++r) {
        fwd[r].resize(num_actions);
        inv[r].resize(n * n);
        for (int a = 0; a < num_actions; ++a) { fwd[r][a] = (a >= n * n) ? a : rotatePos(r, a, n); }
        for (int p = 0; p < n * n; ++p) { inv[r][p] = rotatePos(reversed[r], p, n); }
    }
}

// a game without symmetries (Hex: ref hex.h:61-62,78-79 getRotatePosition / getRotateAction return their argument): all eight maps are the identity
void RotationTables::buildIdentity(int n, int num_actions)
{
    board_size = n;
    for (int r = 0; r < 8; ++r) {
        fwd[r].resize(num_actions);
        inv[r].resize(n * n);
        for (int a = 0; a < num_actions; ++a) { fwd[r][a] = a; }
        for (int p = 0; p < n * n; ++p) { inv[r][p] = p; }
    }
}

static const RotationTables* rotationTables(int n, int num_actions, bool identity = false)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::unique_ptr<RotationTables>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto& slot = cache[{identity ? -n : n, num_actions}];
    if (!slot) {
        slot = std::make_unique<RotationTables>();
        if (identity) { slot->buildIdentity(n, num_actions); } else { slot->build(n, num_actions); }
    }
    return slot.get();
}

void GameEnv::featureBits(int rotation, uint32_t* out) const
{
    const int P = boardSize() * boardSize(), W32 = (P + 31) / 32, C = numInputChannels();
    std::vector<float> f(size_t(C) * P);
    features(rotation, f.data());
    for (int c = 0; c < C; ++c) {
        for (int w = 0; w < W32; ++w) { out[c * W32 + w] = 0; }
        for (int p = 0; p < P; ++p) { if (f[size_t(c) * P + p] != 0.0f) { out[c * W32 + (p >> 5)] |= 1u << (p & 31); } }
    }
}

static inline float scoreOf(int winner) { return winner == 1 ? 1.0f : (winner == 2 ? -1.0f : 0.0f); }

// ---------------------------------------------------------------------------------------------
// TicTacToe (ref tictactoe.cpp:11-146)
// ---------------------------------------------------------------------------------------------
// ref utils/sgf_loader.cpp:89-99 boardCoordinateStringToActionID (the conversion behind BaseBoardAction(action_string_args), base_env.h:326-333)
int GameEnv::actionFromString(const std::string& str) const
{
    const int n = boardSize();
    std::string up = str;
    for (char& c : up) { c = static_cast<char>(std::toupper(static_cast<unsigned char>(c))); }
    if (up == "PASS") { return n * n; }
    if (str.size() < 2) { return -1; }
    const int x = up[0] - 'A' + (up[0] > 'I' ? -1 : 0);
    const int y = atoi(str.substr(1).c_str()) - 1;
    return y * n + x;
}

// What the four games with the planes (own, opponent, black to move, white to move) share: the action history, act() over isLegal() + actUnchecked(), the
// planes and the legal mask, the head of the device snapshot, the facts of the game's row in game_kind.h.  A game supplies word(colour, w) — word w of its
// bitboard of that colour — isLegal() and actUnchecked(), which ends with played().  (CRTP: word() is inlined into the plane loops.)
template <class Game, GameKind K>
class FourPlaneEnv : public GameEnv {
public:
    std::unique_ptr<GameEnv> clone() const override { return std::make_unique<Game>(self()); }
    void copyFrom(const GameEnv& o) override { static_cast<Game&>(*this) = static_cast<const Game&>(o); }
    bool stone(int c, int p) const { return (self().word(c, p >> 6) >> (p & 63)) & 1; }
    bool act(int a, int player) override
    {
        if (!self().isLegal(a, player)) { return false; }
        self().actUnchecked(a, player);
        return true;
    }
    void legalMask(uint8_t* out) const override { for (int a = 0; a < policySize(); ++a) { out[a] = self().isLegal(a, turn_); } }
    void features(int r, float* out) const override
    {
        const int* map = rot_->inv[r].data();
        for (int p = 0; p < P_; ++p) {
            out[p] = stone(turn_ - 1, map[p]) ? 1.0f : 0.0f;
            out[P_ + p] = stone(2 - turn_, map[p]) ? 1.0f : 0.0f;
            out[2 * P_ + p] = turn_ == 1 ? 1.0f : 0.0f;
            out[3 * P_ + p] = turn_ == 2 ? 1.0f : 0.0f;
        }
    }
    void featureBits(int r, uint32_t* out) const override
    {
        const int W32 = (P_ + 31) / 32;
        const int* map = rot_->inv[r].data();
        for (int i = 0; i < 4 * W32; ++i) { out[i] = 0; }
        for (int p = 0; p < P_; ++p) {
            const uint32_t b = 1u << (p & 31);
            if (stone(turn_ - 1, map[p])) { out[p >> 5] |= b; }
            if (stone(2 - turn_, map[p])) { out[W32 + (p >> 5)] |= b; }
            out[(turn_ == 1 ? 2 : 3) * W32 + (p >> 5)] |= b;
        }
    }
    int actionFromString(const std::string& str) const override
    {
        if (gameHasPass(K)) { return GameEnv::actionFromString(str); }
        std::string up = str;
        for (char& c : up) { c = static_cast<char>(std::toupper(static_cast<unsigned char>(c))); }
        return up == "PASS" ? -1 : GameEnv::actionFromString(str); // no pass action
    }
    GameKind deviceKind() const override { return n_ >= gameMinBoard(K) && n_ <= gameMaxBoard(K) ? K : kNoDeviceGame; }
    int numInputChannels() const override { return gameChannels(K); }
    int boardSize() const override { return n_; }
    int policySize() const override { return P_ + (gameHasPass(K) ? 1 : 0); }
    std::vector<std::pair<std::string, std::string>> loaderTags() const override { return {{"SZ", std::to_string(n_)}}; }

protected:
    explicit FourPlaneEnv(int n, bool no_symmetries = false) : n_(n), P_(n * n) { rot_ = rotationTables(n, policySize(), no_symmetries); }
    const Game& self() const { return static_cast<const Game&>(*this); }
    Game& self() { return static_cast<Game&>(*this); }
    void resetHistory() { turn_ = 1; action_ids_.clear(); action_players_.clear(); }
    void played(int a, int player)
    {
        action_ids_.push_back(static_cast<int16_t>(a));
        action_players_.push_back(static_cast<uint8_t>(player));
        turn_ = 3 - player;
    }
    // the fields of GoRootSnapshot every one of the four device engines reads (go_body.h): the two bitboards, the player to move, the actions played;
    // the game fills in what else its engine reads
    GoRootSnapshot& exportHead(void* dst) const
    {
        GoRootSnapshot& s = *static_cast<GoRootSnapshot*>(dst);
        for (int w = 0; w < kGoMaxW; ++w) {
            s.stones[0][w] = self().word(0, w);
            s.stones[1][w] = self().word(1, w);
        }
        s.hash = 0;
        s.hist_len = 0;
        s.turn = turn_;
        s.nmoves = static_cast<int32_t>(action_ids_.size());
        s.passes = 0;
        return s;
    }
    int n_, P_;
};

class TicTacToe final : public FourPlaneEnv<TicTacToe, kTicTacToe> {
public:
    TicTacToe() : FourPlaneEnv(3) { reset(); }
    void reset() override { resetHistory(); m_[0] = m_[1] = 0; }
    uint64_t word(int c, int w) const { return w == 0 ? m_[c] : 0; }
    bool isLegal(int a, int) const override { return a >= 0 && a < 9 && !((m_[0] | m_[1]) >> a & 1); }
    void actUnchecked(int a, int player) override
    {
        m_[player - 1] |= 1u << a;
        played(a, player);
    }
    int winner() const
    {
        static const unsigned lines[8] = {0007, 0070, 0700, 0111, 0222, 0444, 0421, 0124};
        for (unsigned l : lines) {
            if ((m_[0] & l) == l) { return 1; }
            if ((m_[1] & l) == l) { return 2; }
        }
        return 0;
    }
    bool isTerminal() const override { return winner() != 0 || (m_[0] | m_[1]) == 0777; }
    float evalScore(bool is_resign) const override { return scoreOf(is_resign ? 3 - turn_ : winner()); }
    int actionFromString(const std::string& str) const override { return GameEnv::actionFromString(str); } // ("pass" is 9, one past the board, as in ref tictactoe.h)
    void exportDeviceRoot(void* dst) const override { exportHead(dst); } // (go_body.h tttLeafBody)
    std::string name() const override { return "tictactoe"; }

private:
    unsigned m_[2];
};

// ---------------------------------------------------------------------------------------------
// Othello, board <= 8x8 (ref othello.cpp:14-262)
// ---------------------------------------------------------------------------------------------
class Othello final : public FourPlaneEnv<Othello, kOthello> {
public:
    explicit Othello(int n) : FourPlaneEnv(n)
    {
        full_ = 0; not_left_ = 0; not_right_ = 0;
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                uint64_t b = 1ull << (y * n + x);
                full_ |= b;
                if (x != 0) { not_left_ |= b; }
                if (x != n - 1) { not_right_ |= b; }
            }
        reset();
    }
    uint64_t word(int c, int w) const { return w == 0 ? s_[c] : 0; }
    void reset() override // ref othello.cpp:14-27 (black on init, init+n+1; white on init+1, init+n)
    {
        resetHistory();
        const int init = n_ * (n_ / 2 - (1 - n_ % 2)) + (n_ / 2 - 1);
        s_[0] = (1ull << init) | (1ull << (init + n_ + 1));
        s_[1] = (1ull << (init + 1)) | (1ull << (init + n_));
    }
    // one step in direction d for every stone; stones that would leave the board vanish
    uint64_t shift(uint64_t b, int d) const
    {
        switch (d) {
            case 0: return (b << n_) & full_;                 // up
            case 1: return b >> n_;                           // down
            case 2: return (b & not_left_) >> 1;              // left
            case 3: return ((b & not_right_) << 1) & full_;   // right
            case 4: return ((b & not_left_) << (n_ - 1)) & full_;
            case 5: return ((b & not_right_) << (n_ + 1)) & full_;
            case 6: return (b & not_right_) >> (n_ - 1);
            default: return (b & not_left_) >> (n_ + 1);
        }
    }
    uint64_t moves(int player) const
    {
        const uint64_t me = s_[player - 1], op = s_[2 - player], empty = full_ & ~(me | op);
        uint64_t m = 0;
        for (int d = 0; d < 8; ++d) {
            uint64_t x = shift(me, d) & op;
            for (int i = 0; i < n_ - 3; ++i) { x |= shift(x, d) & op; }
            m |= shift(x, d) & empty;
        }
        return m;
    }
    bool isLegal(int a, int player) const override
    {
        const uint64_t m = moves(player);
        if (a == n_ * n_) { return m == 0; } // pass only when the mover has no move (ref othello.cpp:195-201)
        return a >= 0 && a < n_ * n_ && ((m >> a) & 1);
    }
    void actUnchecked(int a, int player) override
    {
        played(a, player);
        if (a == n_ * n_) { return; }
        uint64_t& me = s_[player - 1];
        uint64_t& op = s_[2 - player];
        const uint64_t placed = 1ull << a;
        uint64_t flip = 0;
        for (int d = 0; d < 8; ++d) {
            uint64_t line = 0, x = shift(placed, d);
            while (x & op) { line |= x; x = shift(x, d); }
            if (x & me) { flip |= line; }
        }
        me |= placed | flip;
        op &= ~flip;
    }
    void legalMask(uint8_t* out) const override // (one move generation for all actions, not one per isLegal())
    {
        const uint64_t m = moves(turn_);
        for (int a = 0; a < n_ * n_; ++a) { out[a] = (m >> a) & 1; }
        out[n_ * n_] = (m == 0);
    }
    bool isTerminal() const override
    {
        const size_t k = action_ids_.size();
        return k >= 2 && action_ids_[k - 1] == n_ * n_ && action_ids_[k - 2] == n_ * n_;
    }
    float evalScore(bool is_resign) const override // ref othello.cpp:211-236: winner only once neither side can move
    {
        if (is_resign) { return scoreOf(3 - turn_); }
        if (moves(1) != 0 || moves(2) != 0) { return 0.0f; }
        const int b = __builtin_popcountll(s_[0]), w = __builtin_popcountll(s_[1]);
        return scoreOf(b > w ? 1 : (b < w ? 2 : 0));
    }
    void exportDeviceRoot(void* dst) const override // (go_body.h othLeafBody)
    {
        GoRootSnapshot& s = exportHead(dst);
        int passes = 0;
        for (size_t k = action_ids_.size(); k > 0 && passes < 2 && action_ids_[k - 1] == n_ * n_; --k) { ++passes; }
        s.passes = passes;
    }
    std::string name() const override { return "othello_" + std::to_string(n_) + "x" + std::to_string(n_); }

private:
    uint64_t full_, not_left_, not_right_, s_[2];
};

// ---------------------------------------------------------------------------------------------
// Gomoku, board <= 19x19 (ref gomoku.cpp:14-185): two bitboards of up to 6 words.  The winner is decided by the move just played alone,
// along each of the four lines through its stone (gomoku.cpp:140-162); a win on the move that fills the board is a win.  Outer-open
// restricts the game's first move (no move played yet) to the outer two rings.  No pass action: policySize() == P.
// ---------------------------------------------------------------------------------------------
class Gomoku final : public FourPlaneEnv<Gomoku, kGomoku> {
    static constexpr int kW = (19 * 19 + 63) / 64;
public:
    Gomoku(int n, bool outer_open, bool exactly_five) : FourPlaneEnv(n), outer_open_(outer_open), exactly_five_(exactly_five) { reset(); }
    void reset() override
    {
        resetHistory();
        memset(s_, 0, sizeof(s_));
        winner_ = 0;
    }
    uint64_t word(int c, int w) const { return w < kW ? s_[c][w] : 0; }
    bool isLegal(int a, int) const override // ref gomoku.cpp:48-58: the first move under outer-open is any point of the outer two rings
    {
        if (a < 0 || a >= P_) { return false; }
        if (outer_open_ && action_ids_.empty()) {
            const int i = a / n_, j = a % n_;
            return i < 2 || i >= n_ - 2 || j < 2 || j >= n_ - 2;
        }
        return !stone(0, a) && !stone(1, a);
    }
    void actUnchecked(int a, int player) override
    {
        s_[player - 1][a >> 6] |= 1ull << (a & 63);
        played(a, player);
        winner_ = wins(a, player - 1) ? player : 0; // ref gomoku.cpp:29: replaced on every move
    }
    // the stones of colour c on the line through p in direction (dx, dy), p included (ref gomoku.cpp:140-162)
    int lineLength(int p, int c, int dx, int dy) const
    {
        int len = 1;
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            int x = p % n_ + sgn * dx, y = p / n_ + sgn * dy;
            while (x >= 0 && x < n_ && y >= 0 && y < n_ && stone(c, y * n_ + x)) { ++len; x += sgn * dx; y += sgn * dy; }
        }
        return len;
    }
    bool wins(int p, int c) const
    {
        static const int dirs[4][2] = {{1, 0}, {0, 1}, {1, 1}, {1, -1}};
        for (const auto& d : dirs) {
            const int len = lineLength(p, c, d[0], d[1]);
            if (exactly_five_ ? len == 5 : len >= 5) { return true; }
        }
        return false;
    }
    int stonesPlayed() const
    {
        int k = 0;
        for (int w = 0; w < kW; ++w) { k += __builtin_popcountll(s_[0][w] | s_[1][w]); }
        return k;
    }
    bool isTerminal() const override { return winner_ != 0 || stonesPlayed() == P_; }
    float evalScore(bool is_resign) const override { return scoreOf(is_resign ? 3 - turn_ : winner_); } // ref gomoku.cpp:65-73
    void exportDeviceRoot(void* dst) const override // (go_body.h gmkLeafBody)
    {
        GoRootSnapshot& s = exportHead(dst);
        s.ruleBits() = (outer_open_ ? kGmkOuterOpen : 0) | (exactly_five_ ? kGmkExactlyFive : 0);
        s.winner() = winner_;
    }
    std::string name() const override { return "gomoku" + std::string(outer_open_ ? "_oo_" : "_") + std::to_string(n_) + "x" + std::to_string(n_); }

private:
    bool outer_open_, exactly_five_;
    int winner_;
    uint64_t s_[2][kW];
};

// ---------------------------------------------------------------------------------------------
// Hex, board <= 19x19 (ref hex.cpp:13-141,307-362): two bitboards of up to 6 words.  Black (player 1) connects column 0 with column n - 1, White row 0
// with row n - 1 (hex.cpp:51-61); the neighbours of (x, y) are (x-1,y-1) (x,y-1) (x-1,y) (x+1,y) (x,y+1) (x+1,y+1) (hex.cpp:319-336).  The reference
// propagates two edge flags per cell; here the winner is the mover when the mover's group through the new stone touches both of the mover's edges (the same
// answer), found by a flood from that stone that stops as soon as both edges are reached.  Terminal <=> a winner exists.  With the swap rule
// (env_hex_use_swap_rule, hex.cpp:28-47,86-99) every cell is legal on the second action, and choosing the occupied one replaces Black's stone by a White
// stone on its reflection; the record keeps the chosen action id.  No pass action, no symmetries: the rotation tables are the identity.
// ---------------------------------------------------------------------------------------------
class Hex final : public FourPlaneEnv<Hex, kHex> {
    static constexpr int kW = (19 * 19 + 63) / 64;
public:
    Hex(int n, bool swap) : FourPlaneEnv(n, true), swap_(swap) { reset(); }
    void reset() override
    {
        resetHistory();
        memset(s_, 0, sizeof(s_));
        winner_ = 0;
        nact_ = 0;
        first_ = -1;
    }
    uint64_t word(int c, int w) const { return w < kW ? s_[c][w] : 0; }
    bool isLegal(int a, int) const override // ref hex.cpp:86-99: an empty cell, or any cell on the second action under the swap rule
    {
        if (a < 0 || a >= P_) { return false; }
        return (swap_ && nact_ == 1) || (!stone(0, a) && !stone(1, a));
    }
    void actUnchecked(int a, int player) override
    {
        int p = a;
        if (swap_ && nact_ == 1 && a == first_) { // ref hex.cpp:28-47: the first stone goes, the mover's stone lands on its reflection
            s_[0][a >> 6] &= ~(1ull << (a & 63));
            s_[1][a >> 6] &= ~(1ull << (a & 63));
            p = (n_ - 1 - a % n_) * n_ + (n_ - 1 - a / n_);
        }
        s_[player - 1][p >> 6] |= 1ull << (p & 63);
        if (nact_ == 0) { first_ = a; }
        ++nact_;
        played(a, player); // the chosen id, also for a swap (B[k];W[k])
        if (winner_ == 0 && connects(p, player - 1)) { winner_ = player; } // a winner never goes away
    }
    // does the group of colour c through p touch both of c's edges?  (a stack flood over the six neighbours, ended by the second edge)
    bool connects(int p, int c) const
    {
        uint64_t seen[kW] = {};
        int16_t stack[19 * 19];
        int top = 0;
        bool lo = false, hi = false;
        stack[top++] = static_cast<int16_t>(p);
        seen[p >> 6] |= 1ull << (p & 63);
        static const int dx[6] = {-1, 0, -1, 1, 0, 1}, dy[6] = {-1, -1, 0, 0, 1, 1};
        while (top) {
            const int q = stack[--top], x = q % n_, y = q / n_;
            const int along = c == 0 ? x : y; // Black: columns, White: rows
            lo |= along == 0;
            hi |= along == n_ - 1;
            if (lo && hi) { return true; }
            for (int k = 0; k < 6; ++k) {
                const int u = x + dx[k], v = y + dy[k];
                if (u < 0 || u >= n_ || v < 0 || v >= n_) { continue; }
                const int r = v * n_ + u;
                if (!stone(c, r) || ((seen[r >> 6] >> (r & 63)) & 1)) { continue; }
                seen[r >> 6] |= 1ull << (r & 63);
                stack[top++] = static_cast<int16_t>(r);
            }
        }
        return false;
    }
    bool isTerminal() const override { return winner_ != 0; } // ref hex.cpp:101-104
    float evalScore(bool is_resign) const override { return scoreOf(is_resign ? 3 - turn_ : winner_); } // ref hex.cpp:106-116
    // (the planes, ref hex.cpp:118-141, ignore the rotation: the tables are the identity)
    int actionFromString(const std::string& str) const override // board coordinates ("F6") on the board only
    {
        const int a = FourPlaneEnv::actionFromString(str);
        return a >= 0 && a < P_ ? a : -1;
    }
    void exportDeviceRoot(void* dst) const override // (go_body.h hexLeafBody); nmoves = the actions played, a swap is one
    {
        GoRootSnapshot& s = exportHead(dst);
        s.ruleBits() = swap_ ? kHexSwap : 0;
        s.winner() = winner_;
    }
    std::string name() const override { return "hex_" + std::to_string(n_) + "x" + std::to_string(n_); } // ref hex.h:56

private:
    bool swap_;
    int winner_, nact_, first_; // actions played (a swap is one), the first action (what a swap must repeat)
    uint64_t s_[2][kW];
};

// ---------------------------------------------------------------------------------------------
// Go (ref go.cpp:102-315,690-723)
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int kMaxN = 19, kMaxP = kMaxN * kMaxN, kWords = (kMaxP + 63) / 64;
struct Bits {
    uint64_t w[kWords];
    void clear() { memset(w, 0, sizeof(w)); }
    void set(int i) { w[i >> 6] |= 1ull << (i & 63); }
    void reset(int i) { w[i >> 6] &= ~(1ull << (i & 63)); }
    bool test(int i) const { return (w[i >> 6] >> (i & 63)) & 1; }
};
struct GoStatic {
    int n = 0;
    int16_t nbr[kMaxP][4];
    uint8_t nnbr[kMaxP];
    uint64_t key[2][kMaxP];
};
const GoStatic* goStatic(int n)
{
    static std::mutex mu;
    static std::map<int, std::unique_ptr<GoStatic>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto& slot = cache[n];
    if (!slot) {
        slot = std::make_unique<GoStatic>();
        slot->n = n;
        // the superko test only needs "equal positions <=> equal keys": any good 64-bit Zobrist keys do
        // (the reference draws its keys from mt19937_64(0), go.cpp:19-43; the values themselves are unobservable)
        std::mt19937_64 gen(0x6d7a677075ULL);
        for (int p = 0; p < n * n; ++p) {
            slot->key[0][p] = gen();
            slot->key[1][p] = gen();
            int x = p % n, y = p / n, k = 0;
            if (y + 1 < n) { slot->nbr[p][k++] = static_cast<int16_t>(p + n); }
            if (x + 1 < n) { slot->nbr[p][k++] = static_cast<int16_t>(p + 1); }
            if (y - 1 >= 0) { slot->nbr[p][k++] = static_cast<int16_t>(p - n); }
            if (x - 1 >= 0) { slot->nbr[p][k++] = static_cast<int16_t>(p - 1); }
            slot->nnbr[p] = static_cast<uint8_t>(k);
        }
    }
    return slot.get();
}
} // namespace

class Go final : public GameEnv {
    static constexpr int kHashCap = 1024; // > 2 * (2*361 + 1) positions of the longest legal game at 19x19
public:
    // situational: env_go_ko_rule=situational — a position repeats only with the same player to move: the hash of every position also
    // carries a turn key on odd move counts (ref go.cpp:45-49,141,222); positional (the default): key 0
    Go(int n, float komi, bool situational = false) : n_(n), P_(n * n), komi_(komi), st_(goStatic(n)), turn_key_(situational ? 0x9e3779b97f4a7c15ULL : 0)
    {
        rot_ = rotationTables(n, n * n + 1);
        reset();
    }
    std::unique_ptr<GameEnv> clone() const override { return std::make_unique<Go>(*this); }
    void copyFrom(const GameEnv& o) override { *this = static_cast<const Go&>(o); }
    void reset() override
    {
        turn_ = 1;
        action_ids_.clear();
        action_players_.clear();
        memset(board_, 0, sizeof(board_));
        hash_ = 0;
        memset(seen_, 0, sizeof(seen_));
        seen_used_ = 0;
        hist_len_ = 0;
        for (auto& h : hist_) { h[0].clear(); h[1].clear(); }
        stones_[0].clear();
        stones_[1].clear();
    }

    // ---- superko set: open addressing, 0 = empty slot (a zero hash is stored as 1) ----
    static uint64_t norm(uint64_t h) { return h ? h : 1; }
    bool seen(uint64_t h) const
    {
        h = norm(h);
        for (uint32_t i = static_cast<uint32_t>(h) & (kHashCap - 1);; i = (i + 1) & (kHashCap - 1)) {
            if (seen_[i] == 0) { return false; }
            if (seen_[i] == h) { return true; }
        }
    }
    void remember(uint64_t h)
    {
        h = norm(h);
        for (uint32_t i = static_cast<uint32_t>(h) & (kHashCap - 1);; i = (i + 1) & (kHashCap - 1)) {
            if (seen_[i] == h) { return; }
            if (seen_[i] == 0) { seen_[i] = h; ++seen_used_; return; }
        }
    }

    // flood fill the group at `start`; returns liberty count (stops at `cap` liberties), stones in grp[], XOR of keys in *gh
    int group(int start, int cap, int16_t* grp, int* gsize, uint64_t* gh) const
    {
        uint8_t mark[kMaxP];
        memset(mark, 0, P_);
        const uint8_t color = board_[start];
        int head = 0, tail = 0, libs = 0;
        uint64_t h = 0;
        grp[tail++] = static_cast<int16_t>(start);
        mark[start] = 1;
        while (head < tail) {
            const int p = grp[head++];
            h ^= st_->key[color - 1][p];
            for (int k = 0; k < st_->nnbr[p]; ++k) {
                const int q = st_->nbr[p][k];
                if (mark[q]) { continue; }
                if (board_[q] == 0) {
                    mark[q] = 1;
                    if (++libs >= cap) { *gsize = tail; if (gh) { *gh = 0; } return libs; } // early exit: enough liberties known
                } else if (board_[q] == color) {
                    mark[q] = 1;
                    grp[tail++] = static_cast<int16_t>(q);
                }
            }
        }
        *gsize = tail;
        if (gh) { *gh = h; }
        return libs;
    }

    bool isLegal(int a, int player) const override // ref go.cpp:208-244
    {
        if (a == P_) { return true; }
        if (a < 0 || a > P_ || board_[a] != 0) { return false; }
        bool ok = false;
        uint64_t nh = hash_ ^ turn_key_ ^ st_->key[player - 1][a];
        int16_t grp[kMaxP];
        int16_t seen_rep[4];
        int nrep = 0;
        for (int k = 0; k < st_->nnbr[a]; ++k) {
            const int q = st_->nbr[a][k];
            if (board_[q] == 0) { ok = true; continue; }
            int gs = 0;
            uint64_t gh = 0;
            if (board_[q] == player) {
                if (!ok && group(q, 2, grp, &gs, nullptr) > 1) { ok = true; }
            } else {
                // an enemy block in atari is captured: each block once
                bool dup = false;
                const int libs = group(q, 2, grp, &gs, &gh);
                if (libs == 1) {
                    int rep = grp[0];
                    for (int i = 1; i < gs; ++i) { rep = grp[i] < rep ? grp[i] : rep; }
                    for (int i = 0; i < nrep; ++i) { dup |= (seen_rep[i] == rep); }
                    if (!dup) { seen_rep[nrep++] = static_cast<int16_t>(rep); nh ^= gh; }
                    ok = true;
                }
            }
        }
        return ok && !seen(nh);
    }

    void legalMask(uint8_t* out) const override
    {
        // one whole-board pass: group id, liberty count (saturated at 2) and key-XOR per group
        int16_t gid[kMaxP];
        uint8_t glibs[kMaxP];
        uint64_t ghash[kMaxP];
        for (int p = 0; p < P_; ++p) { gid[p] = -1; }
        int16_t grp[kMaxP];
        for (int p = 0; p < P_; ++p) {
            if (board_[p] == 0 || gid[p] >= 0) { continue; }
            int gs = 0;
            uint64_t gh = 0;
            // full fill (cap = infinity would also do; liberties beyond 2 are never needed, but the hash is)
            const int libs = group(p, kMaxP, grp, &gs, &gh);
            for (int i = 0; i < gs; ++i) { gid[grp[i]] = static_cast<int16_t>(p); }
            glibs[p] = static_cast<uint8_t>(libs > 2 ? 2 : libs);
            ghash[p] = gh;
        }
        const int player = turn_;
        for (int a = 0; a < P_; ++a) {
            if (board_[a] != 0) { out[a] = 0; continue; }
            bool ok = false;
            uint64_t nh = hash_ ^ turn_key_ ^ st_->key[player - 1][a];
            int16_t cap[4];
            int ncap = 0;
            for (int k = 0; k < st_->nnbr[a]; ++k) {
                const int q = st_->nbr[a][k];
                if (board_[q] == 0) { ok = true; continue; }
                const int g = gid[q];
                if (board_[q] == player) {
                    if (glibs[g] > 1) { ok = true; }
                } else if (glibs[g] == 1) {
                    bool dup = false;
                    for (int i = 0; i < ncap; ++i) { dup |= (cap[i] == g); }
                    if (!dup) { cap[ncap++] = static_cast<int16_t>(g); nh ^= ghash[g]; }
                    ok = true;
                }
            }
            out[a] = ok && !seen(nh);
        }
        out[P_] = 1;
    }

    bool act(int a, int player) override
    {
        if (!isLegal(a, player)) { return false; }
        actUnchecked(a, player);
        return true;
    }
    void actUnchecked(int a, int player) override // ref go.cpp:132-190 (observable effects only)
    {
        action_ids_.push_back(static_cast<int16_t>(a));
        action_players_.push_back(static_cast<uint8_t>(player));
        turn_ = 3 - player;
        hash_ ^= turn_key_;
        if (a != P_) {
            board_[a] = static_cast<uint8_t>(player);
            stones_[player - 1].set(a);
            hash_ ^= st_->key[player - 1][a];
            int16_t grp[kMaxP];
            for (int k = 0; k < st_->nnbr[a]; ++k) {
                const int q = st_->nbr[a][k];
                if (board_[q] != 3 - player) { continue; }
                int gs = 0;
                if (group(q, 1, grp, &gs, nullptr) == 0) { // captured
                    for (int i = 0; i < gs; ++i) {
                        const int s = grp[i];
                        board_[s] = 0;
                        stones_[2 - player].reset(s);
                        hash_ ^= st_->key[2 - player][s];
                    }
                }
            }
        }
        hist_[hist_len_ & 7][0] = stones_[0];
        hist_[hist_len_ & 7][1] = stones_[1];
        ++hist_len_;
        remember(hash_);
    }
    bool isTerminal() const override // ref go.cpp:246-257
    {
        const size_t k = action_ids_.size();
        if (k >= 2 && action_ids_[k - 1] == P_ && action_ids_[k - 2] == P_) { return true; }
        return static_cast<int>(k) > 2 * P_;
    }
    float evalScore(bool is_resign) const override // Tromp-Taylor area + komi (ref go.cpp:259-278,703-723)
    {
        if (is_resign) { return scoreOf(3 - turn_); }
        float t1 = 0, t2 = 0;
        for (int p = 0; p < P_; ++p) { t1 += board_[p] == 1; t2 += board_[p] == 2; }
        t2 += komi_;
        uint8_t mark[kMaxP];
        memset(mark, 0, P_);
        int16_t q[kMaxP];
        for (int s = 0; s < P_; ++s) {
            if (board_[s] != 0 || mark[s]) { continue; }
            int head = 0, tail = 0, border = 0; // border: bit0 = touches black, bit1 = touches white
            q[tail++] = static_cast<int16_t>(s);
            mark[s] = 1;
            while (head < tail) {
                const int p = q[head++];
                for (int k = 0; k < st_->nnbr[p]; ++k) {
                    const int r = st_->nbr[p][k];
                    if (board_[r] == 0) { if (!mark[r]) { mark[r] = 1; q[tail++] = static_cast<int16_t>(r); } }
                    else { border |= board_[r]; }
                }
            }
            // a region bordered by black only — or by nothing at all (empty board) — counts for black (go.cpp:714),
            // else one bordered by white only counts for white
            if ((border & 2) == 0) { t1 += tail; }
            else if ((border & 1) == 0) { t2 += tail; }
        }
        return scoreOf(t1 > t2 ? 1 : (t1 < t2 ? 2 : 0));
    }
    void features(int r, float* out) const override // ref go.cpp:280-308
    {
        const int* map = rot_->inv[r].data();
        for (int k = 0; k < 8; ++k) {
            float* own = out + (2 * k) * P_;
            float* opp = own + P_;
            if (hist_len_ - 1 - k < 0) {
                memset(own, 0, 2 * P_ * sizeof(float));
                continue;
            }
            const Bits* h = hist_[(hist_len_ - 1 - k) & 7];
            const Bits& mine = h[turn_ - 1];
            const Bits& theirs = h[2 - turn_];
            for (int p = 0; p < P_; ++p) {
                own[p] = mine.test(map[p]) ? 1.0f : 0.0f;
                opp[p] = theirs.test(map[p]) ? 1.0f : 0.0f;
            }
        }
        const float b = turn_ == 1 ? 1.0f : 0.0f, w = turn_ == 2 ? 1.0f : 0.0f;
        for (int p = 0; p < P_; ++p) { out[16 * P_ + p] = b; out[17 * P_ + p] = w; }
    }
    void featureBits(int r, uint32_t* out) const override
    {
        const int W32 = (P_ + 31) / 32;
        const int* map = rot_->inv[r].data();
        memset(out, 0, size_t(18) * W32 * sizeof(uint32_t));
        for (int k = 0; k < 8; ++k) {
            if (hist_len_ - 1 - k < 0) { break; }
            const Bits* h = hist_[(hist_len_ - 1 - k) & 7];
            const Bits& mine = h[turn_ - 1];
            const Bits& theirs = h[2 - turn_];
            uint32_t* own = out + (2 * k) * W32;
            uint32_t* opp = own + W32;
            for (int p = 0; p < P_; ++p) {
                const int q = map[p];
                own[p >> 5] |= static_cast<uint32_t>(mine.test(q)) << (p & 31);
                opp[p >> 5] |= static_cast<uint32_t>(theirs.test(q)) << (p & 31);
            }
        }
        uint32_t* t = out + (turn_ == 1 ? 16 : 17) * W32;
        for (int p = 0; p < P_; ++p) { t[p >> 5] |= 1u << (p & 31); }
    }
    GameKind deviceKind() const override { return kGo; }
    uint64_t turnKey() const override { return turn_key_; }
    const uint64_t* zobristKeys() const override
    {
        // [2][P_] contiguous copy of the [2][kMaxP] table
        static std::mutex mu;
        static std::map<int, std::vector<uint64_t>> cache;
        std::lock_guard<std::mutex> lock(mu);
        auto& k = cache[n_];
        if (k.empty()) {
            k.resize(size_t(2) * P_);
            for (int c = 0; c < 2; ++c) { for (int p = 0; p < P_; ++p) { k[size_t(c) * P_ + p] = st_->key[c][p]; } }
        }
        return k.data();
    }
    void exportDeviceRoot(void* dst) const override
    {
        static_assert(kWords == kGoMaxW && kHashCap == kGoSeenCap && kMaxP == kGoMaxP, "device snapshot layout");
        GoRootSnapshot& s = *static_cast<GoRootSnapshot*>(dst);
        memcpy(s.stones, stones_, sizeof(s.stones));
        memcpy(s.hist, hist_, sizeof(s.hist));
        memcpy(s.seen, seen_, sizeof(s.seen));
        s.hash = hash_;
        s.hist_len = hist_len_;
        s.turn = turn_;
        s.nmoves = static_cast<int32_t>(action_ids_.size());
        int passes = 0;
        for (size_t k = action_ids_.size(); k > 0 && passes < 2 && action_ids_[k - 1] == P_; --k) { ++passes; }
        s.passes = passes;
        // group id per stone: the first point of the group in scan order
        int16_t grp[kMaxP];
        uint8_t done[kMaxP];
        memset(done, 0, P_);
        for (int p = 0; p < P_; ++p) {
            if (board_[p] == 0 || done[p]) { s.lab[p] = board_[p] == 0 ? 0 : s.lab[p]; continue; }
            int gs = 0;
            (void)group(p, kMaxP + 1, grp, &gs, nullptr);
            for (int i = 0; i < gs; ++i) { s.lab[grp[i]] = static_cast<uint16_t>(p); done[grp[i]] = 1; }
        }
    }
    int numInputChannels() const override { return 18; }
    int boardSize() const override { return n_; }
    int policySize() const override { return P_ + 1; }
    std::string name() const override { return "go_" + std::to_string(n_) + "x" + std::to_string(n_); }
    std::vector<std::pair<std::string, std::string>> loaderTags() const override
    {
        return {{"SZ", std::to_string(n_)}, {"KM", std::to_string(komi_)}};
    }

private:
    int n_, P_;
    float komi_;
    const GoStatic* st_;
    uint64_t turn_key_;
    uint8_t board_[kMaxP];
    uint64_t hash_;
    uint64_t seen_[kHashCap];
    int seen_used_;
    Bits stones_[2];
    Bits hist_[8][2];
    int hist_len_;
};

// ---------------------------------------------------------------------------------------------
// NoGo (ref nogo.h:18-86: NoGoEnv derives from GoEnv): Go's board, actions, planes and records with other rules — a move must neither capture
// nor be suicide, nothing is ever removed, there is no pass, and the player to move without a legal point has lost.  A rules variant of Go's row
// of game_kind.h (kNoGo).  Flat byte board + early-exit flood fills like Go; no hash, no superko set, no score.
// ---------------------------------------------------------------------------------------------
class NoGo final : public GameEnv {
public:
    NoGo(int n, float komi) : n_(n), P_(n * n), komi_(komi), st_(goStatic(n))
    {
        rot_ = rotationTables(n, n * n + 1);
        reset();
    }
    std::unique_ptr<GameEnv> clone() const override { return std::make_unique<NoGo>(*this); }
    void copyFrom(const GameEnv& o) override { *this = static_cast<const NoGo&>(o); }
    void reset() override
    {
        turn_ = 1;
        action_ids_.clear();
        action_players_.clear();
        memset(board_, 0, sizeof(board_));
        hist_len_ = 0;
        for (auto& h : hist_) { h[0].clear(); h[1].clear(); }
        stones_[0].clear();
        stones_[1].clear();
    }
    // liberties of the block at `start`, counted up to `cap`
    int liberties(int start, int cap) const
    {
        uint8_t mark[kMaxP];
        int16_t grp[kMaxP];
        memset(mark, 0, P_);
        const uint8_t color = board_[start];
        int head = 0, tail = 0, libs = 0;
        grp[tail++] = static_cast<int16_t>(start);
        mark[start] = 1;
        while (head < tail) {
            const int p = grp[head++];
            for (int k = 0; k < st_->nnbr[p]; ++k) {
                const int q = st_->nbr[p][k];
                if (mark[q]) { continue; }
                mark[q] = 1;
                if (board_[q] == 0) { if (++libs >= cap) { return libs; } }
                else if (board_[q] == color) { grp[tail++] = static_cast<int16_t>(q); }
            }
        }
        return libs;
    }
    bool isLegal(int a, int player) const override // ref nogo.h:25-57
    {
        if (a < 0 || a >= P_ || board_[a] != 0) { return false; } // (the pass slot of the policy is never legal: nogo.h:30)
        bool ok = false;
        for (int k = 0; k < st_->nnbr[a]; ++k) {
            const int q = st_->nbr[a][k];
            if (board_[q] == 0) { ok = true; continue; }
            const int libs = liberties(q, 2);
            if (board_[q] == player) { ok |= libs > 1; }
            else if (libs == 1) { return false; } // its last liberty is `a`: the move would capture
        }
        return ok; // else suicide: no empty neighbour and no own block that keeps a liberty
    }
    void legalMask(uint8_t* out) const override
    {
        for (int a = 0; a < P_; ++a) { out[a] = isLegal(a, turn_); }
        out[P_] = 0;
    }
    bool act(int a, int player) override
    {
        if (!isLegal(a, player)) { return false; }
        actUnchecked(a, player);
        return true;
    }
    void actUnchecked(int a, int player) override // GoEnv::act (ref go.cpp:132-190) of a move that captures nothing
    {
        action_ids_.push_back(static_cast<int16_t>(a));
        action_players_.push_back(static_cast<uint8_t>(player));
        turn_ = 3 - player;
        if (a >= 0 && a < P_) {
            board_[a] = static_cast<uint8_t>(player);
            stones_[player - 1].set(a);
        }
        hist_[hist_len_ & 7][0] = stones_[0];
        hist_[hist_len_ & 7][1] = stones_[1];
        ++hist_len_;
    }
    bool isTerminal() const override // ref nogo.h:59-66
    {
        for (int a = 0; a < P_; ++a) { if (isLegal(a, turn_)) { return false; } }
        return true;
    }
    float evalScore(bool) const override { return scoreOf(3 - turn_); } // ref nogo.h:68-76: the player not to move, resign or not
    void features(int r, float* out) const override // GoEnv::getFeatures (ref go.cpp:280-308)
    {
        const int* map = rot_->inv[r].data();
        for (int k = 0; k < 8; ++k) {
            float* own = out + (2 * k) * P_;
            float* opp = own + P_;
            if (hist_len_ - 1 - k < 0) {
                memset(own, 0, 2 * P_ * sizeof(float));
                continue;
            }
            const Bits* h = hist_[(hist_len_ - 1 - k) & 7];
            const Bits& mine = h[turn_ - 1];
            const Bits& theirs = h[2 - turn_];
            for (int p = 0; p < P_; ++p) {
                own[p] = mine.test(map[p]) ? 1.0f : 0.0f;
                opp[p] = theirs.test(map[p]) ? 1.0f : 0.0f;
            }
        }
        const float b = turn_ == 1 ? 1.0f : 0.0f, w = turn_ == 2 ? 1.0f : 0.0f;
        for (int p = 0; p < P_; ++p) { out[16 * P_ + p] = b; out[17 * P_ + p] = w; }
    }
    GameKind deviceKind() const override { return kNoGo; }
    void exportDeviceRoot(void* dst) const override // (go_body.h nogoLeafBody: the stones, the ring of past positions, the player to move)
    {
        static_assert(kWords == kGoMaxW, "device snapshot layout");
        GoRootSnapshot& s = *static_cast<GoRootSnapshot*>(dst);
        memcpy(s.stones, stones_, sizeof(s.stones));
        memcpy(s.hist, hist_, sizeof(s.hist));
        s.hash = 0;
        s.hist_len = hist_len_;
        s.turn = turn_;
        s.nmoves = static_cast<int32_t>(action_ids_.size());
        s.passes = 0;
    }
    int numInputChannels() const override { return 18; }
    int boardSize() const override { return n_; }
    int policySize() const override { return P_ + 1; }
    std::string name() const override { return "nogo_" + std::to_string(n_) + "x" + std::to_string(n_); }
    std::vector<std::pair<std::string, std::string>> loaderTags() const override // the loader is Go's (ref nogo.h:88, go.h:127-133)
    {
        return {{"SZ", std::to_string(n_)}, {"KM", std::to_string(komi_)}};
    }

private:
    int n_, P_;
    float komi_; // carried in the KM tag only
    const GoStatic* st_;
    uint8_t board_[kMaxP];
    Bits stones_[2];
    Bits hist_[8][2];
    int hist_len_;
};

// ---------------------------------------------------------------------------------------------
// Havannah (ref havannah.h:37-75, havannah.cpp:38-231,272-496): a game past the rows of game_kind.h with facts of its own (kHavannah).  Edge size N
// (env_board_size, the record's SZ, name()) plays on an E x E array, E = 2N - 1 = boardSize(): cell (i, j) has id i * E + j and is on the board iff
// N - 1 <= i + j <= 3N - 3 (havannah.cpp:321-327); its neighbours are (i-1,j) (i-1,j+1) (i,j-1) (i,j+1) (i+1,j-1) (i+1,j) (havannah.cpp:301-303).  E * E
// actions, no pass, off-board cells never legal, no symmetries.  With the swap rule every on-board cell is legal on the second action, and choosing the
// occupied one makes that cell White's where it is (havannah.cpp:113-122).  THE QUIRK THAT IS KEPT: the reference's feature bitboards never clear Black's bit
// on a swap (havannah.cpp:147 only sets), so from then on the cell is in both history planes while its owner is White — fb_ are those two bitboards as
// the reference keeps them, and a cell's owner is black = fb_[0] & ~fb_[1], white = fb_[1].
// The mover wins when the group through the new stone holds two corners (bridge), meets three sides (fork; the corners belong to no side,
// havannah.cpp:64-86) or closes a ring (isCycle, havannah.cpp:377-395: >= 6 cells, the new stone has >= 2 own neighbours, and either a neighbour of the new
// stone has six own neighbours or detectHole).  detectHole (havannah.cpp:407-496) floods the complement of the group inside the group's bounding box plus a
// frame of one cell; everything outside the box is complement and joined to the frame, so this is a flood of the complement over the whole E x E array
// from its rim — the form used here and on the device.  The reference joins groups incrementally; here the group is found by a flood.
// ---------------------------------------------------------------------------------------------
// MZ_HAV_PROF=1 (measurements, tools/hav_flood_share.py): how many win tests ran, passed the ring's two gates, and went on to flood the complement —
// counted on the host engine, whose leaves under mz_device_env=false are the device engine's leaves (the records of the paths are equal).  Printed at exit.
struct HavProf {
    const bool on = getenv("MZ_HAV_PROF") != nullptr;
    std::atomic<long> tests{0}, gated{0}, flooded{0};
    ~HavProf() { if (on) { fprintf(stderr, "havannah win tests %ld, past the ring's gates %ld, complement floods %ld\n", tests.load(), gated.load(), flooded.load()); } }
};
static HavProf g_hav_prof;

class Havannah final : public GameEnv {
public:
    Havannah(int edge, bool swap) : N_(edge), n_(2 * edge - 1), P_(n_ * n_), swap_(swap)
    {
        rot_ = rotationTables(n_, P_, true);
        valid_.clear();
        corners_.clear();
        for (auto& s : sides_) { s.clear(); }
        cells_ = 0;
        for (int i = 0; i < n_; ++i) { for (int j = 0; j < n_; ++j) { if (onBoard(i, j)) { valid_.set(i * n_ + j); ++cells_; } } }
        const int N = N_, E = n_;
        for (int i = 0; i < N - 2; ++i) { // havannah.cpp:69-76
            sides_[0].set(N + i);
            sides_[1].set((i + 1) * E + N - 2 - i);
            sides_[2].set((N + i) * E);
            sides_[3].set((E - 1) * E + 1 + i);
            sides_[4].set((E - 1 - i) * E - N + 1 + i);
            sides_[5].set((N - 1 - i) * E - 1);
        }
        for (int c : {N - 1, E - 1, (N - 1) * E, N * E - 1, (E - 1) * E, (E - 1) * E - 1 + N}) { corners_.set(c); } // havannah.cpp:79-85
        reset();
    }
    std::unique_ptr<GameEnv> clone() const override { return std::make_unique<Havannah>(*this); }
    void copyFrom(const GameEnv& o) override { *this = static_cast<const Havannah&>(o); }
    void reset() override
    {
        turn_ = 1;
        action_ids_.clear();
        action_players_.clear();
        fb_[0].clear();
        fb_[1].clear();
        for (auto& h : hist_) { h[0].clear(); h[1].clear(); }
        hist_len_ = 0;
        winner_ = 0;
        first_ = -1;
    }
    bool onBoard(int i, int j) const { return i >= 0 && i < n_ && j >= 0 && j < n_ && i + j >= N_ - 1 && i + j <= 3 * N_ - 3; } // havannah.cpp:321-327
    int owner(int p) const { return fb_[1].test(p) ? 2 : (fb_[0].test(p) ? 1 : 0); }
    bool isLegal(int a, int) const override // ref havannah.cpp:164-177
    {
        if (a < 0 || a >= P_ || !valid_.test(a)) { return false; }
        return (swap_ && hist_len_ == 1) || owner(a) == 0;
    }
    void legalMask(uint8_t* out) const override { for (int a = 0; a < P_; ++a) { out[a] = isLegal(a, turn_); } }
    bool act(int a, int player) override
    {
        if (!isLegal(a, player)) { return false; }
        actUnchecked(a, player);
        return true;
    }
    void actUnchecked(int a, int player) override // ref havannah.cpp:107-151
    {
        action_ids_.push_back(static_cast<int16_t>(a)); // the chosen id, also for a swap (B[k];W[k])
        action_players_.push_back(static_cast<uint8_t>(player));
        turn_ = 3 - player;
        if (hist_len_ == 0) { first_ = a; }
        // a swap (the second action repeats the first, rule on) needs nothing more than the stone: White's bit decides the owner, Black's bit stays (the quirk)
        fb_[player - 1].set(a);
        hist_[hist_len_ & 7][0] = fb_[0];
        hist_[hist_len_ & 7][1] = fb_[1];
        ++hist_len_;
        if (winner_ == 0 && wins(a, player)) { winner_ = player; } // a winner never goes away
    }
    template <class F>
    void forNeighbours(int p, F&& f) const // the on-board neighbours (havannah.cpp:293-313)
    {
        static const int di[6] = {-1, -1, 0, 0, 1, 1}, dj[6] = {0, 1, -1, 1, -1, 0};
        const int i = p / n_, j = p % n_;
        for (int k = 0; k < 6; ++k) { if (onBoard(i + di[k], j + dj[k])) { f((i + di[k]) * n_ + j + dj[k]); } }
    }
    int ownNeighbours(int p, int player) const // havannah.cpp:397-405
    {
        int c = 0;
        forNeighbours(p, [&](int q) { c += owner(q) == player; });
        return c;
    }
    bool wins(int a, int player) const // havannah.cpp:272-291 on the group through `a`
    {
        Bits grp;
        grp.clear();
        int16_t stack[kMaxP];
        int top = 0, size = 0;
        stack[top++] = static_cast<int16_t>(a);
        grp.set(a);
        while (top) {
            const int p = stack[--top];
            ++size;
            forNeighbours(p, [&](int q) {
                if (owner(q) == player && !grp.test(q)) { grp.set(q); stack[top++] = static_cast<int16_t>(q); }
            });
        }
        if (g_hav_prof.on) { ++g_hav_prof.tests; }
        int corners = 0, sides = 0;
        for (int w = 0; w < kWords; ++w) { corners += __builtin_popcountll(grp.w[w] & corners_.w[w]); }
        if (corners >= 2) { return true; } // bridge
        for (const Bits& s : sides_) {
            bool meets = false;
            for (int w = 0; w < kWords; ++w) { meets |= (grp.w[w] & s.w[w]) != 0; }
            sides += meets;
        }
        if (sides >= 3) { return true; } // fork
        if (size < 6 || ownNeighbours(a, player) < 2) { return false; } // havannah.cpp:380-385
        bool interior = false;
        forNeighbours(a, [&](int q) { interior |= ownNeighbours(q, player) == 6; }); // havannah.cpp:388-391: a neighbour of any colour, empty or not
        if (g_hav_prof.on) { ++g_hav_prof.gated; g_hav_prof.flooded += interior ? 0 : 1; }
        return interior || hasHole(grp);
    }
    // a cell of the array outside the group that the array's rim cannot reach through cells outside the group (six-neighbour adjacency, off-board cells included)
    bool hasHole(const Bits& grp) const
    {
        Bits seen;
        seen.clear();
        int16_t stack[kMaxP];
        int top = 0;
        for (int p = 0; p < P_; ++p) {
            const int i = p / n_, j = p % n_;
            if ((i == 0 || j == 0 || i == n_ - 1 || j == n_ - 1) && !grp.test(p)) { seen.set(p); stack[top++] = static_cast<int16_t>(p); }
        }
        static const int di[6] = {-1, -1, 0, 0, 1, 1}, dj[6] = {0, 1, -1, 1, -1, 0};
        while (top) {
            const int p = stack[--top], i = p / n_, j = p % n_;
            for (int k = 0; k < 6; ++k) {
                const int u = i + di[k], v = j + dj[k];
                if (u < 0 || u >= n_ || v < 0 || v >= n_) { continue; }
                const int q = u * n_ + v;
                if (grp.test(q) || seen.test(q)) { continue; }
                seen.set(q);
                stack[top++] = static_cast<int16_t>(q);
            }
        }
        for (int p = 0; p < P_; ++p) { if (!grp.test(p) && !seen.test(p)) { return true; } }
        return false;
    }
    bool isTerminal() const override // ref havannah.cpp:179-184: a winner, or no empty cell on the board (a draw)
    {
        if (winner_ != 0) { return true; }
        int stones = 0;
        for (int w = 0; w < kWords; ++w) { stones += __builtin_popcountll(fb_[0].w[w] | fb_[1].w[w]); }
        return stones == cells_;
    }
    float evalScore(bool is_resign) const override { return scoreOf(is_resign ? 3 - turn_ : winner_); } // ref havannah.cpp:186-194
    bool swappable() const { return swap_ && hist_len_ == 1; } // ref havannah.h isSwappable
    void features(int, float* out) const override // ref havannah.cpp:196-231 (the rotation is the identity: havannah.h:71)
    {
        for (int k = 0; k < 8; ++k) {
            float* own = out + (2 * k) * P_;
            float* opp = own + P_;
            // (the reference's history starts with the empty position, whose planes are as empty as those of a position that does not exist)
            if (hist_len_ - 1 - k < 0) {
                memset(own, 0, 2 * P_ * sizeof(float));
                continue;
            }
            const Bits* h = hist_[(hist_len_ - 1 - k) & 7];
            for (int p = 0; p < P_; ++p) {
                own[p] = h[turn_ - 1].test(p) ? 1.0f : 0.0f;
                opp[p] = h[2 - turn_].test(p) ? 1.0f : 0.0f;
            }
        }
        const float sw = swappable() ? 1.0f : 0.0f, b = turn_ == 1 ? 1.0f : 0.0f, w = turn_ == 2 ? 1.0f : 0.0f;
        for (int p = 0; p < P_; ++p) {
            out[16 * P_ + p] = valid_.test(p) ? 1.0f : 0.0f;
            out[17 * P_ + p] = sw;
            out[18 * P_ + p] = b;
            out[19 * P_ + p] = w;
        }
    }
    int actionFromString(const std::string& str) const override // console coordinates on the E x E array (havannah.h:30), on-board cells only; no pass
    {
        std::string up = str;
        for (char& c : up) { c = static_cast<char>(std::toupper(static_cast<unsigned char>(c))); }
        if (up == "PASS") { return -1; }
        const int a = GameEnv::actionFromString(str);
        return a >= 0 && a < P_ && valid_.test(a) ? a : -1;
    }
    GameKind deviceKind() const override { return kHavannah; }
    void exportDeviceRoot(void* dst) const override // (go_body.h havLeafBody: the two feature bitboards, the ring of past positions, the winner, the swap flag)
    {
        static_assert(kWords == kGoMaxW, "device snapshot layout");
        GoRootSnapshot& s = *static_cast<GoRootSnapshot*>(dst);
        memcpy(s.stones, fb_, sizeof(s.stones));
        memcpy(s.hist, hist_, sizeof(s.hist));
        s.hash = swap_ ? kHavSwap : 0; // (hist_len is taken by the ring, so the rule flag travels in the word only Go uses)
        s.hist_len = hist_len_;
        s.turn = turn_;
        s.nmoves = static_cast<int32_t>(action_ids_.size());
        s.winner() = winner_;
    }
    int numInputChannels() const override { return gameChannels(kHavannah); }
    int boardSize() const override { return n_; } // the network board E (game_kind.h networkBoard); the edge size is in name() and the SZ tag
    int policySize() const override { return P_; }
    std::string name() const override { return "havannah" + std::to_string(N_) + "x" + std::to_string(N_); } // ref havannah.h:68 (no underscore)
    std::vector<std::pair<std::string, std::string>> loaderTags() const override { return {{"SZ", std::to_string(N_)}}; } // the edge size (base_env.h: SZ = env_board_size)

private:
    int N_, n_, P_; // edge size, side of the array, cells of the array
    bool swap_;
    int cells_;     // cells on the board: 3N(N - 1) + 1
    Bits valid_, corners_, sides_[6];
    Bits fb_[2];    // the reference's bitboard_pair_ (black keeps the bit of a swapped stone)
    Bits hist_[8][2];
    int hist_len_;  // positions so far = actions played (a swap is one)
    int winner_, first_;
};

// ---------------------------------------------------------------------------------------------
// Atari-shaped synthetic environment (BASELINE configs[4]; ALE, OpenCV and the ROMs are not available).
// Feature contract of the reference's AtariEnv (ref atari.h:17-27, atari.cpp:48-131): 1 player, 18 actions all legal,
// features = for the last 8 steps [1 plane action_id / 18, 3 planes RGB / 255 of a 96x96 screen], oldest first.
// Screens are kept as bytes in an 8-deep ring (27 KB each) and expanded to f32 only when the planes are written.
// ---------------------------------------------------------------------------------------------
class AtariSynth final : public GameEnv {
    static constexpr int kRes = 96, kHist = 8, kActions = 18, kFrame = 3 * kRes * kRes;
    static uint64_t mix(uint64_t z)
    {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
public:
    AtariSynth(const std::string& name, int episode_length, size_t recent_observations)
        : name_(name), episode_length_(episode_length), recent_(recent_observations), frames_(size_t(kHist) * kFrame, 0) { resetSeed(0); }
    std::unique_ptr<GameEnv> clone() const override { return std::make_unique<AtariSynth>(*this); }
    void copyFrom(const GameEnv& o) override { *this = static_cast<const AtariSynth&>(o); }
    bool needsSeed() const override { return true; }
    void reset() override { resetSeed(0); }
    void resetSeed(int seed) override
    {
        turn_ = 1;
        seed_ = seed;
        reward_ = total_reward_ = 0;
        action_ids_.clear();
        action_players_.clear();
        std::fill(frames_.begin(), frames_.end(), 0);
        for (auto& v : valid_) { v = false; }
        for (auto& a : action_plane_) { a = 0.0f; }
        head_ = 0;
        pending_.clear();
        pushed_ = 0;
        lives_.clear();
        lives_.push_back(livesAt(0)); // ref atari.cpp:61-62
        lost_ = 0;
        observations_.clear();
        pushFrame(0, 0.0f, false);
    }
    bool isLegal(int a, int) const override { return a >= 0 && a < kActions; }
    bool act(int a, int player) override
    {
        if (!isLegal(a, player)) { return false; }
        actUnchecked(a, player);
        return true;
    }
    void actUnchecked(int a, int player) override
    {
        const int step = static_cast<int>(action_ids_.size()) + 1;
        const uint64_t h = mix(static_cast<uint64_t>(static_cast<uint32_t>(seed_)) * 0x9E3779B97F4A7C15ULL + 0x5157ULL * step);
        reward_ = ((h >> 40) < uint64_t(0.05 * (1 << 24))) ? 1.0f : 0.0f;
        total_reward_ += reward_;
        lost_ += (mix(static_cast<uint64_t>(static_cast<uint32_t>(seed_)) * 0xA24BAED4963EE407ULL + 0x11F3ULL * step) % 23) == 0;
        lives_.push_back(lost_ >= 3 ? 0 : 3 - lost_); // ref atari.cpp:83: the synthetic ale_.lives()
        action_ids_.push_back(static_cast<int16_t>(a));
        action_players_.push_back(static_cast<uint8_t>(player));
        pushFrame(step, a * 1.0f / kActions, true);
    }
    void legalMask(uint8_t* out) const override { for (int a = 0; a < kActions; ++a) { out[a] = 1; } }
    bool isTerminal() const override { return static_cast<int>(action_ids_.size()) >= episode_length_; }
    float evalScore(bool) const override { return total_reward_; }
    float reward() const override { return reward_; }
    void features(int, float* out) const override
    {
        materialize();
        for (int i = 0; i < kHist; ++i) { // oldest first; slot = (head_ + i) % kHist
            const int slot = (head_ + i) % kHist;
            float* dst = out + size_t(i) * 4 * kRes * kRes;
            const float av = action_plane_[slot];
            for (int p = 0; p < kRes * kRes; ++p) { dst[p] = av; }
            float* rgb = dst + kRes * kRes;
            if (!valid_[slot]) {
                memset(rgb, 0, size_t(kFrame) * sizeof(float));
            } else {
                const uint8_t* f = frames_.data() + size_t(slot) * kFrame;
                for (int p = 0; p < kFrame; ++p) { rgb[p] = static_cast<float>(f[p]) / 255.0f; }
            }
        }
    }
    // raw form of features(): the 8 screens oldest first (3 x 96 x 96 bytes each), then 8 f32 action-plane values, then 8 valid bytes
    int rawFeatureBytes() const override { return kHist * kFrame + kHist * 4 + kHist; }
    void rawFeatures(uint8_t* dst) const override
    {
        materialize();
        float av[kHist];
        for (int i = 0; i < kHist; ++i) {
            const int slot = (head_ + i) % kHist;
            memcpy(dst + size_t(i) * kFrame, frames_.data() + size_t(slot) * kFrame, kFrame);
            av[i] = action_plane_[slot];
            dst[size_t(kHist) * kFrame + kHist * 4 + i] = valid_[slot] ? 1 : 0;
        }
        memcpy(dst + size_t(kHist) * kFrame, av, sizeof(av));
    }
    uint64_t rawSerial() const override { return serial_; }
    int rawValidCount() const override { return pushed_ < kHist ? pushed_ : kHist; } // (no screen is drawn for this)
    int rawFrameBytes() const override { return kFrame; }
    void rawNewest(uint8_t* frame, uint8_t* meta) const override
    {
        materialize();
        memcpy(frame, frames_.data() + size_t((head_ + kHist - 1) % kHist) * kFrame, kFrame);
        float av[kHist];
        for (int i = 0; i < kHist; ++i) {
            const int slot = (head_ + i) % kHist;
            av[i] = action_plane_[slot];
            meta[kHist * 4 + i] = valid_[slot] ? 1 : 0;
        }
        memcpy(meta, av, sizeof(av));
    }
    int numInputChannels() const override { return kHist * 4; }
    int boardSize() const override { return kRes; }
    int policySize() const override { return kActions; }
    int numPlayers() const override { return 1; }
    std::string name() const override { return "atari_" + name_; }
    int actionFromString(const std::string& str) const override // ref atari.cpp:9-39: ALE's action names without their PLAYER_A_ prefix, upper-cased
    {
        static const char* const kNames[18] = {"NOOP", "FIRE", "UP", "RIGHT", "LEFT", "DOWN", "UPRIGHT", "UPLEFT", "DOWNRIGHT", "DOWNLEFT", "UPFIRE", "RIGHTFIRE", "LEFTFIRE",
                                               "DOWNFIRE", "UPRIGHTFIRE", "UPLEFTFIRE", "DOWNRIGHTFIRE", "DOWNLEFTFIRE"};
        std::string up = str;
        for (char& c : up) { c = static_cast<char>(std::toupper(static_cast<unsigned char>(c))); }
        for (int a = 0; a < 18; ++a) { if (up == kNames[a]) { return a; } }
        return -1;
    }
    std::vector<std::pair<std::string, std::string>> loaderTags() const override { return {{"SD", std::to_string(seed_)}}; }
    bool hasObservations() const override { return true; }
    void appendObservations(std::string* out) const override { materialize(); for (const auto& o : observations_) { out->append(o); } }
    const std::vector<int>* livesHistory() const override { return &lives_; }

private:
    int livesAt(int) const { return 3; }
    // A step only notes which screen is due: the 27-KB screen and its observation string are drawn when somebody looks at them (the
    // worker's leaf / record builders, which run one game per thread), not inside the RNG-ordered serial section of a move, where the 64
    // games of a pool would draw theirs one after the other with the GPU waiting (0.3 ms of a 7-ms move on BASELINE configs[4]).
    struct PendingFrame { int step; float action_value; bool with_action; };
    void pushFrame(int step, float action_value, bool with_action)
    {
        pending_.push_back(PendingFrame{step, action_value, with_action});
        ++pushed_;
        ++serial_;
    }
    void materialize() const
    {
        if (pending_.empty()) { return; }
        AtariSynth* self = const_cast<AtariSynth*>(this); // the ring and the observation list are caches of (seed, steps)
        for (const PendingFrame& p : pending_) { self->drawFrame(p.step, p.action_value, p.with_action); }
        self->pending_.clear();
    }
    void drawFrame(int step, float action_value, bool with_action)
    {
        // ring of the last 8 (action, screen) pairs: overwrite the oldest slot, which then becomes the newest
        const int slot = head_;
        uint8_t* f = frames_.data() + size_t(slot) * kFrame;
        // the synthetic screen of (seed, step): one hash byte per 8x8 block of every colour plane — piecewise constant like a real frame
        const uint64_t base = static_cast<uint64_t>(static_cast<uint32_t>(seed_)) * 0xD1B54A32D192ED03ULL + static_cast<uint64_t>(step) * 0x100000001B3ULL;
        constexpr int kB = kRes / 8;
        for (int cy = 0; cy < 3 * kB; ++cy) { // (plane, block row)
            uint8_t row[kRes];
            for (int bx = 0; bx < kB; ++bx) {
                const uint8_t v = static_cast<uint8_t>(mix(base + static_cast<uint64_t>(cy * kB + bx) * 0x9E3779B97F4A7C15ULL) >> 56);
                memset(row + bx * 8, v, 8);
            }
            for (int y = 0; y < 8; ++y) { memcpy(f + (size_t(cy) * 8 + y) * kRes, row, kRes); }
        }
        // ref atari.cpp:85-91: the observation string of the step, older ones dropped beyond the configured window
        observations_.emplace_back(reinterpret_cast<const char*>(f), size_t(kFrame));
        if (observations_.size() > recent_) {
            std::string& old = observations_[observations_.size() - recent_];
            old.clear();
            old.shrink_to_fit();
        }
        valid_[slot] = true;
        action_plane_[slot] = with_action ? action_value : 0.0f;
        head_ = (head_ + 1) % kHist;
    }
    uint64_t serial_ = 0;
    mutable std::vector<PendingFrame> pending_;
    int pushed_ = 0;
    std::string name_;
    int episode_length_, seed_ = 0, head_ = 0, lost_ = 0;
    size_t recent_;
    float reward_ = 0, total_reward_ = 0;
    std::vector<int> lives_;
    std::vector<std::string> observations_;
    std::vector<uint8_t> frames_;
    bool valid_[kHist] = {};
    float action_plane_[kHist] = {};
};

std::unique_ptr<GameEnv> createGameEnv(const EnvOptions& o)
{
    if (o.game == "atari") { return std::make_unique<AtariSynth>(o.atari_name, o.atari_episode_length, std::max<size_t>(1, o.atari_recent_observations)); }
    const GameKind k = gameFromName(o.game.c_str());
    if (k == kNoDeviceGame) { setError("unknown env_game '%s' (tictactoe | go | nogo | othello | gomoku | hex | havannah | atari)", o.game.c_str()); return nullptr; }
    const int n = o.board_size > 0 ? o.board_size : gameDefaultBoard(k);
    static_assert(gameMaxBoard(kGo) <= kMaxN && gameMaxBoard(kGomoku) <= kMaxN && gameMaxBoard(kHex) <= kMaxN && networkBoard(kHavannah, gameMaxBoard(kHavannah)) <= kMaxN, "the table's boards fit the engines' arrays");
    switch (k) {
    case kTicTacToe: return std::make_unique<TicTacToe>();
    case kOthello:
        if (n < gameMinBoard(k) || n > gameMaxBoard(k) || n % 2) { setError("othello board size %d not supported (even, %d..%d)", n, gameMinBoard(k), gameMaxBoard(k)); return nullptr; }
        return std::make_unique<Othello>(n);
    case kGo:
        if (n < gameMinBoard(k) || n > gameMaxBoard(k)) { setError("go board size %d not supported (%d..%d)", n, gameMinBoard(k), gameMaxBoard(k)); return nullptr; }
        if (o.go_ko_rule != "positional" && o.go_ko_rule != "situational") { setError("env_go_ko_rule '%s' not supported (positional | situational, ref go.cpp:47)", o.go_ko_rule.c_str()); return nullptr; }
        return std::make_unique<Go>(n, o.go_komi, o.go_ko_rule == "situational");
    case kNoGo: // ref nogo.h:12,22: 9x9; the smaller boards are for tests.  env_go_ko_rule is not read: nothing is captured, no position repeats
        if (n < gameMinBoard(k) || n > gameMaxBoard(k)) { setError("nogo board size %d not supported (%d..%d)", n, gameMinBoard(k), gameMaxBoard(k)); return nullptr; }
        return std::make_unique<NoGo>(n, o.go_komi);
    case kGomoku: // ref gomoku.h:13,21,44
        if (n > gameMaxBoard(k)) { setError("gomoku board size %d not supported (up to %d)", n, gameMaxBoard(k)); return nullptr; }
        return std::make_unique<Gomoku>(n, o.gomoku_rule == "outer_open", o.gomoku_exactly_five);
    case kHex: // ref hex.h:12,63
        if (n < gameMinBoard(k) || n > gameMaxBoard(k)) { setError("hex board size %d not supported (%d..%d)", n, gameMinBoard(k), gameMaxBoard(k)); return nullptr; }
        return std::make_unique<Hex>(n, o.hex_use_swap_rule);
    case kHavannah: // ref havannah.h:41,74: edge size 8; the array of edge size 10 is 19 x 19, the widest the bitboards hold
        if (n < gameMinBoard(k)) { setError("havannah board size %d not supported: the edge size is at least %d (ref havannah.h:41)", n, gameMinBoard(k)); return nullptr; }
        if (n > gameMaxBoard(k)) { setError("havannah board size %d not supported: edge sizes up to %d (a %dx%d array) have an engine", n, gameMaxBoard(k), networkBoard(k, gameMaxBoard(k)), networkBoard(k, gameMaxBoard(k))); return nullptr; }
        return std::make_unique<Havannah>(n, o.havannah_use_swap_rule);
    default: return nullptr;
    }
}

std::unique_ptr<GameEnv> createGameEnv(const std::string& game, int board_size, float go_komi, const std::string& atari_name, int atari_episode_length,
                                       const std::string& go_ko_rule, size_t atari_recent_observations, const std::string& gomoku_rule, bool gomoku_exactly_five,
                                       bool hex_use_swap_rule)
{
    EnvOptions o;
    o.game = game;
    o.board_size = board_size;
    o.go_komi = go_komi;
    o.go_ko_rule = go_ko_rule;
    o.gomoku_rule = gomoku_rule;
    o.gomoku_exactly_five = gomoku_exactly_five;
    o.hex_use_swap_rule = hex_use_swap_rule;
    o.atari_name = atari_name;
    o.atari_episode_length = atari_episode_length;
    o.atari_recent_observations = atari_recent_observations;
    return createGameEnv(o);
}

} // namespace mz
