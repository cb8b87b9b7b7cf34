"""Records for the learner-side sampler's tests, built on the oracle's rules engine alone (no GPU): random legal playouts, hand-built Go games that pin
what self-play only meets by chance (multi-group captures, merges, kos, snapbacks, chains across the 64-point words of the device's bitboards, captures of
more than one word, the move cap, passes), one-position records around the edges of the device replay's window of kept positions, and records with a move
the rules refuse.  tests/test_loader_cases.py checks every claim made here with the oracle; tests/test_gpu_loader_boards.py feeds the records to the
product's DataLoader and compares with the oracle's, and with the product's host engine.

A position `k` of a record is the state after its first k moves (the planes a sample (game, k) holds); move `i` (0-based) leads from position i to i + 1."""
import functools

import numpy as np

import oracle_lib


def go_conf(n, ko="positional"):
    return f"env_game=go:env_board_size={n}" + (":env_go_ko_rule=situational" if ko == "situational" else "")


def game_conf(game, n, ko="positional"):
    if game == "go":
        return go_conf(n, ko)
    return "env_game=tictactoe" if game == "tictactoe" else f"env_game={game}:env_board_size={n}"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# records and playouts
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def record(n, actions, dlen=None, game="go", reward=False):
    """The bare record the server's sgf file holds: numeric actions, colours alternating from B, no P tag (a one-hot policy).  `dlen` = (first, last)
    sampled position; `reward` adds the R tag MuZero's reward target reads."""
    s = f"(;GM[{game}]RE[1]SZ[{n}]" + (f"DLEN[{dlen[0]}-{dlen[1]}]" if dlen is not None else "")
    for i, a in enumerate(actions):
        s += f";{'BW'[i & 1]}[{a}]" + ("R[0]" if reward else "")
    return s + ")"


def playout(n, seed, max_moves=None, pass_prob=0.0, ko="positional", game="go", region=None, end_with_passes=True):
    """A random legal game as a list of actions.  A pass is drawn with `pass_prob` (never twice in a row: single passes in the middle) and played when
    no other move is legal.  Without `max_moves` the game runs to its natural end (for Go with pass_prob = 0 usually the cap of 2 * n * n + 1 moves);
    with it, the game has at most that many moves and, `end_with_passes`, ends by two passes.  `region` = (moves, k): the first `moves` moves stay
    in the k x k corner at the origin where a legal point is there (captures early in the game, on any board)."""
    rng = np.random.default_rng(seed)
    env = oracle_lib.OracleEnv(game_conf(game, n, ko))
    P = n * n
    acts = []
    while not env.is_terminal() and (max_moves is None or len(acts) < max_moves):
        if max_moves is not None and end_with_passes and game == "go" and len(acts) >= max_moves - 2:
            a = P
        else:
            legal = np.nonzero(env.legal_mask())[0]
            board = legal[legal != P]
            if region is not None and len(acts) < region[0]:
                near = board[(board % n < region[1]) & (board // n < region[1])]
                board = near if len(near) else board
            may_pass = game == "go" and pass_prob > 0 and not (acts and acts[-1] == P)
            a = P if (len(board) == 0 or (may_pass and rng.random() < pass_prob)) else int(rng.choice(board))
        assert env.act(a), (n, seed, len(acts), a)
        acts.append(a)
    return acts


def go_board(env, n):
    """(black, white) boolean arrays of the oracle's Go / 4-plane environment as it stands (unrotated planes)"""
    f = env.features(0).reshape(-1, n * n)
    black_to_move = f[-2, 0] == 1.0
    own, opp = f[0] > 0, f[1] > 0
    return (own, opp) if black_to_move else (opp, own)


def stone_counts(n, actions, ko="positional", game="go"):
    """[k] = (black, white) stones at position k, replayed on the oracle; every move must be legal"""
    env = oracle_lib.OracleEnv(game_conf(game, n, ko))
    out = [(0, 0)] if game == "go" else [tuple(int(x.sum()) for x in go_board(env, n))]
    for i, a in enumerate(actions):
        assert env.act(a, 1 + (i & 1)), f"move {i} ({a}) is illegal"
        b, w = go_board(env, n)
        out.append((int(b.sum()), int(w.sum())))
    return out


def capture_moves(n, actions, upto=None, ko="positional"):
    """indices of the moves of a legal Go game that remove at least one stone"""
    c = stone_counts(n, actions[:upto], ko)
    return [i for i in range(len(c) - 1) if sum(c[i + 1]) < sum(c[i]) + (actions[i] != n * n)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hand-built Go games
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def neighbours(n, p):
    x, y = p % n, p // n
    return [q for q, ok in ((p + n, y + 1 < n), (p + 1, x + 1 < n), (p - n, y > 0), (p - 1, x > 0)) if ok]


def border(n, chain):
    """the points next to a chain, in board order"""
    return sorted({q for p in chain for q in neighbours(n, p)} - set(chain))


def tempo(n, black, white, then=()):
    """Black's and White's stones in their own orders, alternating from Black; the side that has run out (or whose turn it is not, in `then`: (colour,
    point) pairs played in order afterwards) passes.  Passes are never consecutive: a stone follows each."""
    seq = []
    for i in range(max(len(black), len(white))):
        seq += [(1, black[i])] if i < len(black) else []
        seq += [(2, white[i])] if i < len(white) else []
    seq += list(then)
    acts = []
    for colour, p in seq:
        if 1 + (len(acts) & 1) != colour:
            acts.append(n * n)
        acts.append(p)
    return acts


def finish(n, acts, ko="positional"):
    """three quiet moves after the game's last one (a pass, a stone that captures nothing, a pass), so that the positions after the key move
    lie inside the record and inside the part of it the device replays on one wave state"""
    env = oracle_lib.OracleEnv(go_conf(n, ko))
    for i, a in enumerate(acts):
        assert env.act(a, 1 + (i & 1)), f"move {i} ({a}) is illegal"
    acts = acts + [n * n]
    assert env.act(n * n)
    before = sum(int(x.sum()) for x in go_board(env, n))
    for p in np.nonzero(env.legal_mask())[0][::-1]:  # (from the far end of the board: the cases are built near the origin or the centre)
        trial = oracle_lib.OracleEnv(go_conf(n, ko))
        for i, a in enumerate(acts):
            trial.act(a, 1 + (i & 1))
        if p != n * n and trial.act(int(p)) and sum(int(x.sum()) for x in go_board(trial, n)) == before + 1:
            return acts + [int(p), n * n]
    raise AssertionError("no quiet move")


def _case(n, acts, events, ko="positional", tail=True):
    """(n, actions, target_positions, claim): claim = {"ko": rule, "events": [event]}, an event = dict(move=i, ...) with
         captured=k, groups=g, points=[...]   move i removes exactly k enemy stones in g groups, `points` among them (k = 0: none)
         merged=m, chain=[...]                before move i the mover has m distinct groups next to the point; after it `chain` is part of one group with the point
       the targets are the positions i + 1 .. i + 3 after each event's move (the position just after, and two the one-wave replay reaches)"""
    acts = finish(n, acts, ko) if tail else list(acts)
    targets = sorted({k for e in events for k in range(e["move"] + 1, e["move"] + 4) if k <= len(acts)})
    return n, acts, targets, {"ko": ko, "events": events}


def at(n, x, y):
    return y * n + x


def case_capture_groups(k, n=9, cx=4, cy=4):
    """one move captures k distinct groups: single white stones around one empty point, each with that point as its last liberty"""
    c = at(n, cx, cy)
    white = neighbours(n, c)[:k]
    black = [q for q in border(n, white) if q != c]
    acts = tempo(n, black, white, [(1, c)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=k, groups=k, points=white)])


def case_same_group_twice(captured, n=9):
    """the move touches one bent white chain on two sides (the two neighbours carry the same group id); with its last outside liberty left open it is not captured"""
    c = at(n, 4, 4)
    white = [at(n, 3, 4), at(n, 3, 3), at(n, 4, 3)]
    black = [q for q in border(n, white) if q != c]
    if not captured:
        black.remove(at(n, 2, 3))
    acts = tempo(n, black, white, [(1, c)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=3 if captured else 0, groups=1 if captured else 0, points=white if captured else [])])


def case_merge_groups(k, n=9, cx=4, cy=4):
    """one move merges k own groups: single black stones around one empty point"""
    c = at(n, cx, cy)
    black = neighbours(n, c)[:k]
    white = [at(n, i, n - 1) for i in range(k - 1)]  # (far away, for the tempo)
    acts = tempo(n, black, white, [(1, c)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=0, groups=0, points=[], merged=k, chain=black)])


def case_merge_and_capture(n=9):
    c = at(n, 4, 4)
    w = at(n, 4, 3)
    black = [at(n, 3, 4), at(n, 5, 4)] + [q for q in border(n, [w]) if q != c]
    acts = tempo(n, black, [w, at(n, 0, n - 1), at(n, 2, n - 1), at(n, 4, n - 1)], [(1, c)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=1, groups=1, points=[w], merged=2, chain=[q for q in black if q != at(n, 4, 2)])])


def ko_shape(n, ox, oy):
    """moves that end with White's capture in a ko whose two points are (ox + 1, oy + 1) and (ox + 2, oy + 1); returns (actions, a, b): White stands on a,
    Black's stone on b has just been taken"""
    a, b = at(n, ox + 1, oy + 1), at(n, ox + 2, oy + 1)
    return tempo(n, [q for q in neighbours(n, a) if q != b], [q for q in neighbours(n, b) if q != a], [(1, b), (2, a)]), a, b


def case_ko(n=9, ko="positional", ox=2, oy=2):
    """capture, a threat and its answer, then the retake"""
    acts, a, b = ko_shape(n, ox, oy)
    take = len(acts) - 1
    acts += [at(n, 0, 0), at(n, n - 1, n - 1), b]
    return _case(n, acts, [dict(move=take, captured=1, groups=1, points=[b]), dict(move=len(acts) - 1, captured=1, groups=1, points=[a])], ko)


def case_snapback(n=9):
    """Black throws a stone in at (1,0), White takes it from the corner, Black plays (1,0) again and takes five (a capture in the corner and on the edge)"""
    white = [at(n, 0, 1), at(n, 1, 1), at(n, 2, 1), at(n, 2, 0)]
    black = [at(n, 0, 2), at(n, 1, 2), at(n, 2, 2), at(n, 3, 1), at(n, 3, 0)]
    t, u = at(n, 1, 0), at(n, 0, 0)
    acts = tempo(n, black, white, [(1, t), (2, u), (1, t)])
    return _case(n, acts, [dict(move=len(acts) - 2, captured=1, groups=1, points=[t]), dict(move=len(acts) - 1, captured=5, groups=1, points=white + [u])])


def case_capture_chain(n, chain, colour=2):
    """a chain of `colour` is surrounded and taken by the last stone of its border"""
    other = border(n, chain)
    black, white = (other, list(chain)) if colour == 2 else (list(chain), other)
    acts = tempo(n, black, white)
    assert acts[-1] == other[-1]
    return _case(n, acts, [dict(move=len(acts) - 1, captured=len(chain), groups=1, points=list(chain))])


def case_corner(n, corner):
    """a single stone taken in a corner: 0 = the origin, 1 = the last point of the board (point 63 on 8x8)"""
    return case_capture_chain(n, [0 if corner == 0 else n * n - 1])


def case_edge(n=9):
    return case_capture_chain(n, [at(n, 4, 0), at(n, 5, 0)])


def case_boundary_capture(n, p, colour=2):
    """the captured chain holds both p and p + 1 (the last point of one 64-point word of the device's bitboards and the first of the next) and one more on either side"""
    assert (p + 1) % n != 0
    chain = [q for q in (p - 1, p, p + 1, p + 2) if q // n == p // n]
    return case_capture_chain(n, chain, colour)


def case_boundary_merge(n, p, play_low):
    """Black joins two stones through p or p + 1: the merged chain holds both points of the word boundary"""
    a, others = (p, [p + 1, p - n]) if play_low else (p + 1, [p, p + 1 + n])
    white = [at(n, 0, 0)] if p > 3 * n else [n * n - 1]
    acts = tempo(n, others, white, [(1, a)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=0, groups=0, points=[], merged=2, chain=others + [a])])


def case_big_capture(n=19, rows=4, hole=(9, 1)):
    """White fills rows 0 .. rows - 1 except one point, Black the row above and then that point: one capture of rows * n - 1 stones (75 on 19x19: more than a
    64-point word, spanning two); Black passes, never twice in a row, while White fills"""
    h = at(n, *hole)
    white = [p for p in range(rows * n) if p != h]
    black = [at(n, x, rows) for x in range(n)]
    acts = tempo(n, black, white, [(1, h)])
    return _case(n, acts, [dict(move=len(acts) - 1, captured=len(white), groups=1, points=white)])


@functools.lru_cache(None)
def case_move_cap(n, ko="positional"):
    """a random game that runs into the cap of 2 * n * n + 1 moves; the targets are its last positions, the one after the last move included"""
    for seed in range(200):
        acts = playout(n, 1000 * n + seed, pass_prob=0.0, ko=ko)
        if len(acts) == 2 * n * n + 1:
            size = len(acts)
            return n, acts, [size - 3, size - 2, size - 1, size], {"ko": ko, "events": [], "length": size, "captures_at_least": 1}
    raise AssertionError("no seed reaches the move cap")


@functools.lru_cache(None)
def case_passes(n=9):
    """single passes in the middle, two passes at the end"""
    for seed in range(200):
        acts = playout(n, 77 + seed, max_moves=60, pass_prob=0.15)
        mid = [i for i, a in enumerate(acts[:-2]) if a == n * n]
        if len(acts) == 60 and len(mid) >= 3 and capture_moves(n, acts):
            targets = sorted({k for i in mid for k in (i + 1, i + 2)} | {58, 59, 60})
            return n, acts, targets, {"ko": "positional", "events": [], "length": 60, "single_passes": mid, "ends_with_two_passes": True}
    raise AssertionError("no seed qualifies")


BOUNDARIES = {19: [63, 127, 191, 255, 319], 13: [63, 127]}


def hand_cases():
    """name -> (n, actions, target_positions, claim)"""
    out = {}
    for k in (1, 2, 3, 4):
        out[f"capture_{k}_groups"] = case_capture_groups(k)
    out["capture_4_groups_19"] = case_capture_groups(4, 19, 3, 3)  # around point 60: the four stones lie in word 0 and word 1 (points 41, 59, 61, 79)
    out["same_group_twice_captured"] = case_same_group_twice(True)
    out["same_group_twice_alive"] = case_same_group_twice(False)
    for k in (2, 3, 4):
        out[f"merge_{k}_groups"] = case_merge_groups(k)
    out["merge_4_groups_19"] = case_merge_groups(4, 19, 7, 3)  # around point 64
    out["merge_and_capture"] = case_merge_and_capture()
    out["ko"] = case_ko()
    out["ko_situational"] = case_ko(ko="situational")
    out["ko_5"] = case_ko(5, ox=0, oy=1)
    out["snapback"] = case_snapback()
    out["snapback_5"] = case_snapback(5)
    out["corner"] = case_corner(9, 0)
    out["far_corner"] = case_corner(9, 1)
    out["edge"] = case_edge()
    out["point_63_of_8x8"] = case_corner(8, 1)
    out["row_7_of_8x8"] = case_capture_chain(8, [60, 61, 62, 63])
    for n, ps in BOUNDARIES.items():
        for p in ps:
            out[f"capture_{p}_{p + 1}_on_{n}"] = case_boundary_capture(n, p)
            out[f"merge_{p}_{p + 1}_on_{n}_low"] = case_boundary_merge(n, p, True)
            out[f"merge_{p}_{p + 1}_on_{n}_high"] = case_boundary_merge(n, p, False)
    out["capture_black_63_64_on_19"] = case_boundary_capture(19, 63, colour=1)
    out["capture_75_stones"] = case_big_capture()
    for n in (5, 9, 19):
        out[f"move_cap_{n}"] = case_move_cap(n)
    out["passes"] = case_passes()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the window of positions the one-wave replay keeps (loader_kernels.hip: keep = 8)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
WINDOW_SIZES = (5, 8, 9, 13, 19)
WINDOW_LENGTH = 32


@functools.lru_cache(None)
def window_game(n):
    """a playout of WINDOW_LENGTH moves with at least two captures inside its first 12 moves (the first seed that qualifies), ended by two passes"""
    for seed in range(500):
        acts = playout(n, 31 * n + seed, max_moves=WINDOW_LENGTH, region=(12, 3))
        if len(acts) == WINDOW_LENGTH and len(capture_moves(n, acts, 12)) >= 2:
            return acts
    raise AssertionError("no seed qualifies")


def window_positions(size):
    return [0, 1, 2, 7, 8, 9, 10, size - 1, size]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# records with a move the rules refuse
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _sending_two_returning_one(n=5):
    """Black adds a stone in the corner (two stones, one liberty), White takes both, Black takes the taking stone back: the position before Black's first
    move again, now with White to move — a repeat that positional superko forbids and situational superko allows"""
    acts = [at(n, 1, 0), at(n, 0, 1), at(n, 3, 0), at(n, 1, 1), at(n, 2, 1), at(n, 4, 4)]
    return acts + [at(n, 0, 0), at(n, 2, 0), at(n, 1, 0), at(n, 3, 4), at(n, 4, 3)], 8


def _othello_prefix(n, seed, want):
    """a random legal Othello prefix after which `want(env)` gives an illegal action"""
    for s in range(seed, seed + 200):
        acts = playout(n, s, max_moves=int(np.random.default_rng(s).integers(2, 7)), game="othello", end_with_passes=False)
        env = oracle_lib.OracleEnv(game_conf("othello", n))
        for a in acts:
            env.act(a)
        bad = want(env)
        if bad is not None and not env.is_terminal():
            return acts, bad
    raise AssertionError("no seed qualifies")


def illegal_records():
    """name -> dict(game, n, ko, actions, move (index of the first move the rules refuse), legal (False; True = the rules take every move), claim)"""
    out = {}

    def add(name, game, n, actions, move, claim, ko="positional", legal=False):
        out[name] = dict(game=game, n=n, ko=ko, actions=list(actions), move=move, legal=legal, claim=claim)

    add("go_own_stone", "go", 5, [12, 7, 12, 8, 13], 2, "Black plays on Black's stone at 12: refused, the turn stays with Black")
    add("go_enemy_stone", "go", 5, [12, 12, 7, 8], 1, "White plays on Black's stone at 12: refused; a parity replay turns 12 white")
    add("go_suicide_single", "go", 5, [1, 24, 5, 0, 12, 13], 3, "White plays the corner between Black's 1 and 5 and takes nothing: refused")
    add("go_suicide_group", "go", 5, [2, 0, 5, 24, 6, 1, 12, 13], 5, "White's 1 would join the corner stone into a group of two without a liberty: refused")
    ko_acts, a, b = ko_shape(5, 0, 1)
    for rule in ("positional", "situational"):
        add(f"go_ko_retake_{rule}", "go", 5, ko_acts + [b, 24, 0], len(ko_acts), "Black retakes the ko at once: the position after Black's earlier stone on the same point, refused under both superko rules", ko=rule)
    s2r1, m = _sending_two_returning_one()
    add("go_repeat_positional", "go", 5, s2r1, m, "sending two, returning one: move 8 repeats the position before move 6 with the other player to move: refused under positional superko", ko="positional")
    add("go_repeat_situational", "go", 5, s2r1, m, "the same record under situational superko: the player to move differs, every move is legal", ko="situational", legal=True)
    add("go_move_after_two_passes", "go", 5, [12, 25, 25, 7, 8], 3,
        "a stone after two passes: act() does not look at isTerminal() (go.cpp:132-190 tests isLegalAction alone), the move is played: a legal record for the replay", legal=True)
    acts, bad = _othello_prefix(6, 3, lambda env: next((int(p) for p in range(36) if not env.legal_mask()[p] and not any(x[p] for x in go_board(env, 6))), None))
    add("othello_no_flip", "othello", 6, acts + [bad], len(acts), "an empty point that flips nothing: refused")
    acts, bad = _othello_prefix(4, 11, lambda env: 16 if env.legal_mask()[:16].any() else None)
    add("othello_pass_with_moves", "othello", 4, acts + [bad], len(acts), "a pass while a move exists: refused")
    add("tictactoe_occupied", "tictactoe", 3, [4, 4, 0], 1, "the centre twice: refused")
    add("gomoku_occupied", "gomoku", 9, [40, 41, 40, 3], 2, "a stone on a stone (no move of Gomoku removes one): refused")
    add("hex_occupied", "hex", 5, [12, 7, 12, 3], 2, "a stone on a stone, not the swap (which is the second move on the first move's point): refused")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# a replay that takes the stone's colour from the move index and tests nothing (what a device replay without a legality test computes)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def parity_planes(game, n, actions, pos):
    """unrotated planes of position `pos` in the layout of the engines' getFeatures: Go 8 x (to move, other) + 2 colour planes, the other games 2 + 2"""
    P = n * n
    board = np.zeros(P, np.int8)
    if game == "othello":
        h = n // 2
        board[at(n, h - 1, h - 1)] = board[at(n, h, h)] = 1
        board[at(n, h, h - 1)] = board[at(n, h - 1, h)] = 2
    hist = []
    for i, a in enumerate(actions[:pos]):
        m = 1 + (i & 1)
        if a < P:
            board[a] = m
            if game == "go":
                for q in neighbours(n, a):
                    if board[q] == 3 - m:
                        grp, libs = _group(n, board, q)
                        if not libs:
                            board[grp] = 0
            elif game == "othello":
                for dx, dy in ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)):
                    x, y, run = a % n + dx, a // n + dy, []
                    while 0 <= x < n and 0 <= y < n and board[at(n, x, y)] == 3 - m:
                        run.append(at(n, x, y))
                        x, y = x + dx, y + dy
                    if run and 0 <= x < n and 0 <= y < n and board[at(n, x, y)] == m:
                        board[run] = m
        hist.append(board.copy())
    turn = 1 + (pos & 1)
    planes = []
    if game == "go":
        for k in range(8):
            b = hist[len(hist) - 1 - k] if len(hist) - 1 - k >= 0 else np.zeros(P, np.int8)
            planes += [b == turn, b == 3 - turn]
    else:
        planes += [board == turn, board == 3 - turn]
    planes += [np.full(P, turn == 1), np.full(P, turn == 2)]
    return np.array(planes, np.float32).reshape(-1)


def _group(n, board, start):
    grp, libs, todo = [start], set(), [start]
    seen = {start}
    while todo:
        p = todo.pop()
        for q in neighbours(n, p):
            if board[q] == 0:
                libs.add(q)
            elif board[q] == board[start] and q not in seen:
                seen.add(q)
                grp.append(q)
                todo.append(q)
    return grp, libs


def groups_of(n, mask):
    """connected components of the points set in a boolean board"""
    board = mask.astype(np.int8)
    left, out = set(np.nonzero(mask)[0].tolist()), []
    while left:
        grp, _ = _group(n, board, next(iter(left)))
        out.append(sorted(grp))
        left -= set(grp)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests load: name -> Batch.  The CPU test proves with the oracle's loader alone that every target (game, position) is sampled.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Batch:
    """records of one loader configuration: `games` = [(actions, (first, last) sampled position)], every position of the ranges being a target"""

    def __init__(self, n, games, batch_size, seed, batches=3, ko="positional", game="go", extra="", reward=False):
        self.n, self.games, self.batches, self.game, self.ko = n, games, batches, game, ko
        self.conf = game_conf(game, n, ko)
        self.lconf = f"{self.conf}{extra}:learner_batch_size={batch_size}:program_seed={seed}"
        self.records = [record(n, a, d, game, reward) for a, d in games]
        self.targets = {(g, k) for g, (a, d) in enumerate(games) for k in range(d[0], d[1] + 1)}


def _spans(targets):
    """the target positions as the record's one DLEN range"""
    return (min(targets), max(targets))


@functools.lru_cache(None)
def batches():
    out = {}
    by_board = {}
    for name, (n, acts, targets, claim) in hand_cases().items():
        by_board.setdefault((n, claim["ko"]), []).append((acts, _spans(targets)))
    for (n, ko), games in sorted(by_board.items()):
        out[f"hand_{n}_{ko}"] = Batch(n, games, HAND_BATCH[(n, ko)][0], HAND_BATCH[(n, ko)][1], ko=ko)
    for n in WINDOW_SIZES:
        acts = window_game(n)
        out[f"window_{n}"] = Batch(n, [(acts, (k, k)) for k in window_positions(len(acts))], 32, WINDOW_SEED[n], batches=2)
    # MuZero: games longer than n * n moves, sampled within 5 moves of their end: the 5 unrolled steps pass the end of the game and draw random action planes
    # (go.cpp:725-737: randInt() % (n * n + 1); the draw n * n leaves the plane empty)
    for n in (5, 7):
        games = []
        for ko in ("positional",):
            acts = case_move_cap(n, ko)[1]
            games += [(acts, (len(acts) - 5, len(acts))), (acts[:n * n + 6], (n * n + 1, n * n + 6))]
        out[f"muzero_{n}"] = Batch(n, games, 64, MUZERO_SEED[n], extra=":nn_type_name=muzero:learner_muzero_unrolling_step=5", reward=True)
    return out


# (learner_batch_size, program_seed) per board: the first seed with which three batches of the oracle's sampler meet every target (tests/test_loader_cases.py asserts it)
HAND_BATCH = {(5, "positional"): (64, 1), (8, "positional"): (32, 1), (9, "positional"): (128, 5), (9, "situational"): (32, 1), (13, "positional"): (64, 1), (19, "positional"): (128, 1)}
WINDOW_SEED = {5: 1, 8: 1, 9: 1, 13: 1, 19: 1}
MUZERO_SEED = {5: 1, 7: 1}


def sample_buffers(B, shapes):
    nf, na, npol, nv, nr = shapes
    return [np.zeros((B, max(k, 1)), np.float32) for k in (nf, na, npol, nv, nr)] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]


def oracle_sampled(batch, shapes=None):
    """(the set of (game, position) the oracle's loader samples over the batches of a Batch, the sampled arrays of every batch)"""
    ol = oracle_lib.OracleLoader(batch.lconf)
    for r in batch.records:
        assert ol.add_record(r) == 1
    ol.finish()
    B = int(batch.lconf.split("learner_batch_size=")[1].split(":")[0])
    P = batch.n * batch.n
    U = int(batch.lconf.split("learner_muzero_unrolling_step=")[1].split(":")[0]) if "muzero" in batch.lconf else 0
    shapes = shapes or ((18 if batch.game == "go" else 4) * P, U * P, (U + 1) * (P + 1), U + 1, U)
    seen, out = set(), []
    for _ in range(batch.batches):
        bufs = sample_buffers(B, shapes)
        ol.sample_data(*bufs)
        seen |= {(int(g), int(k)) for g, k in bufs[6]}
        out.append(bufs)
    return seen, out
