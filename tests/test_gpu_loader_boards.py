"""GPU tests of the learner-side sampler's own Go replay (loader_kernels.hip goReplayMoves) beyond 9x9 self-play records: random legal playouts on boards of
every bitboard width (1 .. 6 words of 64 points), the hand-built games and window records of tests/loader_cases.py (whose claims tests/test_loader_cases.py
proves on the CPU), regrowth of the device buffers, eviction, MuZero's unrolled steps past the end of a game, small Othello boards, and records with a move
the rules refuse.  Everything is bit for bit against the oracle's loader with the same seed; the hand-built and window cases also against the product's
host engine (a reference that shares no loader code)."""
import numpy as np
import pytest

import loader_cases as lc
from test_gpu_loader import _compare

pytestmark = pytest.mark.gpu

NAMES = ["features", "action_features", "policy", "value", "reward", "loss_scale", "sampled_index"]


def _line(rec):
    """a bare record as the `SelfPlay ... #` line test_gpu_loader._compare takes apart again"""
    return f"SelfPlay 1 0 0 1 {rec} #"


def _same(mine, theirs, tag):
    for name, a, b in zip(NAMES, mine, theirs):
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), f"{tag}: {name} differs in {int((~same).sum())} of {same.size} values (first sample {int(np.argwhere(~same)[0][0])})"


def _sample_both(dl, ol, tag):
    B, *shapes = dl.shapes()
    mine, theirs = lc.sample_buffers(B, shapes), lc.sample_buffers(B, shapes)
    dl.sample_data(*mine)
    ol.sample_data(*theirs)
    _same(mine, theirs, tag)
    return mine


def _host_engine_agrees(mz, conf, games, mine, cache):
    """every sample's planes are the host engine's planes of actions[:position] under exactly one of the 8 rotations (at least one where the position is symmetric)"""
    for feats, (g, k) in zip(mine[0], mine[6]):
        key = (int(g), int(k))
        if key not in cache:
            env = mz.Env(conf)
            for i, a in enumerate(games[key[0]][:key[1]]):
                assert env.act(a, 1 + (i & 1)), f"game {key[0]}: the host engine refuses move {i}"
            cache[key] = [env.features(r) for r in range(8)]
        rots = [r for r in range(8) if np.array_equal(feats, cache[key][r])]
        distinct = len({f.tobytes() for f in cache[key]})
        assert rots, f"(game {key[0]}, position {key[1]}) is no rotation of the host engine's planes"
        assert len(rots) == 1 or distinct < 8, f"(game {key[0]}, position {key[1]}) matches rotations {rots} of an asymmetric position"


# n -> (ko rule, batch size, how the records go in); 2 .. 8: one word per colour (8x8: exactly 64 points), 11: two, 12 / 13: three, 16 / 17: four / five, 19: six
PLAYOUTS = [(2, "positional", 32), (3, "positional", 32), (5, "positional", 64), (5, "situational", 64), (7, "positional", 64), (8, "positional", 64),
            (9, "positional", 64), (9, "situational", 64), (11, "positional", 64), (12, "positional", 48), (13, "positional", 48), (16, "positional", 32),
            (17, "positional", 32), (19, "positional", 32)]


@pytest.mark.parametrize("n,ko,B", PLAYOUTS)
def test_random_playouts_match_the_oracle(mz, oracle, tmp_path, n, ko, B):
    """2 - 4 random legal games per board (one to its natural end, the others cut short with single passes and ended by two), the whole data range, three batches"""
    P = n * n
    games = [lc.playout(n, 100 * n + 1, ko=ko), lc.playout(n, 100 * n + 2, max_moves=max(6, P), pass_prob=0.08, ko=ko), lc.playout(n, 100 * n + 3, max_moves=max(4, P // 2), pass_prob=0.02, ko=ko)]
    if n <= 9:
        games.append(lc.playout(n, 100 * n + 4, pass_prob=0.05, ko=ko))
    lines = [_line(lc.record(n, a)) for a in games]
    lconf = f"{lc.go_conf(n, ko)}:learner_batch_size={B}:program_seed={n + 3}"
    _compare(mz, oracle, lconf, lines, tmp_path, batches=3, as_file=(n == 13))


@pytest.mark.parametrize("name", sorted(lc.batches()))
def test_hand_built_and_window_records(mz, oracle, tmp_path, name):
    """the records of tests/loader_cases.py: every target (game, position) is drawn by the product's own sampler too, every array equals the oracle's, and the planes
    equal the host engine's"""
    b = lc.batches()[name]
    dl, ol, out = _compare(mz, oracle, b.lconf, [_line(r) for r in b.records], tmp_path, batches=b.batches, as_file=False)
    seen = {(int(g), int(k)) for mine, _ in out for g, k in mine[6]}
    assert b.targets <= seen, f"never sampled: {sorted(b.targets - seen)}"
    cache = {}
    for mine, _ in out:
        _host_engine_agrees(mz, b.conf, [a for a, _ in b.games], mine, cache)


def test_longer_record_regrows_the_device_buffers(mz, oracle):
    """a batch from short games, then a record longer than any so far (more position slots per sample: the device side is allocated again), then another batch"""
    n, lconf = 9, lc.go_conf(9) + ":learner_batch_size=32:program_seed=6"
    dl, ol = mz.DataLoader(lconf), oracle.OracleLoader(lconf)

    def add(actions):
        r = lc.record(n, actions)
        assert dl.add_record(r) == 1 and ol.add_record(r) == 1
        ol.finish()

    for seed in (1, 2, 3):
        add(lc.playout(n, seed, max_moves=20))
    _sample_both(dl, ol, "short games")
    long_game = lc.playout(n, 4, max_moves=130, pass_prob=0.03)
    assert len(long_game) == 130
    add(long_game)
    assert dl.num_games() == ol.num_games() == 4 and dl.num_data() == ol.num_data()
    for it in range(3):
        mine = _sample_both(dl, ol, f"after the long game, batch {it}")
    assert any(g == 3 and k > 22 for g, k in mine[6]), "a position of the long game past the old slot count"
    add(lc.playout(n, 5))  # ... and once more, to the move cap or the game's natural end
    _sample_both(dl, ol, "after the longest game")


def test_eviction_keeps_the_newest_games(mz, oracle):
    n, lconf = 7, lc.go_conf(7) + ":zero_replay_buffer=1:zero_num_games_per_iteration=3:learner_batch_size=48:program_seed=8"
    dl, ol = mz.DataLoader(lconf), oracle.OracleLoader(lconf)
    for seed in range(5):
        r = lc.record(n, lc.playout(n, 40 + seed, max_moves=20 + 9 * seed, pass_prob=0.05))
        assert dl.add_record(r) == 1 and ol.add_record(r) == 1
        ol.finish()
        assert dl.num_games() == ol.num_games() == min(seed + 1, 3) and dl.num_data() == ol.num_data()
    for it in range(2):
        _sample_both(dl, ol, f"batch {it}")


@pytest.mark.parametrize("n", [4, 6])
def test_small_othello_boards(mz, oracle, tmp_path, n):
    P = n * n
    games = [lc.playout(n, 10 * n + s, game="othello") for s in range(12)]
    forced = [a for a in games if any(x == P and y != P for x, y in zip(a[:-2], a[1:-1]))]
    assert forced, "no game with a forced pass in the middle"
    games = forced[:1] + [a for a in games if a is not forced[0]][:3]
    lconf = f"env_game=othello:env_board_size={n}:learner_batch_size=64:program_seed={n}"
    _compare(mz, oracle, lconf, [_line(lc.record(n, a, game="othello")) for a in games], tmp_path, batches=3, as_file=False)


REASONS = ("occupied point", "suicide or repeated position", "flips no stone", "pass while a move exists", "not allowed by the rules")


@pytest.mark.parametrize("name", sorted(lc.illegal_records()))
def test_records_with_a_refused_move(mz, oracle, name):
    """a record with a move the rules refuse either samples exactly what the oracle samples (whose replay skips the move) or is refused with the move's index and
    the reason; one that loads and gives other planes is the failure.  After a refusal the loader samples its legal records like a loader that never saw the other."""
    r = lc.illegal_records()[name]
    game, n = r["game"], r["n"]
    conf = lc.game_conf(game, n, r["ko"])
    lconf = f"{conf}:learner_batch_size=32:program_seed=3"
    legal = r["actions"][:r["move"]] if game != "go" else lc.playout(n, 9, max_moves=14, ko=r["ko"])
    first, bad = lc.record(n, legal, game=game), lc.record(n, r["actions"], game=game)
    dl = mz.DataLoader(lconf)
    assert dl.add_record(first) == 1
    rc = dl.add_record(bad)
    assert rc in (0, 1)
    if r["legal"]:
        assert rc == 1, f"every move of this record is legal ({r['claim']}): {mz.last_error()}"
    if rc == 0:
        err = mz.last_error()
        assert f"move {r['move']} " in err and any(why in err for why in REASONS), err
        assert dl.num_games() == 1
    kept = [legal] + ([r["actions"]] if rc == 1 else [])
    if game in ("gomoku", "hex"):  # (no oracle for these games: the host engine is the reference, and its replay refuses the move)
        assert rc == 0, "a stone on a stone was loaded"
        B, *shapes = dl.shapes()
        mine = lc.sample_buffers(B, shapes)
        dl.sample_data(*mine)
        _host_engine_agrees(mz, conf, kept, mine, {})
        return
    ol = oracle.OracleLoader(lconf)
    assert ol.add_record(first) == 1 and (rc == 0 or ol.add_record(bad) == 1)
    ol.finish()
    assert dl.num_data() == ol.num_data()
    for it in range(2):
        mine = _sample_both(dl, ol, f"batch {it}")
    if rc == 1:
        assert any(g == 1 and k > r["move"] for g, k in mine[6]) or r["legal"], "no sample past the refused move"
