"""The records of tests/loader_cases.py are what they claim to be — checked with the oracle's rules engine and the oracle's loader alone (no GPU, no product
code): every hand-built capture / merge / ko claim, the window games' early captures, every illegal record's refused move, and that the sampler
configurations the GPU tests use (tests/test_gpu_loader_boards.py) really draw every target (game, position)."""
import numpy as np
import pytest

import loader_cases as lc

HAND = lc.hand_cases()
ILLEGAL = lc.illegal_records()


def _replay(n, actions, ko, game="go"):
    """[(black, white)] per position, [accepted] per move, [planes] per position on the oracle's engine with the recorded colours"""
    import oracle_lib
    env = oracle_lib.OracleEnv(lc.game_conf(game, n, ko))
    boards, ok, planes = [lc.go_board(env, n)], [], [env.features(0)]
    for i, a in enumerate(actions):
        ok.append(env.act(a, 1 + (i & 1)))
        boards.append(lc.go_board(env, n))
        planes.append(env.features(0))
    return boards, ok, planes


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_claims_hold_on_the_oracle(oracle, name):
    n, actions, targets, claim = HAND[name]
    P = n * n
    boards, ok, planes = _replay(n, actions, claim["ko"])
    assert all(ok), f"move {ok.index(False)} is illegal"
    assert len(actions) <= 2 * P + 1 and targets and all(0 <= k <= len(actions) for k in targets)
    assert not any(a == P and b == P for a, b in zip(actions[:-1], actions[1:-1])), "two passes in a row before the end"
    for e in claim["events"]:
        i = e["move"]
        a, m = actions[i], i & 1  # m: index of the mover in (black, white)
        before, after = boards[i], boards[i + 1]
        assert a < P and after[m][a] and int(after[m].sum()) == int(before[m].sum()) + 1, "the mover gains exactly the stone played"
        removed = before[1 - m] & ~after[1 - m]
        assert int(removed.sum()) == e["captured"] and int(after[1 - m].sum()) == int(before[1 - m].sum()) - e["captured"]
        assert all(removed[p] for p in e["points"]) and len(lc.groups_of(n, removed)) == e["groups"]
        touched = {tuple(g) for g in lc.groups_of(n, before[1 - m]) if any(q in g for q in lc.neighbours(n, a))}
        assert len(touched) >= e["groups"]
        if name.startswith("same_group_twice"):
            assert len(touched) == 1 and sum(before[1 - m][q] for q in lc.neighbours(n, a)) == 2, "one enemy group on two sides of the move"
        if "merged" in e:
            own = {tuple(g) for g in lc.groups_of(n, before[m]) if any(q in g for q in lc.neighbours(n, a))}
            assert len(own) == e["merged"]
            chain = [g for g in lc.groups_of(n, after[m]) if a in g][0]
            assert set(e["chain"]) <= set(chain)
        assert {i + 1, i + 2, i + 3} <= set(targets), "sampled just after the move and where the one-wave replay has made it"
    if "length" in claim:
        assert len(actions) == claim["length"]
    for k in targets:  # a replay that only alternates colours computes the same planes on a legal record
        assert np.array_equal(lc.parity_planes("go", n, actions, k), planes[k]), f"position {k}"


def test_boundary_cases_hold_both_points_of_every_word_boundary():
    for n, ps in lc.BOUNDARIES.items():
        for p in ps:
            assert p % 64 == 63 and p // n == (p + 1) // n
            e = HAND[f"capture_{p}_{p + 1}_on_{n}"][3]["events"][0]
            assert {p, p + 1} <= set(e["points"])
            for side in ("low", "high"):
                e = HAND[f"merge_{p}_{p + 1}_on_{n}_{side}"][3]["events"][0]
                assert {p, p + 1} <= set(e["chain"]) | {HAND[f"merge_{p}_{p + 1}_on_{n}_{side}"][1][e["move"]]}
    e = HAND["capture_75_stones"][3]["events"][0]
    assert e["captured"] == 75 > 64 and {0, 63, 64, 75} <= set(e["points"])
    assert 63 in HAND["point_63_of_8x8"][3]["events"][0]["points"] and 63 in HAND["row_7_of_8x8"][3]["events"][0]["points"]
    assert [HAND[f"capture_{k}_groups"][3]["events"][0]["groups"] for k in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [HAND[f"merge_{k}_groups"][3]["events"][0]["merged"] for k in (2, 3, 4)] == [2, 3, 4]


def test_move_cap_and_pass_games(oracle):
    for n in (5, 9, 19):
        _, actions, targets, claim = HAND[f"move_cap_{n}"]
        assert len(actions) == 2 * n * n + 1 and targets[-1] == len(actions) and len(lc.capture_moves(n, actions)) >= 3
        env = oracle.OracleEnv(lc.go_conf(n))
        for a in actions[:-1]:
            assert env.act(a)
        assert not env.is_terminal() and env.act(actions[-1]) and env.is_terminal(), "the last move is the one that reaches the cap"
    n, actions, targets, claim = HAND["passes"]
    P = n * n
    assert actions[-2:] == [P, P] and actions[-3] != P and len(claim["single_passes"]) >= 3
    assert all(actions[i] == P and actions[i + 1] != P and actions[i - 1] != P for i in claim["single_passes"])


@pytest.mark.parametrize("n", lc.WINDOW_SIZES)
def test_window_games_capture_early(oracle, n):
    actions = lc.window_game(n)
    assert len(actions) == lc.WINDOW_LENGTH and actions[-2:] == [n * n, n * n]
    assert len(lc.capture_moves(n, actions, 12)) >= 2, "captures inside the first 12 moves: before, at and past the 8 kept positions"
    b = lc.batches()[f"window_{n}"]
    assert sorted(k for _, k in b.targets) == [0, 1, 2, 7, 8, 9, 10, len(actions) - 1, len(actions)]


@pytest.mark.parametrize("name", sorted(ILLEGAL))
def test_illegal_records_hold_a_refused_move(oracle, name):
    r = ILLEGAL[name]
    game, n, actions, i = r["game"], r["n"], r["actions"], r["move"]
    if game in ("gomoku", "hex"):  # (no oracle engine: no move of these games removes a stone, so a point played twice is occupied the second time)
        assert actions[i] in actions[:i] and not (game == "hex" and i == 1)
        assert not np.array_equal(lc.parity_planes(game, n, actions, i + 1), lc.parity_planes(game, n, actions[:i] + actions[i + 1:], i))
        return
    boards, ok, planes = _replay(n, actions, r["ko"], game)
    if r["legal"]:
        assert all(ok), r["claim"]
        for k in range(len(actions) + 1):
            assert np.array_equal(lc.parity_planes(game, n, actions, k), planes[k]), f"position {k}"
        return
    assert ok.index(False) == i, r["claim"]
    assert np.array_equal(planes[i], planes[i + 1]), "the refused move leaves the position alone, the turn included"
    for k in range(i + 1):
        assert np.array_equal(lc.parity_planes(game, n, actions, k), planes[k]), f"position {k}: the record is legal up to the refused move"
    for k in range(i + 1, len(actions) + 1):
        assert not np.array_equal(lc.parity_planes(game, n, actions, k), planes[k]), f"position {k}: a replay without a legality test gives the same planes"


def test_the_two_superko_rules_differ_on_the_repeat(oracle):
    a, b = ILLEGAL["go_repeat_positional"], ILLEGAL["go_repeat_situational"]
    assert a["actions"] == b["actions"] and (a["ko"], b["ko"]) == ("positional", "situational") and not a["legal"] and b["legal"]
    boards, ok, _ = _replay(5, a["actions"], "situational")
    i = a["move"]
    assert all(np.array_equal(x, y) for x, y in zip(boards[i + 1], boards[i - 2])), "the position before Black's corner stone, three moves later: the other player is to move"


def test_othello_parity_replay_is_the_oracle_on_legal_games(oracle):
    for n, seed in ((4, 1), (6, 2)):
        actions = lc.playout(n, seed, game="othello")
        _, ok, planes = _replay(n, actions, "positional", "othello")
        assert all(ok)
        for k in range(len(actions) + 1):
            assert np.array_equal(lc.parity_planes("othello", n, actions, k), planes[k])


@pytest.mark.parametrize("name", sorted(lc.batches()))
def test_the_oracle_sampler_draws_every_target(oracle, name):
    b = lc.batches()[name]
    seen, out = lc.oracle_sampled(b)
    assert b.targets <= seen, f"never sampled: {sorted(b.targets - seen)}"
    assert int(b.lconf.split("learner_batch_size=")[1].split(":")[0]) <= 128
    if name.startswith("muzero"):  # the unrolled steps past the end of the game: random action planes, the empty one (the draw n * n) among them
        P, size = b.n * b.n, len(b.games[0][0])
        assert size > P
        empty = onehot = 0
        for bufs in out:
            for (g, k), af in zip(bufs[6], bufs[1].reshape(len(bufs[6]), 5, P)):
                for step in range(5):
                    if g == 0 and k + step >= size:
                        s = int(af[step].sum())
                        assert s in (0, 1)
                        empty, onehot = empty + (s == 0), onehot + (s == 1)
        assert empty >= 1 and onehot >= 10, (empty, onehot)
