"""tests/match_model.py on the CPU: the schedule of a match pinned by literals worked out by hand, match_elo pinned by literals, and for every row that
tests/test_gpu_match.py runs against the HIP worker the proof that its inputs can tell the right reading of the schedule from three wrong ones (the two
networks swapped, colour-blind restarts, one network for both sides): each must change at least one record.  The table of rows (ROWS) and the model's matches
are shared with tests/test_gpu_match.py.

The networks are f32 networks of the oracle's forward, which the device's f32 path equals bit for bit (tests/test_gpu_net.py); the rows reuse the
descriptors and weight seeds that tests/test_gpu_search_model.py and tests/test_gpu_think.py already hold to the search model exactly where those files
have two seeds for a descriptor, and every row — old seeds or new — is certified with tests/test_tree_model.py's margin condition or listed, with its
figure, in NO_MARGIN."""
import math

import pytest

import match_model as MM
import search_model as S
import test_search_model as T
import test_think_model as M
import tree_model as R

# ---------------------------------------------------------------------------------------------
# a. the schedule on scripted games, by hand.  G = 4: lane 0 = slots 0, 1, lane 1 = slots 2, 3; N = 6.  Games in the order they start, (length, score):
#   serial 0 slot 0 t0 0 length 3 -> last move in step 2     first player (0 + 0) mod 2 = A
#   serial 1 slot 1 t0 0 length 2 -> step 1                  A
#   serial 2 slot 2 t0 0 length 4 -> step 3                  (1 + 0) mod 2 = B
#   serial 3 slot 3 t0 0 length 3 -> step 2                  B
#   after step 1: slot 1 is free, 4 < 6 started  -> serial 4, t0 2, first (0 + 2) mod 2 = A: an EVEN length keeps the first player; length 2 -> step 3
#   after step 2: slot 0 -> serial 5, t0 3, first (0 + 3) mod 2 = B: an ODD length hands the first move over; length 3 -> step 5
#                 slot 3 -> 6 have started: filler, t0 3 (first (1 + 3) mod 2 = A), length 5
#   after step 3: slot 1 (serial 4) and slot 2 (serial 2) end: fillers, t0 4
#   after step 5: serial 5 ends: the sixth counted game -> the match is over, 6 steps; slot 0 has been handed its next game, a fourth filler
# lines leave in the order 1 | 0, 3 | 4, 2 | 5.  Scores: 0: +1 (A wins as first), 1: 0, 2: +1 (B started: A loses as second), 3: -1 (A wins as second),
# 4: -1 (A loses as first), 5: 0 (draw, A second).  Moves of counted games: 3 + 2 + 4 + 3 + 2 + 3 = 17.
# ---------------------------------------------------------------------------------------------
HAND_GAMES = [(3, 1.0), (2, 0.0), (4, 1.0), (3, -1.0), (2, -1.0), (3, 0.0), (5, 0.0), (5, 0.0), (5, 0.0), (5, 0.0)]


def test_schedule_by_hand():
    sch = MM.run_schedule(4, 6, HAND_GAMES)
    assert [(f[0], f[1], MM.SIDES[f[2]], f[3], f[4]) for f in sch.finished] == [
        (1, 1, "A", 0, 1), (0, 0, "A", 0, 2), (3, 3, "B", 0, 2), (4, 1, "A", 2, 3), (2, 2, "B", 0, 3), (5, 0, "B", 3, 5)]
    assert sch.fillers == [(3, 3), (1, 4), (2, 4), (0, 6)]
    assert sch.stats == dict(games_started=6, games_finished=6, moves=17, filler_games=4, a_first=[1, 1, 1], a_second=[1, 1, 1], resignations=0, steps=6, done=True)


def test_schedule_lanes_share_their_side_to_move():
    """in every step of the hand case all games of a lane have side (h + t) mod 2 to move, and both sides search in every step"""
    sch = MM.Schedule(4, 6)
    it = iter(HAND_GAMES)
    for sl in sch.slots:
        sl.script = next(it)
    while not sch.stats["done"]:
        sides = [sch.side_to_move(sl) for sl in sch.slots]
        assert sides == [sch.t % 2, sch.t % 2, (1 + sch.t) % 2, (1 + sch.t) % 2]
        for sl in sch.end_step({sl.slot: (True, sch.t - sl.t0 + 1 == sl.script[0], sl.script[1], False) for sl in sch.slots}):
            sl.script = next(it)


def test_schedule_colour_blind_differs():
    """the wrong reading 'a restarted game always has A first' gives serial 5 (t0 3 in lane 0) to A, and its lane stops sharing its side to move"""
    sch = MM.run_schedule(4, 6, HAND_GAMES, colour_blind=True)
    assert [MM.SIDES[f[2]] for f in sch.finished] == ["A", "A", "B", "A", "B", "A"]


def test_schedule_smallest():
    """G = N = 2: one game per lane, no restart is counted; G odd or N < G is not a match"""
    sch = MM.run_schedule(2, 2, [(1, 1.0), (2, 1.0), (9, 0.0), (9, 0.0)])
    assert sch.stats["a_first"] == [1, 0, 0] and sch.stats["a_second"] == [0, 0, 1] and sch.stats["steps"] == 2 and sch.stats["filler_games"] == 2
    for G, N in ((3, 4), (0, 4), (4, 3)):
        with pytest.raises(AssertionError):
            MM.Schedule(G, N)


# ---------------------------------------------------------------------------------------------
# b. match_elo, by hand.  6 / 2 / 2: s = 0.7, elo = 400 log10(7 / 3) = 147.19; var = (6 * 0.09 + 2 * 0.04 + 2 * 0.49) / 10 = 0.16, se(s) = sqrt(0.016) =
# 0.126491, slope 400 / (ln 10 * 0.21) = 827.228 -> 104.64.  5 / 0 / 5: elo 0, var 0.25, se(s) = 0.158114, slope 400 / (ln 10 * 0.25) = 694.87 -> 109.87.
# ---------------------------------------------------------------------------------------------
def test_match_elo_by_hand():
    from minizero_amd.lib import match_elo
    e = match_elo(dict(a_first=[4, 1, 0], a_second=[2, 1, 2]))
    assert e["games"] == 10 and e["score"] == pytest.approx(0.7) and e["elo"] == pytest.approx(147.19, abs=0.01) and e["se"] == pytest.approx(104.64, abs=0.01)
    assert e["first"]["games"] == 5 and e["first"]["score"] == pytest.approx(0.9) and e["second"]["score"] == pytest.approx(0.5) and e["second"]["elo"] == 0.0
    e = match_elo(dict(a_first=[5, 0, 0], a_second=[0, 0, 5]))
    assert e["elo"] == 0.0 and e["se"] == pytest.approx(109.87, abs=0.01)
    assert e["first"]["elo"] == math.inf and e["second"]["elo"] == -math.inf and e["first"]["se"] == math.inf
    e = match_elo(dict(a_first=[0, 0, 0], a_second=[0, 4, 0]))
    assert math.isnan(e["first"]["elo"]) and e["first"]["games"] == 0 and e["elo"] == 0.0 and e["se"] == 0.0


# ---------------------------------------------------------------------------------------------
# c. the rows of tests/test_gpu_match.py: name -> (configuration, network, (weight seed of A, of B), G, N, steps compared or None for the whole match).
# The weight seeds are chosen here, on the CPU, with the model alone (pairs of seeds from 1 to 6 scanned in order): no AmbiguousOrder, the selection margin of
# tests/test_tree_model.py, the three wrong readings told apart, and — ttt, hex3_swap, ttt_mz — counted restarts after an odd and after an even number of steps.
# ---------------------------------------------------------------------------------------------
TTT2_MZ = M.TTT2[:12] + ("muzero",)
OTH4 = ("othello_4x4", 4, 4, 4, 8, 4, 4, 1, 1, 17, 16, 1, "alphazero")
HEX3 = ("hex_3x3", 4, 3, 3, 32, 3, 3, 1, 1, 9, 16, 1, "alphazero")
NO_RESIGN = ":actor_resign_threshold=-2"
ROWS = {
    "ttt": ("env_game=tictactoe:actor_num_simulation=8" + NO_RESIGN, M.TTT2, (1, 5), 4, 10, None),
    "hex3_swap": ("env_game=hex:env_board_size=3:actor_num_simulation=8" + NO_RESIGN, HEX3, (3, 2), 4, 10, None),
    "othello4_gumbel": ("env_game=othello:env_board_size=4" + T._gumbel(8, 4) + NO_RESIGN, OTH4, (2, 4), 4, 6, None),
    "ttt_mz": ("env_game=tictactoe:nn_type_name=muzero:actor_num_simulation=8" + NO_RESIGN, TTT2_MZ, (1, 2), 4, 10, None),
    # the settings of test_think_model's ttt_resign row: games that end by resignation
    "ttt_resign": (M.ROWS["ttt_resign"][0], M.TTT2, (5, 3), 4, 6, None),
    "ttt_n_equals_g": ("env_game=tictactoe:actor_num_simulation=8" + NO_RESIGN, M.TTT2, (1, 3), 2, 2, None),
    # the per-game simulation kernel of 9x9 Go: the first three moves of every slot (the networks and seeds of test_search_model's go_puct_n24)
    "go9": ("env_game=go:env_board_size=9:actor_num_simulation=12", T.GO8, (1, 2), 4, 4, 3),
}
WHOLE = [n for n, r in ROWS.items() if r[5] is None]
# rows whose margin (test_rows_have_their_selection_margin prints every figure) stays below tree_model.score_bound: none of them needs it — the model's
# networks are the oracle's f32 forward, which the device equals bit for bit — and they run under the same exact comparison
NO_MARGIN = ()

_CACHE = {}


def row_nets(oracle, name):
    _, desc_args, seeds = ROWS[name][:3]
    return tuple(M.row_net(oracle, desc_args, s) for s in seeds)


def row_weights(oracle, name):
    _, desc_args, seeds = ROWS[name][:3]
    return tuple(T.case_weights(oracle, desc_args, s) for s in seeds)


def row_model(oracle, name, reading="right"):
    """(lines, stats, slots, margins) of the model's match of a row under a reading of the schedule, computed once"""
    if (name, reading) not in _CACHE:
        conf, desc_args, seeds, G, N, steps = ROWS[name]
        cfg, muzero, _ = T.model_cfg(conf)
        nets = row_nets(oracle, name)
        kw = dict(swapped=reading == "swapped", colour_blind=reading == "colour_blind")
        if reading == "one_net":
            nets = (nets[0], nets[0])
        with R.Margins() as m:
            lines, stats, slots = MM.play_match(cfg, lambda: T.make_env(oracle, conf), nets, G, N, muzero=muzero, max_steps=steps, **kw)
        _CACHE[name, reading] = (lines, stats, slots, m)
    return _CACHE[name, reading]


def shown(model):
    """everything of a model's match that the GPU test compares"""
    lines, stats, slots, _ = model
    return ([(l["serial"], l["slot"], l["head"], l["PB"], l["PW"], l["moves"]) for l in lines], stats, [(s.serial, s.first, s.moves) for s in slots])


@pytest.mark.parametrize("name", list(ROWS))
def test_rows_tell_the_wrong_readings_apart(oracle, name):
    right = shown(row_model(oracle, name))
    for reading in ("swapped", "colour_blind", "one_net"):
        if reading == "colour_blind" and (ROWS[name][5] is not None or ROWS[name][4] == ROWS[name][3]):
            continue  # no counted restart in this row: nothing a colour rule could show
        wrong = shown(row_model(oracle, name, reading))
        records = lambda sh: ([x[3:] for x in sh[0]], [x[2] for x in sh[2]])  # (PB, PW, moves) of every line, the moves of every slot's running game
        assert records(wrong) != records(right), f"{name}: the reading '{reading}' plays the same records"


@pytest.mark.parametrize("name", [n for n in WHOLE if n != "ttt_n_equals_g"])
def test_whole_rows_show_the_schedule(oracle, name):
    """N is no multiple of G, at least one filler runs, and counted games restart in a slot after an odd and after an even length: the first move changes
    hands and stays"""
    lines, stats, _, _ = row_model(oracle, name)
    G, N = ROWS[name][3:5]
    assert N % G != 0 and stats["filler_games"] >= 1 and stats["games_finished"] == N == len(lines) and stats["done"]
    assert sum(stats["a_first"]) + sum(stats["a_second"]) == N
    by_slot = {}
    for l in lines:
        by_slot.setdefault(l["slot"], []).append(l)
    # (a game takes one step per move, and one more if it ends by resignation: the resigning side spends its step on it)
    steps_of = lambda l: len(l["moves"]) + (0 if "." in l["RE"] else 1)
    follow = [(steps_of(a) % 2, a["PB"] == b["PB"]) for ls in by_slot.values() for a, b in zip(ls, ls[1:]) if b["serial"] >= G]
    print(name, stats, follow)
    assert all(same == (parity == 0) for parity, same in follow)
    if name in ("ttt", "hex3_swap", "ttt_mz"):
        assert {p for p, _ in follow} == {0, 1}, f"{name}: restarts of both parities are what the row is for"


def test_resign_row_resigns_for_both_results(oracle):
    lines, stats, _, _ = row_model(oracle, "ttt_resign")
    print(stats, [(l["head"], l["PB"], l["RE"]) for l in lines])
    # every game of the row ends by resignation, some before their first move, and each side wins games by the other's: A loses as first, wins as second
    assert stats["resignations"] == ROWS["ttt_resign"][4] and stats["a_first"][2] > 0 and stats["a_second"][0] > 0
    assert {len(l["moves"]) for l in lines} >= {0} and any(l["moves"] for l in lines) and all("." not in l["RE"] for l in lines)


@pytest.mark.parametrize("name", list(ROWS))
def test_rows_have_their_selection_margin(oracle, name):
    cfg = T.model_cfg(ROWS[name][0])[0]
    m = row_model(oracle, name)[3]
    print(f"{name}: {m.selections} selections, {m.scored} scored, score margin {m.score:.3e} (bound {R.score_bound(cfg):.3e})")
    assert m.scored > 0 and (m.score >= R.score_bound(cfg) or name in NO_MARGIN), (name, m.score)
