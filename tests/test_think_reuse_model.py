"""The tree-reuse model of tests/think_reuse_model.py on the CPU: with reuse off it is think_model.Search move for move; its rows keep trees, clear trees
and re-root twice, asserted on the model's own log; the capacity bound 1 + (n + 1) * A holds on every row; and each wrong reading named in
think_reuse_model.READINGS changes a record, a tree field or a counter of some row, so the rows tell the model from it.  tests/test_gpu_think_reuse.py runs
the same rows against the HIP worker.  Nothing here compares with a tolerance."""
import pytest

import test_search_model as T
import test_think_model as M
import think_model as TM
import think_reuse_model as RM

N16 = "actor_num_simulation=16"
# name -> (configuration, network, weight seed, searched moves, opponent or None).  One searcher plays both sides unless an opponent answers through act
ROWS = {
    "ttt": (f"env_game=tictactoe:{N16}", M.TTT2, 1, 9, None),
    "go_rot": (f"env_game=go:env_board_size=9:{N16}" + M.ROT, T.GO8, 1, 12, None),
    "othello_rot": (f"env_game=othello:env_board_size=8:{N16}" + M.ROT, T.OTH8, 1, 6, None),
    "ttt_reply": (f"env_game=tictactoe:{N16}", M.TTT2, 1, 3, "most_visited_reply"),
    "ttt_unvisited": (f"env_game=tictactoe:{N16}", M.TTT2, 1, 3, "unvisited_reply"),
    "go_reply": (f"env_game=go:env_board_size=9:{N16}", T.GO8, 1, 4, "most_visited_reply"),
    "go_unvisited": (f"env_game=go:env_board_size=9:{N16}", T.GO8, 1, 3, "unvisited_reply"),
}
BATCHES = {"ttt": (2, 4), "go_rot": (4,), "othello_rot": (2,), "ttt_reply": (2,), "ttt_unvisited": (2,), "go_reply": (4,), "go_unvisited": (4,)}
_CACHE = {}


def reuse_row(oracle, name, B, reuse=True, reading=None, max_steps=None, moves=None):
    """(records, log) of a row: computed once and shared with tests/test_gpu_think_reuse.py"""
    key = (name, B, reuse, reading, max_steps, moves)
    if key not in _CACHE:
        conf, desc_args, wseed, row_moves, opp = ROWS[name]
        cfg, _, kv = T.model_cfg(conf)
        rot = kv.get("actor_use_random_rotation_features") == "true"
        draw = M.rotation_stream(oracle, int(kv["program_seed"])) if rot else None
        log = []
        recs = RM.play(cfg, M.row_env(oracle, conf), M.row_net(oracle, desc_args, wseed), moves or row_moves, B, draw, reuse, reading,
                       getattr(RM, opp) if opp else None, max_steps, log=log)
        _CACHE[key] = (recs, log)
    return _CACHE[key]


def dump(t):
    return tuple(tuple(int(x) if k in ("action", "player", "first", "nkids") else float(x) for x in getattr(t, k)) for k in RM.FIELDS if k != "hidden")


def signature(row):
    """everything a row shows: the records, and per move the counters and every field of every node of the trees"""
    recs, log = row
    return M.strings(recs), [(e["root"], e["think"], e["reuse"], e["reply"], [dump(t) for t in e["trees"]]) for e in log]


@pytest.mark.parametrize("name", ["ttt", "go_rot", "othello_rot"])
def test_reuse_off_is_the_think_model(oracle, name):
    conf, desc_args, wseed, moves, _ = ROWS[name]
    cfg, _, kv = T.model_cfg(conf)
    B = BATCHES[name][0]
    draw = M.rotation_stream(oracle, int(kv["program_seed"])) if "rotation" in conf else None
    searches = []
    want = TM.play(cfg, M.row_env(oracle, conf), M.row_net(oracle, desc_args, wseed), moves, B, draw, searches=searches)
    recs, log = reuse_row(oracle, name, B, reuse=False)
    assert M.strings(recs) == M.strings(want)
    assert log[-1]["think"] == (sum(s.steps for s in searches), sum(s.walks for s in searches), sum(s.queries for s in searches))
    assert log[-1]["reuse"] == (0, 0, 0) and all(e["root"] == 0 for e in log)


def test_rows_show_what_they_are_for(oracle):
    for name, Bs in BATCHES.items():
        for B in Bs:
            recs, log = reuse_row(oracle, name, B)
            n = T.model_cfg(ROWS[name][0])[0].actor_num_simulation
            assert all(int(e["trees"][0].count[0]) == n + 1 for e in log), "a search ends at n + 1 root visits, whatever it started with"
            assert log[-1]["think"][2] == sum(n + 1 - e["root"] for e in log), "a root kept with c visits costs n + 1 - c simulations"
            assert all(all(v == 0 for v in t.vl) for e in log for t in e["trees"])
            assert all(t.action[0] == -1 for e in log for t in e["trees"])
    for name in ("ttt", "go_rot", "othello_rot", "ttt_reply", "go_reply"):
        _, log = reuse_row(oracle, name, BATCHES[name][0])
        assert sum(1 for e in log if e["root"] > 0) >= 2, f"{name} keeps no tree"
    for name in ("ttt_reply", "go_reply"):
        _, log = reuse_row(oracle, name, BATCHES[name][0])
        two = [e for e in log if e["reply"] is not None and len(e["trees"][2].action) > 1]
        assert two and all(0 < e["trees"][2].count[0] < e["trees"][1].count[0] for e in two), "no grandchild kept"
    for name in ("ttt_unvisited", "go_unvisited"):
        _, log = reuse_row(oracle, name, BATCHES[name][0])
        cleared = [e for e in log if e["reply"] is not None]
        assert cleared and all(len(e["trees"][2].action) == 1 and len(e["trees"][1].action) > 1 for e in cleared), "the reply does not clear a kept tree"
        assert all(e["root"] == 0 for e in log)
    _, log = reuse_row(oracle, "ttt", 2)
    assert any(len(e["trees"]) > 1 and len(e["trees"][1].action) == 1 for e in log), "TicTacToe never plays into a terminal (unexpanded) child"


def test_capacity_bound_holds(oracle):
    for name, Bs in BATCHES.items():
        conf, desc_args = ROWS[name][:2]
        n, A = T.model_cfg(conf)[0].actor_num_simulation, desc_args[9]
        for B in Bs:
            _, log = reuse_row(oracle, name, B)
            assert max(max(e["nodes"]) for e in log) <= 1 + (n + 1) * A


def test_cut_search_is_kept(oracle):
    """a think stopped after three steps keeps its partial tree, and no later search goes past n + 1"""
    _, log = reuse_row(oracle, "ttt", 4, max_steps=3, moves=3)
    assert 1 < log[0]["trees"][0].count[0] < 17, "the first search was not cut"
    assert log[1]["root"] > 0, "the cut search's tree was not kept"
    assert all(e["root"] < int(e["trees"][0].count[0]) <= 17 for e in log)


# reading -> the rows (name, batch) on which it changes something
TELLS = {
    "n_new_simulations": [("ttt", 2), ("ttt", 4), ("othello_rot", 2)],
    "root_keeps_action": [("ttt", 2), ("go_rot", 4), ("go_reply", 4)],
    "unexpanded_child_kept": [("ttt_unvisited", 2), ("go_unvisited", 4)],
    "one_ply_only": [("ttt_reply", 2), ("go_reply", 4)],
    "vl_survives": [("ttt", 2), ("ttt", 4), ("go_rot", 4)],
    "draws_for_skipped_walks": [("go_rot", 4), ("othello_rot", 2)],
}


@pytest.mark.parametrize("reading", RM.READINGS)
def test_rows_tell_the_model_from_a_wrong_reading(oracle, reading):
    assert set(TELLS) == set(RM.READINGS)
    for name, B in TELLS[reading]:
        assert signature(reuse_row(oracle, name, B)) != signature(reuse_row(oracle, name, B, reading=reading)), \
            f"{name} with a batch of {B} does not tell the model from '{reading}'"
