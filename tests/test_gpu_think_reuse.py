"""Tree reuse of the batched think on the HIP worker (mz_think_reuse_tree=true: think_reroot_kernel behind mz_worker_act, the next search going on from the
kept root) held to the model of tests/think_reuse_model.py, which tests/test_think_reuse_model.py pins on the CPU.  Whole games by think -> act ->
reset_search: the decision, the P and V strings, the think counters and the re-root counters of every move as exact strings and integers; after every
search and every act every field of every visited node of mz_worker_tree against the model's tree, floats as bits, and tree_string as text.  Nothing here has
a tolerance.  Without the feature every test fails: the configuration parser does not know the key."""
import copy

import numpy as np
import pytest

import test_gpu_think as GT
import test_search_model as T
import test_think_model as M
import test_think_reuse_model as X
import think_reuse_model as RM
import tree_model as R
from helpers import sharpen

pytestmark = pytest.mark.gpu
MANUAL = ":mz_manual_step=true"
KEY = "mz_think_reuse_tree"
ON = f":{KEY}=true"


def open_worker(mz, conf, desc_args, w, B, extra=ON, games=1):
    wk = mz.Worker(T.full_conf(conf, games) + MANUAL + f":{M.KEY}={B}" + extra, GT.desc_of(mz, desc_args), w)
    wk.command("start")
    return wk


def finish(wk):
    while not wk.search_done():
        assert wk.run_cycles(5) >= 0


def check_tree(wk, g, t, what, text=True):
    """every field of every visited node against the model's tree: integers exactly, floats as bits; every figure is printed before anything is asserted"""
    got, want = wk.tree(g), R.entries(t)
    n = min(len(got["count"]), len(want["count"]))
    off = {k: int((got[k][:n].view(np.uint32) != want[k][:n].view(np.uint32)).sum()) for k in R.FLOATS}
    print(f"{what}: {len(got['count'])} entries (model {len(want['count'])}); entries whose bits differ: " + ", ".join(f"{k} {v}" for k, v in off.items()))
    for k in R.INTS:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the model\n{got[k]}\n{want[k]}"
    for k in R.FLOATS:
        assert got[k].dtype == np.float32 and got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs from the model in {off[k]} entries"
    if text:
        rec = wk.peek_records(g + 1)[g]
        assert wk.tree_string(g) == R.render(t, rec), f"{what}: tree_string is not the model's tree rendered"
        assert wk.node_info(g, 0) == R.node_text(t, 0)


def follow(mz, oracle, name, B, wk=None, g=0, max_steps=None, moves=None, trees=True):
    """one game of a worker driven through the row's log: every move against the model"""
    conf, desc_args, wseed = X.ROWS[name][:3]
    recs, log = X.reuse_row(oracle, name, B, max_steps=max_steps, moves=moves)
    own = wk is None
    if own:
        wk = open_worker(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), B)
    played, searched = 0, []
    for k, e in enumerate(log):
        if max_steps is None:
            finish(wk)
        else:
            steps = (e["think"][0] - (log[k - 1]["think"][0] if k else 0))
            assert wk.run_cycles(steps) == steps
            if not wk.search_done():
                wk.finish_search()
        d = e["decision"]
        a, p, resign = wk.search_action(g)
        assert (a, p, bool(resign)) == (d["action"], d["player"], recs[k]["resign"]), f"{name} move {k}: decision {(a, p, resign)} != model {(d['action'], d['player'], recs[k]['resign'])}"
        if trees:
            check_tree(wk, g, e["trees"][0], f"{name} B={B} move {k} after the search")
        if recs[k]["resign"]:
            break
        assert wk.act(g, a, p)
        searched.append(played)
        played += 1
        if trees:
            check_tree(wk, g, e["trees"][1], f"{name} B={B} move {k} after act")
        if e["reply"] is not None:
            assert wk.act(g, *e["reply"])
            played += 1
            if trees:
                check_tree(wk, g, e["trees"][2], f"{name} B={B} move {k} after the reply")
        if own:
            assert wk.think_stats() == e["think"], f"{name} move {k}: think counters {wk.think_stats()} != model {e['think']}"
            assert wk.think_reuse_stats() == e["reuse"], f"{name} move {k}: re-root counters {wk.think_reuse_stats()} != model {e['reuse']}"
        if k + 1 < len(log):
            wk.reset_search()
    got = T.parse_record(wk.peek_records(g + 1)[g], played)
    mine = [got[i] for i in searched]  # (a reply is a move of the record too: BaseActor::act gives it the P and V of the search before it)
    model = [(r["action"], {int(a): c for a, c in r["P"].items()}, r["V"], r["R"]) for r in recs if not r["resign"]]
    assert mine == model, f"{name}: the record's moves differ from the model's"
    if own:
        wk.close()
    return log


@pytest.mark.parametrize("name,B", [("ttt", 2), ("ttt", 4), ("go_rot", 4), ("othello_rot", 2)], ids=lambda x: str(x))
def test_whole_game_equals_model(mz, oracle, name, B):
    """TicTacToe to its end (the last move plays into a terminal, unexpanded child: cleared), 12 moves of 9x9 Go and 6 of Othello with a rotation per walk"""
    log = follow(mz, oracle, name, B)
    assert sum(1 for e in log if e["root"] > 0) >= 2


@pytest.mark.parametrize("name,B", [("ttt_reply", 2), ("go_reply", 4)], ids=lambda x: str(x))
def test_two_plies_keep_the_grandchild(mz, oracle, name, B):
    log = follow(mz, oracle, name, B)
    assert any(e["reply"] is not None and len(e["trees"][2].action) > 1 for e in log)


def plain_drive(wk, moves, opponent_moves=None):
    """think -> act (-> the given reply) -> reset_search, `moves` times; -> per move (action, player, resign, P, V, think counters)"""
    out = []
    for k in range(moves):
        finish(wk)
        a, p, r = wk.search_action(0)
        assert wk.act(0, a, p)
        if opponent_moves is not None:
            assert wk.act(0, *opponent_moves[k])
        out.append((a, p, r, wk.think_stats()))
        wk.reset_search()
    return out, wk.peek_records(1)[0]


@pytest.mark.parametrize("name,B", [("ttt_unvisited", 2), ("go_unvisited", 4)], ids=lambda x: str(x))
def test_unvisited_reply_clears(mz, oracle, name, B):
    """a reply whose child has no visit clears the tree: the model's game, and byte for byte the game of a worker without the key given the same moves"""
    conf, desc_args, wseed = X.ROWS[name][:3]
    log = follow(mz, oracle, name, B)
    replies = [e["reply"] for e in log]
    assert all(r is not None for r in replies)
    w = T.case_weights(oracle, desc_args, wseed)
    out = []
    for extra in (ON, ""):
        wk = open_worker(mz, conf, desc_args, w, B, extra)
        out.append(plain_drive(wk, len(replies), replies))
        wk.close()
    assert out[0] == out[1]


_OUTSIDE = {}


def outside_model(oracle, name, B):
    """game 1 of the test below as a single-game model: the row's first search, then a move of the searcher's that has no visit (the last such root child)
    played through act, which clears, then the search of that position.  -> (the move, the trees after the first search, after act and after the second
    search, the second decision)"""
    if (name, B) not in _OUTSIDE:
        conf, desc_args, wseed = X.ROWS[name][:3]
        rs = RM.ReuseSearch(T.model_cfg(conf)[0], M.row_env(oracle, conf), M.row_net(oracle, desc_args, wseed), B)
        d = rs.think()
        t0 = copy.deepcopy(rs.tree)
        outside = next(t0.action[c] for c in reversed(list(t0.kids(0))) if t0.count[c] == 0)
        rs.act(outside, d["player"])
        t1 = copy.deepcopy(rs.tree)
        d2 = rs.think()
        _OUTSIDE[name, B] = (outside, t0, t1, copy.deepcopy(rs.tree), d2, rs.stats())
    return _OUTSIDE[name, B]


def test_three_games_in_one_worker(mz, oracle):
    """one game re-roots, one is cleared by a move outside the tree, one is reset with mz_worker_reset_game: each equals its own single-game model after
    every call — trees with floats as bits, tree_string as text, decisions, counters"""
    name, B, n = "ttt", 2, 16
    conf, desc_args, wseed = X.ROWS[name][:3]
    recs, log = X.reuse_row(oracle, name, B)
    outside, o0, o1, o2, od2, ostats = outside_model(oracle, name, B)
    assert ostats == (1, 0, 0) and len(o1.action) == 1
    first = (log[0]["decision"]["action"], log[0]["decision"]["player"], recs[0]["resign"])
    wk = open_worker(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), B, games=3)
    finish(wk)
    a, p, _ = first
    for g in range(3):
        got = wk.search_action(g)
        assert (got[0], got[1], bool(got[2])) == first, f"game {g}: first decision {got} != model {first}"
        check_tree(wk, g, log[0]["trees"][0], f"game {g} after the first search")
    assert wk.act(0, a, p)
    assert wk.think_reuse_stats() == log[0]["reuse"]
    assert wk.act(1, outside, p)
    assert wk.think_reuse_stats() == (2, 1, log[0]["reuse"][2])
    assert wk.act(2, a, p)
    assert wk.think_reuse_stats() == (3, 2, 2 * log[0]["reuse"][2])
    check_tree(wk, 2, log[0]["trees"][1], "game 2 after act, before its reset")
    wk.reset_game(2)
    check_tree(wk, 0, log[0]["trees"][1], "game 0 after act")
    check_tree(wk, 1, o1, "game 1 after the move outside the tree")
    fresh = RM.fresh_tree(T.model_cfg(conf)[0], o0.player[0])  # (a new game: the root of the row's first search before any visit)
    check_tree(wk, 2, fresh, "game 2 after its reset")
    assert wk.think_reuse_stats() == (3, 2, 2 * log[0]["reuse"][2])  # (a reset is no move: game 2 had kept its subtree until then)
    wk.reset_search()
    finish(wk)
    check_tree(wk, 0, log[1]["trees"][0], "game 0 after the second search")
    check_tree(wk, 1, o2, "game 1 after the search of its own position")
    check_tree(wk, 2, log[0]["trees"][0], "game 2, a new game, after its first search")
    want = [(log[1]["decision"]["action"], log[1]["decision"]["player"], recs[1]["resign"]), (od2["action"], od2["player"], bool(od2["resign"])), first]
    for g in range(3):
        got = wk.search_action(g)
        assert (got[0], got[1], bool(got[2])) == want[g], f"game {g}: second decision {got} != its model's {want[g]}"
    assert wk.think_stats()[2] == 3 * (n + 1) + (n + 1 - log[1]["root"]) + 2 * (n + 1)
    # one more move of each: game 0 re-roots again, game 1 keeps a subtree for the first time, game 2 as the row's first move
    assert wk.act(0, want[0][0], want[0][1])
    check_tree(wk, 0, log[1]["trees"][1], "game 0 after its second act")
    assert wk.act(1, od2["action"], od2["player"]) and wk.act(2, a, p)
    check_tree(wk, 2, log[0]["trees"][1], "game 2 after its act")
    check_tree(wk, 0, log[1]["trees"][1], "game 0 after the other games' acts")
    r = wk.think_reuse_stats()
    assert r[0] == 6 and r[2] == 2 * log[0]["reuse"][2] + (log[1]["reuse"][2] - log[0]["reuse"][2]) + int(wk.tree(1)["count"][0]) + log[0]["reuse"][2]
    wk.close()


def test_action_node_is_refused_after_a_re_root(mz, oracle):
    """node_info(.., 1), the node the decision chose, is a root child only until a move re-roots the tree: refused by name after act, served again after
    the next search; with the key off it stays served after act, as ever"""
    name, B = "ttt", 2
    conf, desc_args, wseed = X.ROWS[name][:3]
    w = T.case_weights(oracle, desc_args, wseed)
    for extra in (ON, ""):
        wk = open_worker(mz, conf, desc_args, w, B, extra)
        finish(wk)
        assert wk.node_info(0, 1)
        a, p, _ = wk.search_action(0)
        assert wk.act(0, a, p)
        if extra:
            with pytest.raises(mz.MzError) as e:
                wk.node_info(0, 1)
            assert KEY in str(e.value) and "re-rooted" in str(e.value), str(e.value)
            assert wk.node_info(0, 0)
        else:
            assert wk.node_info(0, 1)
        wk.reset_search()
        finish(wk)
        assert wk.node_info(0, 1)
        wk.close()


def test_cut_search_is_kept(mz, oracle):
    """mz_worker_finish_search after three steps, then act: the partial tree is kept and no search goes past n + 1"""
    log = follow(mz, oracle, "ttt", 4, max_steps=3, moves=3)
    assert log[1]["root"] > 0


def test_weight_swap_clears(mz, oracle):
    name, B = "ttt", 2
    conf, desc_args, wseed = X.ROWS[name][:3]
    w = T.case_weights(oracle, desc_args, wseed)
    _, log = X.reuse_row(oracle, name, B)
    wk = open_worker(mz, conf, desc_args, w, B)
    finish(wk)
    a, p, _ = wk.search_action(0)
    assert wk.act(0, a, p) and wk.tree(0)["count"][0] == log[0]["trees"][1].count[0] > 0
    wk.set_weights(w)
    tr = wk.tree(0)
    assert len(tr["parent"]) == 1 and tr["count"][0] == 0 and tr["num_children"][0] == 0
    wk.reset_search()
    finish(wk)
    assert wk.think_stats()[2] == 2 * 17 and wk.tree(0)["count"][0] == 17
    wk.close()


def test_default_unchanged(mz, oracle):
    """the key absent and the key false: equal records, counters and trees on a row of test_gpu_think.py's kind"""
    conf, desc_args, wseed = M.ROWS["go_rot"][:3]
    w = T.case_weights(oracle, desc_args, wseed)
    out = []
    for extra in ("", f":{KEY}=false"):
        got, st = GT.drive(mz, conf, desc_args, w, 2, 2, 4, extra)
        out.append((got, st["think"], st["cycles"], st["leaf_evals"]))
    assert out[0] == out[1]
    wk = open_worker(mz, conf, desc_args, w, 4, f":{KEY}=false")
    finish(wk)
    before = wk.tree(0)
    a, p, _ = wk.search_action(0)
    assert wk.act(0, a, p)
    after = wk.tree(0)
    assert all(before[k].tobytes() == after[k].tobytes() for k in before), "with the key off the tree stays as it is until reset_search"
    assert wk.think_reuse_stats() == (0, 0, 0)
    wk.close()


def test_bf16x3_records_equal_f32(mz):
    """the exact network of test_gpu_think.test_bf16x3_records_equal_f32 with the key on: equal records, counters and re-root counters"""
    import exact_nets as E
    shape, kind, shift = E.CERTIFIED_CASES[0]
    net = E.certified_net(shape, kind, shift)
    a = net.args
    d = mz.make_desc(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], vh=a[10], dv=a[11], type_name=a[12])
    w = net.blob(heads_from=mz.generate_weights(d, 3))
    conf = "env_game=go:env_board_size=9:actor_num_simulation=12:actor_resign_threshold=-2:actor_use_random_rotation_features=true"
    out = []
    for prec in ("f32", "bf16x3"):
        wk = open_worker(mz, conf, tuple(a[:13]), w, 4, ON + f":mz_nn_precision={prec}")
        moves, rec = plain_drive(wk, 4)
        out.append((moves, rec, wk.think_reuse_stats(), {k: v.tobytes() for k, v in wk.tree(0).items()}))
        wk.close()
    assert out[0] == out[1]
    assert out[0][2][0] == 4


SHARP = [("ttt", f"env_game=tictactoe:{X.N16}:actor_resign_threshold=-2", M.TTT2, 9, 9), ("go", f"env_game=go:env_board_size=9:{X.N16}:actor_resign_threshold=-2", T.GO8, 82, 24)]


@pytest.mark.parametrize("name,conf,desc_args,A,moves", SHARP, ids=[s[0] for s in SHARP])
def test_capacity_on_a_sharp_network(mz, oracle, name, conf, desc_args, A, moves):
    """a sharpened policy (tests/test_gpu_sharp.py's construction: the policy FC times 1024) keeps one line over many moves: no pool error, the visited
    tree never above the bound, and a search never longer than n + 1 queries"""
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    w = sharpen(od, oracle.gen_weights(od, 1), 1024, 1)
    wk = open_worker(mz, conf, desc_args, w, 4)
    n, kept, before = 16, 0, 0
    for _ in range(moves):
        finish(wk)
        assert wk.tree_size(0) <= 1 + (n + 1) * A and wk.tree(0)["count"][0] == n + 1
        a, p, _ = wk.search_action(0)
        if not wk.act(0, a, p):
            break
        assert wk.tree_size(0) <= 1 + (n + 1) * A
        r = wk.think_reuse_stats()
        assert wk.tree(0)["count"][0] == r[2] - before
        kept, before = r[1], r[2]
        wk.reset_search()
        if wk.env_query(0, 0):
            break
    assert kept >= 3, "the sharpened network did not keep a line"
    print(f"{name}: re-root counters {wk.think_reuse_stats()}, think counters {wk.think_stats()}")
    wk.close()


REFUSALS = [
    ("no_manual_step", f":{M.KEY}=4" + ON, "mz_manual_step"),
    ("batch_of_one", MANUAL + f":{M.KEY}=1" + ON, M.KEY),
    ("dirichlet_noise", MANUAL + f":{M.KEY}=4:actor_use_dirichlet_noise=true" + ON, "actor_use_dirichlet_noise"),
    ("gumbel_noise", MANUAL + f":{M.KEY}=4:actor_use_gumbel_noise=true" + ON, "actor_use_gumbel_noise"),
]


@pytest.mark.parametrize("what,extra,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_name(mz, what, extra, word):
    d = GT.desc_of(mz, T.GO8)
    with pytest.raises(mz.MzError) as e:
        mz.Worker(T.full_conf("env_game=go:env_board_size=9:actor_num_simulation=8", 1) + extra, d, mz.generate_weights(d, 1))
    assert KEY in str(e.value) and word in str(e.value), str(e.value)
