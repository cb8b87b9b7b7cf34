"""The read-out of the visited search tree (tree_read_kernel behind mz_worker_tree / mz_worker_tree_string / mz_worker_node_info and ZeroActor::getMCTS())
held to the search model of tests/search_model.py and the batched-think model of tests/think_model.py: the WHOLE tree of a search, not only the root that a
record shows — parent, ordinal, action, player, num_children, depth and count exactly; policy, logit, noise, value and reward within TOL; mean within
TOL * (1 + deepest depth), a mean being an average of discounted sums of at most that many network outputs.  TOL is the bound tests/test_gpu_net.py holds the f32
network to the oracle with; the rows and the condition under which a tolerance may be used at all (every selection decided by a margin far above what TOL can
move) are those of tests/test_tree_model.py.  Every test here fails without the read-out: the entry points do not exist."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_search_model as G
import test_search_model as T
import test_think_model as M
import test_tree_model as X
import think_model as TM
import tree_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANUAL = ":mz_manual_step=true"
PLANS = {"sim_kernel": "", "lockstep": G.LOCKSTEP, "lockstep_host_env": G.HOST_ENV}
COUNTERS = ("cycles", "leaf_evals", "moves", "games", "sim_launches", "sim_cycles", "pre_evals", "pre_hits", "pre_alt_hits", "pre_launches", "pre_batch_launches",
            "pre_pair_launches")


def desc_of(mz, desc_args):
    return mz.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])


def open_worker(mz, oracle, name, extra="", games=1, B=None, manual=True):
    _, conf, desc_args = X.TREE_ROWS[name][:3]
    key = f":{M.KEY}={B}" if B and B > 1 else ""
    wk = mz.Worker(T.full_conf(conf, games) + (MANUAL if manual else "") + key + extra, desc_of(mz, desc_args), X.row_weights(oracle, name))
    wk.command("start")
    return wk


def finish(wk):
    while not wk.search_done():
        assert wk.run_cycles(5) >= 0


def is_muzero(name):
    return T.model_cfg(X.TREE_ROWS[name][1])[1]


def check_plan(name, plan, st):
    """the launch counters and the host-rules timer say which plan ran"""
    if plan == "sim_kernel":
        assert st["sim_launches"] > 0, "the simulation kernel did not run"
    else:
        assert st["sim_launches"] == 0, (plan, st["sim_launches"])
        if not is_muzero(name):  # (a MuZero leaf has no rules: its two lock-step plans are one)
            assert (st["ms_env"] > 0) == (plan == "lockstep_host_env"), (plan, st["ms_env"])


def check_tree(got, t, what=""):
    """case 1's rules.  Every figure is printed before anything is asserted"""
    want = R.entries(t)
    deepest = int(want["depth"].max())
    n = min(len(got["count"]), len(want["count"]))
    diffs = {k: float(np.abs(got[k][:n].astype(np.float64) - want[k][:n]).max()) for k in R.FLOATS}
    print(f"{what}: {len(got['count'])} entries (model {len(want['count'])}), deepest {deepest}, max |device - model|: " + ", ".join(f"{k} {v:.3g}" for k, v in diffs.items()))
    for k in R.INTS + ("count",):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the model\n{got[k]}\n{want[k]}"
    for k in ("policy", "logit", "noise", "value", "reward"):
        assert diffs[k] <= R.TOL, f"{what}: {k} off by {diffs[k]:.3g} > {R.TOL:g}"
    assert diffs["mean"] <= R.TOL * (1 + deepest), f"{what}: mean off by {diffs['mean']:.3g} > {R.TOL * (1 + deepest):g}"
    assert all(got[k].dtype == (np.int32 if k in R.INTS else np.float32) for k in got)


def seeds_of(wk, games):
    return [int(T.SEED.search(r).group(1)) if T.SEED.search(r) else None for r in wk.peek_records(games)]


# ---------------------------------------------------------------------------------------------
# 1. the whole tree against the model, every family on every execution plan it has
# ---------------------------------------------------------------------------------------------
FAMILY_RUNS = [(n, p) for n in X.FAMILY_ROWS for p in PLANS if not (is_muzero(n) and p == "lockstep_host_env")]


@pytest.mark.parametrize("name,plan", FAMILY_RUNS, ids=lambda x: str(x))
def test_whole_tree_equals_model(mz, oracle, name, plan):
    games = X.ATARI_GAMES if T.is_atari(X.TREE_ROWS[name][1]) else (1 if X.TREE_ROWS[name][4] else 2)  # (one RNG stream: the rotation draws of two games interleave)
    wk = open_worker(mz, oracle, name, PLANS[plan], games)
    finish(wk)
    sds = seeds_of(wk, games)
    for g in range(games):
        t, sel, _ = X.model_tree(oracle, name, 1 if X.TREE_ROWS[name][4] else None, env_seed=sds[g])
        check_tree(wk.tree(g), t, f"{name} {plan} game {g}")
        assert wk.node_info(g, 0) == R.node_text_of(wk.tree(g), 0)
        kids = [e for e in range(len(wk.tree(g)["parent"])) if wk.tree(g)["parent"][e] == 0]
        chosen = [e for e in kids if wk.tree(g)["ordinal"][e] == sel - t.first[0]]
        assert len(chosen) == 1 and wk.node_info(g, 1) == R.node_text_of(wk.tree(g), chosen[0]), "the action node is not the model's chosen child"
    check_plan(name, plan, wk.stats())
    wk.close()


# ---------------------------------------------------------------------------------------------
# 2. across plans: the two lock-step plans bit for bit; the simulation kernel in its exact fields, its float differences reported
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["go_puct", "go_mz_puct"])
def test_plans_agree(mz, oracle, name):
    trees = {}
    for plan, extra in PLANS.items():
        wk = open_worker(mz, oracle, name, extra, 1)
        finish(wk)
        trees[plan] = wk.tree(0)
        wk.close()
    a, b, s = trees["lockstep"], trees["lockstep_host_env"], trees["sim_kernel"]
    for k in R.INTS + R.FLOATS:
        assert a[k].tobytes() == b[k].tobytes(), f"{name}: {k} differs between the two lock-step plans"
    for k in R.INTS + ("count",):
        assert np.array_equal(s[k], a[k]), f"{name}: {k} differs between the simulation kernel and lock-step"
    for k in R.FLOATS[1:]:  # reported, not asserted: whether the simulation kernel's floats are lock-step's bit for bit is not known
        d = np.abs(s[k].astype(np.float64) - a[k])
        print(f"{name} simulation kernel vs lock-step: {k} differs in {int((s[k].view(np.uint32) != a[k].view(np.uint32)).sum())} of {len(d)} entries, max {float(d.max()):.3g}")


# ---------------------------------------------------------------------------------------------
# 3. the string
# ---------------------------------------------------------------------------------------------
NODE = re.compile(r"([NBW?])\[(-?\d+)\]C\[([^\]]*)\]")


def flat_nodes(s, record):
    """The small parser: the printed nodes in the order of the string (depth first) as (player char, action id, text), and the root's text.  (Children printed
    without parentheses cannot be told from siblings by the grammar alone — `B[3]C[..]W[1]C[..]W[2]C[..]` —, so the nesting is checked the other way round:
    the string must be what Tree::toString gives over the read-out's own parent links, render_readout below.)"""
    body = s[len(record) - 1:-1]
    return [(m.group(1), int(m.group(2)), m.group(3)) for m in NODE.finditer(body)], re.match(r"C\[([^\]]*)\]", body).group(1)


def render_readout(tr, record):
    """Tree::toString over the read-out's arrays, for comparison with the device's string: depth first, parentheses iff more than one expanded child"""
    n = len(tr["parent"])
    kids = [[] for _ in range(n)]
    for e in range(1, n):
        kids[tr["parent"][e]].append(e)

    def info(e):
        k = sum(1 for c in kids[e] if tr["num_children"][c] > 0)
        out = []
        for c in kids[e]:
            s = "%s[%d]C[%s]%s" % (R.player_char(int(tr["player"][c])), tr["action"][c], R.node_text_of(tr, c), info(c))
            out.append("(" + s + ")" if k > 1 else s)
        return "".join(out)

    return record[:-1] + "C[" + R.node_text_of(tr, 0) + "]" + info(0) + ")"


def structure(tr):
    """the depth-first list of (player char, action, text) computed from the read-out alone"""
    n = len(tr["parent"])
    kids = [[] for _ in range(n)]
    for e in range(1, n):
        kids[tr["parent"][e]].append(e)
    order = []

    def walk(e):
        for c in kids[e]:
            order.append((R.player_char(int(tr["player"][c])), int(tr["action"][c]), R.node_text_of(tr, c)))
            walk(c)

    walk(0)
    return order


@pytest.mark.parametrize("name", ["ttt_puct", "go_puct", "go_mz_gumbel"])
def test_tree_string_parses_back(mz, oracle, name):
    wk = open_worker(mz, oracle, name, "", 1)
    finish(wk)
    rec, tr, s = wk.peek_records(1)[0], wk.tree(0), wk.tree_string(0)
    nodes, root_text = flat_nodes(s, rec)
    assert s.startswith(rec[:-1] + "C[") and s.endswith(")") and root_text == R.node_text_of(tr, 0)
    assert nodes == structure(tr), "the printed nodes are not the read-out's, depth first, with '%.4f' of its values"
    assert s == render_readout(tr, rec), "parentheses or order differ from Tree::toString over the read-out"
    assert s.count("(") == s.count(")") and len(nodes) == len(tr["parent"]) - 1
    wk.close()


FLOAT_FIELDS = re.compile(r"p = [^,\]]*, p_logit = [^,\]]*, p_noise = [^,\]]*, v = [^,\]]*, r = [^,\]]*, mean = [^,\]]*, ")


def test_tree_string_equals_the_rendered_model(mz, oracle):
    """TicTacToe: structure, actions and counts byte for byte (four printed digits of a value that is only good to TOL may differ: the floats are dropped)"""
    wk = open_worker(mz, oracle, "ttt_puct", "", 1)
    finish(wk)
    rec = wk.peek_records(1)[0]
    t = X.model_tree(oracle, "ttt_puct")[0]
    got, want = FLOAT_FIELDS.sub("", wk.tree_string(0)), FLOAT_FIELDS.sub("", R.render(t, rec))
    assert "count = " in got and "mean" not in got and got == want
    wk.close()


# ---------------------------------------------------------------------------------------------
# 4. mid-search and after
# ---------------------------------------------------------------------------------------------
def test_mid_search_and_after(mz, oracle):
    name = "ttt_puct"
    wk = open_worker(mz, oracle, name, G.LOCKSTEP, 1)
    s = X.new_search(oracle, name, 1)
    done = 0
    for k in (1, 2, 7):
        assert wk.run_cycles(k - done) == k - done and not wk.search_done()
        while s.t.num_simulation() < k:
            s.step()
        done = k
        check_tree(wk.tree(0), s.t, f"after {k} cycles")
        if k == 1:
            assert len(wk.tree(0)["parent"]) == 1 and wk.tree(0)["num_children"][0] == 9 and wk.tree(0)["count"][0] == 1
    before = wk.tree(0)
    wk.finish_search()
    after = wk.tree(0)
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)
    assert wk.node_info(0, 1)  # the decision is there
    a, p, _ = wk.search_action(0)
    assert wk.act(0, a, p)
    wk.reset_search()
    assert wk.run_cycles(1) == 1
    cfg = T.model_cfg(X.TREE_ROWS[name][1])[0]
    env = T.make_env(oracle, X.TREE_ROWS[name][1])
    env.act(a, p)
    s2 = TM.Search(cfg, env, M.row_net(oracle, X.TREE_ROWS[name][2], X.TREE_ROWS[name][3]), 1)
    s2.step()
    check_tree(wk.tree(0), s2.t, "the next search after one cycle")
    assert len(wk.tree(0)["parent"]) == 1 and wk.tree(0)["num_children"][0] == 8 and wk.tree(0)["player"][0] == p
    assert wk.stats()["sim_launches"] == 0
    wk.close()


# ---------------------------------------------------------------------------------------------
# 5. the batched think
# ---------------------------------------------------------------------------------------------
THINK_RUNS = [(n, B) for n, r in X.TREE_ROWS.items() if r[0] == "batched think" for B in r[4]]


@pytest.mark.parametrize("name,B", THINK_RUNS, ids=lambda x: str(x))
def test_batched_think_tree(mz, oracle, name, B):
    wk = open_worker(mz, oracle, name, "", 1, B)
    s = X.new_search(oracle, name, B)
    steps = 0
    while not s.done():
        s.step()
        assert wk.run_cycles(1) == 1
        steps += 1
        tr = wk.tree(0)
        if steps <= 2 or s.done():  # between the first steps, and after the search
            check_tree(tr, s.t, f"{name} B={B} after step {steps}")
        for e in range(len(tr["parent"])):
            kids = tr["count"][tr["parent"] == e]
            assert kids.sum() <= tr["count"][e], f"the kept children of entry {e} count more visits than the entry"
    assert wk.search_done() and wk.think_stats() == (s.steps, s.walks, s.queries)
    t, sel, _ = X.model_tree(oracle, name, B)
    check_tree(wk.tree(0), t, f"{name} B={B}, the whole search")
    wk.close()


# ---------------------------------------------------------------------------------------------
# 6. wide parents
# ---------------------------------------------------------------------------------------------
GO19 = ("go_19x19", 18, 19, 19, 8, 19, 19, 1, 1, 362, 16, 1, "alphazero")


def check_wide(mz, wk, min_root_children, min_kept):
    finish(wk)
    tr = wk.tree(0)
    n = len(tr["parent"])
    assert tr["num_children"][0] >= min_root_children
    for e in range(n):
        o = tr["ordinal"][tr["parent"] == e]
        assert np.all(np.diff(o) > 0), f"ordinals of the children of entry {e} do not increase: {o}"
    assert np.all(np.diff(tr["parent"][1:]) >= 0) and np.all(tr["count"][1:] > 0) and tr["count"][0] > 0
    root_kids = np.flatnonzero(tr["parent"] == 0)
    print(f"{len(root_kids)} of the root's {tr['num_children'][0]} children kept, {n} entries")
    assert len(root_kids) >= min_kept
    a, p, _ = wk.search_action(0)
    assert wk.act(0, a, p)
    moves = T.parse_record(wk.peek_records(1)[0], 1)
    P = {k: float(v) for k, v in moves[0][1].items()}
    assert {int(tr["action"][e]): float(tr["count"][e]) for e in root_kids} == P, "the root's kept children are not the P tag's"
    wk.close()


def test_wide_root_9x9(mz, oracle):
    """82 children: the lanes stride the root's children twice (this search follows one line: a single root child is kept, found in the first stride)"""
    check_wide(mz, open_worker(mz, oracle, "go_puct", "", 1), 82, 1)


def test_wide_root_19x19(mz):
    """362 children and more than one stride of KEPT ones: the append position of a stride starts where the stride before it ended.  A PUCT constant of
    1000 makes the prior term outweigh every q, so nearly every simulation opens another root child: the read-out fills its n + 2 entries almost to the last"""
    d = desc_of(mz, GO19)
    conf = "env_game=go:env_board_size=19:actor_num_simulation=150:actor_mcts_puct_init=1000"
    wk = mz.Worker(T.full_conf(conf, 1) + MANUAL, d, mz.generate_weights(d, 1))
    wk.command("start")
    check_wide(mz, wk, 362, 65)


# ---------------------------------------------------------------------------------------------
# 7. it does not disturb the search
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(PLANS))
def test_read_out_does_not_disturb_the_search(mz, oracle, plan):
    name, games, moves = "go_rot", 4, 3
    out = []
    for reading in (False, True):
        wk = open_worker(mz, oracle, name, PLANS[plan], games)
        for _ in range(moves):
            while not wk.search_done():
                assert wk.run_cycles(1) >= 0
                if reading:
                    for g in range(games):
                        assert len(wk.tree(g)["parent"]) >= 1
            acts = [wk.search_action(g) for g in range(games)]
            for g, (a, p, _) in enumerate(acts):
                assert wk.act(g, a, p)
            wk.reset_search()
        st = wk.stats()
        out.append((wk.peek_records(games), wk.pop_lines(), {k: st[k] for k in COUNTERS}))
        check_plan(name, plan, st)
        wk.close()
    assert out[0] == out[1]
    assert all(len(T.parse_record(r, moves)) == moves for r in out[0][0])


# ---------------------------------------------------------------------------------------------
# 8. errors by name
# ---------------------------------------------------------------------------------------------
def test_errors_by_name(mz, oracle):
    import ctypes as C
    wk = open_worker(mz, oracle, "ttt_puct", "", 2, manual=False)
    assert wk.run_cycles(3) == 3
    for call in (lambda: wk.tree(0), lambda: wk.tree_string(0), lambda: wk.node_info(0, 0)):
        with pytest.raises(mz.MzError) as e:
            call()
        assert "tree: the worker plays on its own (mz_manual_step=false)" in str(e.value)
    wk.close()
    wk = open_worker(mz, oracle, "ttt_puct", "", 2)
    assert wk.run_cycles(4) == 4
    for g in (-1, 2):
        with pytest.raises(mz.MzError) as e:
            wk.tree(g)
        assert "libmzgpu error -1" in str(e.value) and "out of range" in str(e.value)
    with pytest.raises(mz.MzError) as e:
        wk.node_info(0, 1)
    assert "libmzgpu error -3" in str(e.value) and "not complete" in str(e.value)
    n = len(wk.tree(0)["parent"])
    assert n >= 2
    buf = np.zeros(n, np.int32)
    rc = wk.L.mz_worker_tree(wk.h, 0, n - 1, buf.ctypes.data_as(C.POINTER(C.c_int)), *([None] * 12))
    assert rc == -4 and f"{n} needed" in mz.last_error()
    assert wk.L.mz_worker_tree(wk.h, 0, n, buf.ctypes.data_as(C.POINTER(C.c_int)), *([None] * 12)) == n and buf[0] == -1
    wk.close()


# ---------------------------------------------------------------------------------------------
# 9. the facade
# ---------------------------------------------------------------------------------------------
def test_tree_through_the_facade(mz, oracle, tmp_path):
    """tests/csrc/tree_check.cpp: createActor, think(true) twice, then getMCTS()->toString(record), getSearchDistributionString(), a walk over
    getRootNode()->getChild(i) and getSearchNodeInfo() — equal to what the ctypes worker gives for the same configuration"""
    from minizero_amd.export_weights import write_mzw
    exe = str(tmp_path / "tree_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "csrc", "tree_check.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-L" + os.path.join(ROOT, "minizero_amd"), "-lmzgpu", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "minizero_amd"), "-o", exe], check=True)
    name = "go_puct"
    _, conf, desc_args = X.TREE_ROWS[name][:3]
    d, w = desc_of(mz, desc_args), X.row_weights(oracle, name)
    pt = str(tmp_path / "weight_iter_1.pt")
    write_mzw(pt[:-3] + ".mzw", d, w)
    swap = lambda c: c.replace("nn_file_name=m.pt", f"nn_file_name={pt}")
    p = subprocess.run([exe, swap(T.full_conf(conf, 1)), "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for line in p.stdout.strip().split("\n"):
        k, _, v = line.partition(" ")
        out.setdefault(k, []).append(v)
    wk = mz.Worker(swap(T.full_conf(conf, 1)) + MANUAL, d, w)
    wk.command("start")
    finish(wk)
    a, pl, _ = wk.search_action(0)
    assert wk.act(0, a, pl)
    wk.reset_search()
    finish(wk)
    a2, p2, _ = wk.search_action(0)
    assert wk.act(0, a2, p2)  # think(true) has played the second move too; the tree stays until the next search is reset
    tr, rec = wk.tree(0), wk.peek_records(1)[0]
    assert out["TREE"] == [wk.tree_string(0)] and out["RECORD"] == [rec]
    root_kids = np.flatnonzero(tr["parent"] == 0)
    assert out["DIST"] == [",".join(f"{int(tr['action'][e])}:{float(tr['count'][e]):g}" for e in root_kids)]
    assert out["DIST"][0] == ",".join(f"{k}:{v}" for k, v in T.parse_record(rec, 2)[1][1].items()), "the distribution is not the record's P tag"
    assert out["INFO"] == ["  root node info: " + wk.node_info(0, 0), "action node info: " + wk.node_info(0, 1)]
    assert out["CHILD"] == [f"{e - root_kids[0]} {int(tr['ordinal'][e])} {int(tr['action'][e])} {float(tr['count'][e]):g} {int(tr['num_children'][e])}" for e in root_kids]
    assert out["NUMSIM"] == [str(int(tr["count"][0]))] and out["MAXCOUNT"] == [str(a2)]
    wk.close()
