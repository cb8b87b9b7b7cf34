"""Symmetry averaging of the batched think on the HIP worker (mz_think_symmetries=8: think_sym_planes_kernel and think_sym_reduce_kernel around one forward
over 8 x games x B rows) held to the model of tests/think_sym_model.py, which tests/test_think_sym_model.py pins on the CPU.  Whole games by think -> act ->
reset_search: the records as exact strings, after every search every field of every visited node of mz_worker_tree against the model's tree, floats as
bits, and tree_string as text; the think counters and the symmetry counters as integers.  The rows are those of test_think_sym_model.ROWS: TicTacToe, 9x9
Go, 8x8 Othello, Gomoku 15x15 and 19x19 Go, each with and without a rotation drawn per walk.  Nothing here has a tolerance.  Without the feature every test
fails at worker creation: the configuration parser does not know the key."""
import pytest

import test_gpu_think as GT
import test_gpu_think_reuse as GR
import test_search_model as T
import test_think_model as M
import test_think_sym_model as X
import think_model as TM
import think_reuse_model as RM
import think_sym_model as SM

pytestmark = pytest.mark.gpu
MANUAL = ":mz_manual_step=true"
ON = f":{X.KEY}=8"


def open_worker(mz, conf, desc_args, w, B, extra=ON, games=1):
    wk = mz.Worker(T.full_conf(conf, games) + MANUAL + f":{M.KEY}={B}" + extra, GT.desc_of(mz, desc_args), w)
    wk.command("start")
    return wk


def trees_of(searches, k, games):
    return [searches[k].t] if games == 1 else [searches[k][g].t for g in range(games)]


def run_row(mz, oracle, name, B, rot, games=1):
    """the row's games on a worker with the key at 8: every move's trees, then the records and the counters, against the model"""
    conf, desc_args, wseed, moves = X.ROWS[name][:4]
    recs, searches, _ = X.sym_row(oracle, name, B, rot, games=games)
    wk = open_worker(mz, X.row_conf(name, rot), desc_args, T.case_weights(oracle, desc_args, wseed), B, games=games)
    for k in range(moves):
        GR.finish(wk)
        for g, t in enumerate(trees_of(searches, k, games)):
            GR.check_tree(wk, g, t, f"{name} B={B} rot={rot} game {g} move {k} after the search")
        for g in range(games):
            a, p, resign = wk.search_action(g)
            assert not resign and wk.act(g, a, p)
        wk.reset_search()
    GT.check([(T.parse_record(r, moves), False) for r in wk.peek_records(games)], recs)
    think, sym, st = wk.think_stats(), wk.think_symmetry_stats(), wk.stats()
    wk.close()
    assert all(len(r) == moves for r in recs)
    assert think == GT.counts(searches), (think, GT.counts(searches))
    assert sym == (think[2], 8 * think[2]) and st["leaf_evals"] == think[2] and st["sim_launches"] == 0
    return think


@pytest.mark.parametrize("name,B,rot", X.ALL, ids=lambda x: str(x))
def test_row_equals_model(mz, oracle, name, B, rot):
    """one word per plane (TicTacToe), two and the pass (9x9 Go), the pass on four planes (Othello), four words (Gomoku 15x15) and six with a partial last
    word (19x19 Go); batches of 2 and 8 (19x19: 4); the rotation option on (a draw per walk, made and not used) and off"""
    run_row(mz, oracle, name, B, rot)


def test_three_games_in_one_worker(mz, oracle):
    """the feature buffer is [8][games][B] with games = 3: every game equals the model's game of it on the one stream of draws, and the counters are three
    times one game's (the draws are not used, so the three games are one game: test_dirichlet_noise_on_the_first_move has two that differ)"""
    think = run_row(mz, oracle, "othello8", 2, True, games=3)
    assert think[2] == 3 * 3 * 17


def plain_games(mz, conf, desc_args, w, B, extra, games=2, moves=2):
    wk = open_worker(mz, conf, desc_args, w, B, extra, games)
    for _ in range(moves):
        GR.finish(wk)
        for g in range(games):
            a, p, _ = wk.search_action(g)
            assert wk.act(g, a, p)
        wk.reset_search()
    st = wk.stats()
    out = (wk.peek_records(games), wk.think_stats(), st["cycles"], st["leaf_evals"], {k: v.tobytes() for k, v in wk.tree(0).items()}), wk.think_symmetry_stats()
    wk.close()
    return out


def test_key_at_1_is_todays_path(mz, oracle):
    """the key at 1 and the key absent: equal records, counters and trees, and one network row per query; at 8 on the same row eight"""
    _, desc_args, wseed = X.ROWS["go9"][:3]
    conf = X.row_conf("go9", True)
    w = T.case_weights(oracle, desc_args, wseed)
    absent, at1, at8 = (plain_games(mz, conf, desc_args, w, 4, extra) for extra in ("", f":{X.KEY}=1", ON))
    assert absent == at1
    assert at1[1] == (at1[0][1][2], at1[0][1][2]) and at1[1][0] == 2 * 2 * 17
    assert at8[1] == (at8[0][1][2], 8 * at8[0][1][2]) and at8[1][0] == 2 * 2 * 17
    assert at8[0][0] != at1[0][0], "an ordinary network is not invariant: the games differ"


def test_with_tree_reuse(mz, oracle):
    """mz_think_reuse_tree=true: 9x9 Go with a rotation drawn per walk, held to tests/think_reuse_model.py driven with the averaging evaluation — decisions,
    the trees after every search and after every act, the think and re-root counters"""
    name, B, rot, moves = "go9", 4, True, 4
    conf, desc_args, wseed = X.ROWS[name][:3]
    conf = X.row_conf(name, rot)
    cfg, _, kv = T.model_cfg(conf)
    log = []
    with SM.std_sort(X.std_sort_fn()):
        recs = RM.play(cfg, X.sym_env(oracle, name, rot), SM.SymNet(M.row_net(oracle, desc_args, wseed)), moves, B, M.rotation_stream(oracle, int(kv["program_seed"])), log=log)
    assert len(recs) == moves and sum(1 for e in log if e["root"] > 0) >= 2
    wk = open_worker(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), B, ON + f":{GR.KEY}=true")
    for k, e in enumerate(log):
        GR.finish(wk)
        d = e["decision"]
        a, p, resign = wk.search_action(0)
        assert (a, p, bool(resign)) == (d["action"], d["player"], False), f"move {k}: decision {(a, p, resign)} != model {(d['action'], d['player'])}"
        GR.check_tree(wk, 0, e["trees"][0], f"reuse move {k} after the search")
        assert wk.act(0, a, p)
        GR.check_tree(wk, 0, e["trees"][1], f"reuse move {k} after act")
        assert wk.think_stats() == e["think"] and wk.think_reuse_stats() == e["reuse"], (k, wk.think_stats(), e["think"], wk.think_reuse_stats(), e["reuse"])
        assert wk.think_symmetry_stats() == (e["think"][2], 8 * e["think"][2])
        wk.reset_search()
    GT.check([(T.parse_record(wk.peek_records(1)[0], moves), False)], [recs])
    wk.close()


def test_dirichlet_noise_on_the_first_move(mz, oracle):
    """two games, two noise vectors on the root the first step expands (from the averaged priors): game g takes draws [g * nc, (g + 1) * nc)"""
    conf, desc_args, wseed = "env_game=go:env_board_size=9:actor_num_simulation=16" + X.NO_RESIGN + T.DIRICHLET, T.GO8, 1
    cfg, _, kv = T.model_cfg(conf)
    games, B = 2, 4
    nc = int(sum(T.make_env(oracle, conf, rules=True).legal()))
    draws = T.noise_draws(oracle, "dirichlet", int(kv["program_seed"]), games, nc, float(kv["actor_dirichlet_noise_alpha"]))
    net = M.row_net(oracle, desc_args, wseed)
    with SM.std_sort(X.std_sort_fn()):
        model = [TM.play(cfg, SM.SymEnv(T.make_env(oracle, conf, rules=True), 9), SM.SymNet(net), 1, B, first_noise=draws[g]) for g in range(games)]
    got, _ = GT.drive(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), games, 1, B, ON)
    GT.check(got, model)
    assert model[0][0]["P"] != model[1][0]["P"], "two noise vectors that lead to one search show nothing"


def test_bf16x3_records_equal_f32(mz):
    """the certified exact network of test_gpu_think.test_bf16x3_records_equal_f32 (the towers put out the same bits at both precisions): with the key at 8
    the records under bf16x3 equal those under f32 byte for byte"""
    import exact_nets as E
    shape, kind, shift = E.CERTIFIED_CASES[0]
    net = E.certified_net(shape, kind, shift)
    a = net.args
    d = mz.make_desc(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], vh=a[10], dv=a[11], type_name=a[12])
    w = net.blob(heads_from=mz.generate_weights(d, 3))
    conf = "env_game=go:env_board_size=9:actor_num_simulation=12:actor_resign_threshold=-2:actor_use_random_rotation_features=true"
    out = [plain_games(mz, conf, tuple(a[:13]), w, 4, ON + f":mz_nn_precision={p}") for p in ("f32", "bf16x3")]
    assert out[0] == out[1]
    assert out[0][1] == (2 * 2 * 13, 8 * 2 * 2 * 13)


REFUSALS = [("hex11", T._hex(11), "hex"), ("havannah4", T._hav(4), "havannah")]


@pytest.mark.parametrize("what,row,game", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_games_without_symmetries_are_refused(mz, what, row, game):
    """Hex and Havannah: the rotation tables are the identity, the eight views of a leaf would be one"""
    conf, desc_args = row
    d = GT.desc_of(mz, desc_args)
    with pytest.raises(mz.MzError) as e:
        mz.Worker(T.full_conf(conf + ":actor_num_simulation=8", 1) + MANUAL + f":{M.KEY}=4" + ON, d, mz.generate_weights(d, 1))
    assert X.KEY in str(e.value) and game in str(e.value), str(e.value)
    wk = mz.Worker(T.full_conf(conf + ":actor_num_simulation=8", 1) + MANUAL + f":{M.KEY}=4:{X.KEY}=1", d, mz.generate_weights(d, 1))  # (at 1 the game plays as ever)
    wk.close()
