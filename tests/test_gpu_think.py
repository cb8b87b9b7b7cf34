"""The batched think of the HIP worker (actor_mcts_think_batch_size = B > 1 under mz_manual_step=true: think_select_kernel, think_leaf_kernel,
think_cand_kernel, think_expand_backup_kernel around one forward per step) held to the model of tests/think_model.py, which is written from the reference's
text and pinned on the CPU by tests/test_think_model.py: action, P, V and R of every move, the resignation and the end of the game as exact strings, and the
worker's counters of steps, walks and queries equal to the model's.  The rows are those of test_think_model.ROWS (TicTacToe, Go and Othello with a rotation
drawn per walk) and rows of test_search_model.GAME_CASES for Gomoku, Hex with the swap, NoGo and Havannah over tests/rule_envs.py.  Without the feature every
B > 1 case fails: the worker plays the search of B = 1.  Nothing here has a tolerance."""
import os
import subprocess

import pytest

import test_search_model as T
import test_think_model as M
import think_model as TM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANUAL = ":mz_manual_step=true"


def desc_of(mz, desc_args):
    return mz.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])


def drive(mz, conf, desc_args, w, games, moves, B=None, extra="", cycles_per_move=None):
    """`moves` searches of every game of one worker, the caller playing the searched action after each (per-actor stepping); a game that resigns or ends stops
    the drive.  cycles_per_move: run that many cycles, then mz_worker_finish_search (the time limit striking between two steps).
    -> (per game: [(action, P, V, R)], resigned at the next search?), statistics"""
    key = "" if B is None else f":{M.KEY}={B}"
    wk = mz.Worker(T.full_conf(conf, games) + MANUAL + key + extra, desc_of(mz, desc_args), w)
    wk.command("start")
    resigned, played = [False] * games, 0
    for _ in range(moves):
        if cycles_per_move is None:
            while not wk.search_done():
                assert wk.run_cycles(5) >= 0
        else:
            assert wk.run_cycles(cycles_per_move) == cycles_per_move and not wk.search_done()
            wk.finish_search()
        acts = [wk.search_action(g) for g in range(games)]
        resigned = [r for _, _, r in acts]
        if any(resigned):
            break
        for g, (a, p, _) in enumerate(acts):
            assert wk.act(g, a, p)
        played += 1
        wk.reset_search()
    st = dict(wk.stats())
    st["think"] = wk.think_stats()
    recs = [T.parse_record(r, played) for r in wk.peek_records(games)]
    wk.close()
    return [(recs[g], resigned[g]) for g in range(games)], st


def check(got, model_records):
    """every game of the worker against the model's game of it"""
    assert len(got) == len(model_records)
    for g, ((mv, resigned), rec) in enumerate(zip(got, model_records)):
        played = [(r["action"], {int(k): v for k, v in r["P"].items()}, r["V"], r["R"]) for r in rec if not r["resign"]]
        assert [m[0] for m in mv] == [m[0] for m in played], f"game {g}: actions {[m[0] for m in mv]} != model {[m[0] for m in played]}"
        for k, (a, b) in enumerate(zip(mv, played)):
            assert a[2] == b[2], f"game {g} move {k}: V {a[2]} != model {b[2]}"
            assert a[1] == b[1], f"game {g} move {k}: P differs from the model: {sorted(set(a[1].items()) ^ set(b[1].items()))}"
            assert a[3] == b[3], f"game {g} move {k}: R {a[3]} != model {b[3]}"
        assert resigned == bool(rec and rec[-1]["resign"]), f"game {g}: resigned {resigned}, model {bool(rec and rec[-1]['resign'])}"


def counts(searches):
    ss = M.searches_of(searches)
    return sum(s.steps for s in ss), sum(s.walks for s in ss), sum(s.queries for s in ss)


def run_row(mz, oracle, name, B, games=1, moves=None):
    conf, desc_args, wseed, row_moves, _, vgain = M.ROWS[name]
    recs, searches = M.think_row(oracle, name, B, games=games, moves=moves)
    got, st = drive(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed, vgain), games, moves or row_moves, B)
    check(got, recs)
    assert st["think"] == counts(searches), (st["think"], counts(searches))
    assert st["sim_launches"] == 0
    return st


@pytest.mark.parametrize("name,B", [(n, b) for n in ("ttt", "ttt_resign", "go_rot", "othello_rot") for b in M.ROWS[n][4]], ids=lambda x: str(x))
def test_row_equals_model(mz, oracle, name, B):
    """TicTacToe with B in {2, 3, 16}: duplicates below the root, terminal leaves as queries, last steps shorter than the batch, and a resignation that
    depends on the virtual loss still on the last path; 9x9 Go and 8x8 Othello with B in {4, 8} and a rotation drawn for every walk, duplicates included"""
    run_row(mz, oracle, name, B)


def test_three_games_in_one_worker(mz, oracle):
    """rotation off: each game equals the model, so a leak between the games of a worker fails; the counters are three times one game's"""
    st = run_row(mz, oracle, "ttt", 3, games=3, moves=3)
    assert st["think"][2] == 3 * 3 * 17


# Gomoku, Hex with the swap rule, NoGo and Havannah on the boards of tests/test_gpu_search_model_games.py: (row of T.GAME_CASES, weight seed)
GAME_ROWS = [("gomoku15_puct_n16", 2), ("hex11_puct_n16", 2), ("nogo9_puct_n16", 1), ("hav8_puct_n16", 2)]
_GAME_MODEL = {}


def game_model(oracle, name, wseed, B, moves):
    if (name, wseed, B) not in _GAME_MODEL:
        conf, desc_args = T.GAME_CASES[name][:2]
        searches = []
        recs = TM.play(T.model_cfg(conf)[0], T.make_env(oracle, conf), M.row_net(oracle, desc_args, wseed), moves, B, searches=searches)
        _GAME_MODEL[name, wseed, B] = (recs, searches)
    return _GAME_MODEL[name, wseed, B]


@pytest.mark.parametrize("name,wseed", GAME_ROWS, ids=lambda x: str(x))
def test_game_row_equals_model(mz, oracle, name, wseed):
    B, moves = 4, 2
    conf, desc_args = T.GAME_CASES[name][:2]
    recs, searches = game_model(oracle, name, wseed, B, moves)
    got, st = drive(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), 1, moves, B)
    check(got, [recs])
    assert st["think"] == counts(searches) and st["sim_launches"] == 0


def test_dirichlet_noise_on_the_first_move(mz, oracle):
    """two games, two noise vectors on the root expanded by the first step: game g takes draws [g * nc, (g + 1) * nc) of the Dirichlet stream, as in lock-step"""
    conf, desc_args, _, kind = T.NOISY["go_dirichlet"]
    cfg, _, kv = T.model_cfg(conf)
    games, B, wseed = 2, 4, 1  # (weight seed 2, the lock-step row's, raises AmbiguousOrder under the second noise vector)
    nc = int(sum(T.make_env(oracle, conf).legal()))
    draws = T.noise_draws(oracle, kind, int(kv["program_seed"]), games, nc, float(kv["actor_dirichlet_noise_alpha"]))
    net = M.row_net(oracle, desc_args, wseed)
    model = [TM.play(cfg, T.make_env(oracle, conf), net, 1, B, first_noise=draws[g]) for g in range(games)]
    got, _ = drive(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), games, 1, B)
    check(got, model)
    assert model[0][0]["P"] != model[1][0]["P"], "two noise vectors that lead to one search show nothing"


def test_batch_of_one_is_todays_path(mz, oracle):
    """B = 1 with the key set: the simulation kernel runs and the records are those without the key; the think counters stay 0"""
    conf, desc_args, seeds, moves = T.CASES["go_puct_n24"][:4]
    w = T.case_weights(oracle, desc_args, seeds[0])
    with_key, st1 = drive(mz, conf, desc_args, w, 2, 2, 1)
    without, st0 = drive(mz, conf, desc_args, w, 2, 2, None)
    assert with_key == without and st1["sim_launches"] == st0["sim_launches"] > 0 and st1["think"] == (0, 0, 0)
    assert st1["cycles"] == st0["cycles"] and st1["leaf_evals"] == st0["leaf_evals"]


def test_key_is_ignored_without_manual_step(mz, oracle):
    """ActorGroup never uses the key: a self-play worker with it plays the records of one without"""
    conf, desc_args, seeds = T.CASES["ttt_puct_n16"][:3]
    w = T.case_weights(oracle, desc_args, seeds[0])
    out = []
    for key in ("", f":{M.KEY}=8"):
        wk = mz.Worker(T.full_conf(conf, 2) + key, desc_of(mz, desc_args), w)
        wk.command("start")
        assert wk.run_cycles(17 * 4) == 17 * 4
        out.append((wk.peek_records(2), wk.pop_lines(), wk.think_stats()))
        wk.close()
    assert out[0] == out[1] and out[0][2] == (0, 0, 0)


def test_time_limit_between_steps(mz, oracle):
    """a think that ends after two steps (mz_worker_finish_search, what think() calls when the clock says so) decides like the model cut at that step"""
    conf, desc_args, wseed = M.ROWS["ttt"][:3]
    recs, searches = M.think_row(oracle, "ttt", 3, max_steps=2, moves=1)
    got, st = drive(mz, conf, desc_args, T.case_weights(oracle, desc_args, wseed), 1, 1, 3, cycles_per_move=2)
    check(got, recs)
    assert st["think"] == (2, 6, 4)


def test_bf16x3_records_equal_f32(mz):
    """a certified exact network (tests/exact_nets.py: the towers put out the same bits at both precisions): the batched think's records are equal"""
    import exact_nets as E
    shape, kind, shift = E.CERTIFIED_CASES[0]
    net = E.certified_net(shape, kind, shift)
    a = net.args
    d = mz.make_desc(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], vh=a[10], dv=a[11], type_name=a[12])
    w = net.blob(heads_from=mz.generate_weights(d, 3))
    conf = "env_game=go:env_board_size=9:actor_num_simulation=12:actor_resign_threshold=-2:actor_use_random_rotation_features=true"
    desc_args = tuple(a[:13])
    out = [drive(mz, conf, desc_args, w, 2, 2, 4, f":mz_nn_precision={p}") for p in ("f32", "bf16x3")]
    assert out[0][0] == out[1][0] and all(len(mv) == 2 for mv, _ in out[0][0])
    assert out[0][1]["think"] == out[1][1]["think"] and out[0][1]["think"][2] == 2 * 2 * 13


REFUSALS = [
    ("muzero", "env_game=go:env_board_size=9:nn_type_name=muzero:actor_num_simulation=8", T.GO8_MZ, 4, "", "AlphaZero"),
    ("gumbel", "env_game=go:env_board_size=9:actor_num_simulation=8:actor_use_gumbel=true:actor_gumbel_sample_size=4", T.GO8, 4, "", "actor_use_gumbel"),
    ("host_env", "env_game=go:env_board_size=9:actor_num_simulation=8", T.GO8, 4, ":mz_device_env=false", "mz_device_env"),
    ("too_large", "env_game=go:env_board_size=9:actor_num_simulation=8", T.GO8, 65, "", "at most 64"),
    ("value_rescale", "env_game=go:env_board_size=9:actor_num_simulation=8:actor_mcts_value_rescale=true", T.GO8, 4, "", "actor_mcts_value_rescale"),
]


@pytest.mark.parametrize("what,conf,desc_args,B,extra,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_name(mz, what, conf, desc_args, B, extra, word):
    d = desc_of(mz, desc_args)
    with pytest.raises(mz.MzError) as e:
        mz.Worker(T.full_conf(conf, 1) + MANUAL + f":{M.KEY}={B}" + extra, d, mz.generate_weights(d, 1))
    assert M.KEY in str(e.value) and word in str(e.value), str(e.value)


def test_think_through_the_facade(mz, oracle, tmp_path):
    """tests/csrc/think_check.cpp: createActor, think(true) three times with B = 8, getRecord — the record and the counters equal the ctypes worker's"""
    from minizero_amd.export_weights import write_mzw
    exe = str(tmp_path / "think_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "csrc", "think_check.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-L" + os.path.join(ROOT, "minizero_amd"), "-lmzgpu", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "minizero_amd"), "-o", exe], check=True)
    conf, desc_args, wseed = M.ROWS["othello_rot"][:3]
    d, w = desc_of(mz, desc_args), T.case_weights(oracle, desc_args, wseed)
    pt = str(tmp_path / "weight_iter_1.pt")
    write_mzw(pt[:-3] + ".mzw", d, w)
    full = T.full_conf(conf, 1).replace("nn_file_name=m.pt", f"nn_file_name={pt}") + f":{M.KEY}=8"
    p = subprocess.run([exe, full, "3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    rec = T.parse_record([l for l in lines if l.startswith("RECORD ")][0][len("RECORD "):], 3)
    think = tuple(int(x) for x in [l for l in lines if l.startswith("THINK ")][0].split()[1:])
    got, st = drive(mz, conf, desc_args, w, 1, 3, 8)
    assert rec == got[0][0] and len(rec) == 3 and think == st["think"]
    check(got, M.think_row(oracle, "othello_rot", 8, moves=3)[0])
