"""Match play on the HIP worker (mz_worker_create_match) against the model of tests/match_model.py: every `Match` line, every record and
mz_match_stats of whole matches on the smallest boards, on the wide simulation kernel and on lock-step; the first moves on the per-game simulation kernel
of 9x9 Go; every move searched by the right network under a random selection; the execution plans agree; A = B plays a plain worker's games; a precision
per side on an exactly representable network; the bookkeeping; every refusal by its key.  The rows (networks, weight seeds, G, N) are those of
tests/test_match_model.py, which shows on the CPU that they tell the wrong readings of the schedule apart.

What is compared how: a line's head (`Match true <DLEN count> <length> <result>`), its RE / DLEN / PB / PW tags and every move's colour, action, V and R as
exact strings; the P tag of a PUCT root as the exact string, of a Gumbel root as the dictionary of its exact strings (the reference prints an
unordered_map there: tests/search_model.py does not model its iteration order)."""
import functools
import re

import pytest

import exact_nets as E
import match_model as MM
import search_model as S
import test_match_model as X
import test_search_model as T

pytestmark = pytest.mark.gpu

LOCKSTEP = ":mz_sim_kernel=false"
HOST_ENV = ":mz_sim_kernel=false:mz_device_env=false"
LINE = re.compile(r"^(Match \S+ \d+ \d+ \S+) \(;(.*)\) #$")
TAG = re.compile(r"([A-Z]+)\[([^\]]*)\]")
MOVE = re.compile(r";([BW])\[(\d+)\]P\[([^\]]*)\]V\[([^\]]*)\]R\[([^\]]*)\]")


def desc_of(lib, desc_args):
    return lib.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])


def moves_of(record, gumbel):
    """[(colour, action, P, V, R)] of a record in the form the model gives them"""
    p = (lambda s: {int(x.split(":")[0]): x.split(":")[1] for x in s.split(",")} if s else {}) if gumbel else (lambda s: s)
    return [(c, int(a), p(pt), v, r) for c, a, pt, v, r in MOVE.findall(record)]


def parse_line(line, gumbel):
    m = LINE.match(line)
    assert m, line[:200]
    body = m.group(2)
    tags = dict(TAG.findall(body.split(";")[0]))
    return dict(head=m.group(1), RE=tags["RE"], DLEN=tags["DLEN"], PB=tags["PB"], PW=tags["PW"], moves=moves_of(body, gumbel))


def match_conf(name, extra=""):
    conf, _, _, G, N, _ = X.ROWS[name]
    return T.full_conf(conf, G) + f":mz_match_games={N}" + extra


@functools.lru_cache(maxsize=None)
def play(name, extra="", same=False):
    """(lines, match stats, records of every slot afterwards, worker stats) of a row's whole match; same: side B gets side A's weights"""
    import minizero_amd as mz
    import oracle_lib as oracle
    wa, wb = X.row_weights(oracle, name)
    wk = mz.MatchWorker(match_conf(name, extra), desc_of(mz, X.ROWS[name][1]), wa, wa if same else wb)
    assert wk.lanes() == 2
    stats, lines = wk.play()
    assert wk.run_cycles(wk.cycles_per_move()) == 0 and wk.run_cycles(1) == 0, "a finished match runs no further cycle"
    assert wk.stats() == stats
    out = (lines, stats, wk.peek_records(X.ROWS[name][3]), wk.worker_stats())
    wk.close()
    return out


def check_whole(oracle, name, got):
    lines, stats, records, _ = got
    m_lines, m_stats, m_slots, _ = X.row_model(oracle, name)
    gumbel = T.model_cfg(X.ROWS[name][0])[0].actor_use_gumbel
    assert stats == m_stats, f"{name}: match_stats {stats} != model {m_stats}"
    assert len(lines) == len(m_lines) == X.ROWS[name][4]
    for k, (line, want) in enumerate(zip(lines, m_lines)):
        have = parse_line(line, gumbel)
        for key in ("head", "RE", "DLEN", "PB", "PW"):
            assert have[key] == want[key], f"{name}: line {k} (serial {want['serial']}, slot {want['slot']}): {key} {have[key]!r} != model {want[key]!r}"
        assert have["moves"] == want["moves"], f"{name}: line {k} (serial {want['serial']}): moves differ from the model\n  {have['moves']}\n  {want['moves']}"
    # the games still running when the match ended: the slots' fillers (and the games the last step started), move for move
    for sl, rec in zip(m_slots, records):
        tags = dict(TAG.findall(rec.split(";")[1]))
        assert moves_of(rec, gumbel) == sl.moves and tags["PB"] == MM.SIDES[sl.first] and tags["PW"] == MM.SIDES[1 - sl.first], (name, sl.slot, rec[:300])


# ---------------------------------------------------------------------------------------------
# whole games against the model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["", LOCKSTEP], ids=["sim_kernel", "lockstep"])
def test_tictactoe_match_equals_model(mz, oracle, extra):
    """2 b x 16, G = 4, N = 10, n = 8: restarts after an odd and after an even number of steps, four filler games"""
    got = play("ttt", extra)
    check_whole(oracle, "ttt", got)
    assert (got[3]["sim_launches"] == 0) == bool(extra), "the plan asked for did not run"


@pytest.mark.parametrize("name", ["hex3_swap", "othello4_gumbel", "ttt_mz"])
def test_match_equals_model(mz, oracle, name):
    """Hex 3x3 with the swap rule, Othello 4x4 under a Gumbel root, MuZero PUCT on TicTacToe"""
    check_whole(oracle, name, play(name))


def test_go_first_moves_on_the_simulation_kernel(mz, oracle):
    """the per-game simulation kernel of 9x9 Go (G = 4, n = 12): the first three moves of every slot through peek_record; games need not finish"""
    conf, desc_args, _, G, N, steps = X.ROWS["go9"]
    wa, wb = X.row_weights(oracle, "go9")
    wk = mz.MatchWorker(match_conf("go9"), desc_of(mz, desc_args), wa, wb)
    wk.command("start")
    k = wk.cycles_per_move()
    for _ in range(steps + 1):  # (a step's moves are made at the start of the next)
        assert wk.run_cycles(k) == k
    records, st, ms = wk.peek_records(G), wk.worker_stats(), wk.stats()
    wk.close()
    assert st["sim_launches"] > 0, "the simulation kernel did not run"
    _, m_stats, m_slots, _ = X.row_model(oracle, "go9")
    assert ms == m_stats
    for sl, rec in zip(m_slots, records):
        assert moves_of(rec, False)[:steps] == sl.moves and len(sl.moves) == steps, (sl.slot, rec[:300])
        assert f"PB[{MM.SIDES[sl.first]}]PW[{MM.SIDES[1 - sl.first]}]" in rec


# ---------------------------------------------------------------------------------------------
# every move searched by the right network
# ---------------------------------------------------------------------------------------------
def test_every_move_is_searched_by_its_sides_network(mz, oracle):
    """actor_select_action_by_softmax_count=true on TicTacToe: the games differ, the selection is random, the search is not.  For every move of every counted
    game the P tag equals the model's search of that position with the network of the side to move — and not the other side's, where the two differ"""
    name = "ttt"
    lines = play(name, ":actor_select_action_by_count=false:actor_select_action_by_softmax_count=true")[0]
    conf = X.ROWS[name][0]
    cfg = T.model_cfg(conf)[0]
    nets = X.row_nets(oracle, name)
    told, games = 0, set()
    for line in lines:
        g = parse_line(line, False)
        first = MM.SIDES.index(g["PB"])
        env = T.make_env(oracle, conf)
        games.add(tuple(m[1] for m in g["moves"]))
        for k, (colour, action, p, v, r) in enumerate(g["moves"]):
            assert env.turn() == (S.BLACK if colour == "B" else S.WHITE)
            side = (first + k) % 2
            want = {}
            for s in (side, 1 - side):
                t, _, gz = S.search(cfg, env, nets[s])
                want[s] = (MM.p_string(cfg, t, gz), t.root_value_string())
            assert (p, v) == want[side], f"move {k} of {line[:120]}: searched by another network than side {MM.SIDES[side]}'s"
            told += want[side] != want[1 - side]
            env.act(action, env.turn())
    assert told > len(lines) and len(games) > 1, "the two networks or the games do not differ: the row shows nothing"


# ---------------------------------------------------------------------------------------------
# plans agree; A = B; a precision per side
# ---------------------------------------------------------------------------------------------
def test_plans_agree(mz):
    """the simulation kernel, lock-step on the device rules and lock-step on the host rules: identical lines, records and stats"""
    a, b, c = play("ttt"), play("ttt", LOCKSTEP), play("ttt", HOST_ENV)
    assert a[3]["sim_launches"] > 0 and b[3]["sim_launches"] == 0 and c[3]["sim_launches"] == 0
    assert a[:3] == b[:3] == c[:3]


@pytest.mark.parametrize("name", ["ttt", "othello4_gumbel"])
def test_equal_sides_play_a_plain_workers_games(mz, oracle, name):
    """A = B under deterministic settings: the moves of every game — P, V and R tags included — are those of a plain Worker on the same configuration and weights"""
    conf, desc_args, _, G, N, _ = X.ROWS[name]
    lines, stats = play(name, "", True)[:2]
    wk = mz.Worker(T.full_conf(conf, G), desc_of(mz, desc_args), X.row_weights(oracle, name)[0])
    wk.command("start")
    plain = []
    while not plain:
        wk.run_cycles(wk.cycles_per_move())
        plain = wk.pop_lines()
    wk.close()
    body = lambda line: line[line.index(";", line.index("(;") + 2):]  # the moves, behind the root's tags
    assert plain[0].startswith("SelfPlay ") and len(lines) == N
    for line in lines:
        assert line.startswith("Match ") and body(line) == body(plain[0]) and line.split(" ")[1:5] == plain[0].split(" ")[1:5]
    score = float(plain[0].split(" ")[4])
    first = 0 if score > 0 else (2 if score < 0 else 1)
    assert stats["a_first"][first] + stats["a_second"][2 - first] == N and sum(stats["a_first"]) + sum(stats["a_second"]) == N


def _go_exact(precisions):
    """the first moves of a 9x9 Go match on a certified exact network (tests/exact_nets.py; the two sides differ in their heads), per-side precisions"""
    import minizero_amd as mz
    shape, kind, shift = next(c for c in E.CERTIFIED_CASES if c[0] == "go9x64")
    net = E.certified_net(shape, kind, shift)
    d = desc_of(mz, net.args)
    wa, wb = net.blob(heads_from=mz.generate_weights(d, 3)), net.blob(heads_from=mz.generate_weights(d, 4))
    conf = ("env_game=go:env_board_size=9:actor_num_simulation=12:zero_num_parallel_games=4:mz_match_games=4:program_seed=5:nn_file_name=x.pt:actor_resign_threshold=-2"
            f":zero_num_threads=2:mz_match_precision_a={precisions[0]}:mz_match_precision_b={precisions[1]}")
    wk = mz.MatchWorker(conf, d, wa, wb)
    wk.command("start")
    for _ in range(4):
        assert wk.run_cycles(13) == 13
    out = (wk.peek_records(4), wk.stats(), wk.worker_stats()["sim_launches"])
    wk.close()
    return out


def test_precision_per_side_on_an_exact_network(mz):
    """f32 against bf16x3 (and bf16x3 against f32) gives the records of f32 against f32: on a certified network both towers put out the same bits"""
    ref = _go_exact(("f32", "f32"))
    assert ref[2] > 0 and all(len(MOVE.findall(r)) == 3 for r in ref[0]) and len(set(ref[0][:2]) | set(ref[0][2:])) > 1
    for p in (("f32", "bf16x3"), ("bf16x3", "f32")):
        got = _go_exact(p)
        assert got[2] > 0 and got[:2] == ref[:2], p


# ---------------------------------------------------------------------------------------------
# bookkeeping
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ttt", "hex3_swap", "ttt_n_equals_g", "ttt_resign"])
def test_bookkeeping(mz, oracle, name):
    """wins + draws + losses = finished = N = the number of lines; the step counter is the worker's moves; N = G; resignations are tallied for the right side"""
    lines, stats, _, wst = play(name)
    G, N = X.ROWS[name][3:5]
    assert stats["done"] and stats["games_started"] == stats["games_finished"] == N == len(lines) == wst["games"]
    assert sum(stats["a_first"]) + sum(stats["a_second"]) == N and wst["cycles"] == stats["steps"] * (T.model_cfg(X.ROWS[name][0])[0].actor_num_simulation + 1)
    tally = dict(a_first=[0, 0, 0], a_second=[0, 0, 0])
    resigned = 0
    for line in lines:  # the tally again, from the lines alone
        g = parse_line(line, False)
        score = float(g["head"].split(" ")[4])
        first = 0 if score > 0 else (2 if score < 0 else 1)
        if g["PB"] == "A":
            tally["a_first"][first] += 1
        else:
            tally["a_second"][2 - first] += 1
        resigned += "." not in g["RE"]
    assert tally == {k: stats[k] for k in tally} and resigned == stats["resignations"]
    if name == "ttt_n_equals_g":
        assert G == N and stats["filler_games"] >= 1
    if name == "ttt_resign":
        check_whole(oracle, name, play(name))
        assert stats["resignations"] == N and stats["a_first"][2] > 0 and stats["a_second"][0] > 0, "both sides must win a game by the other's resignation"


def test_side_names_and_fixed_keys(mz, oracle):
    wa, wb = X.row_weights(oracle, "ttt")
    wk = mz.MatchWorker(match_conf("ttt", ":mz_match_name_a=old:mz_match_name_b=new"), desc_of(mz, X.ROWS["ttt"][1]), wa, wb)
    for key, value in (("mz_match_games", "12"), ("mz_match_name_a", "x"), ("mz_match_name_b", "x"), ("mz_match_precision_a", "bf16x3"), ("mz_match_precision_b", "f32")):
        with pytest.raises(mz.MzError, match=key):
            wk.command(f"update_config {key}={value}")
    assert not mz.load().mz_worker_net(wk.h), "a match gives out no network handle: its networks are fixed and take turns"
    with pytest.raises(mz.MzError, match="match"):
        wk.net()
    assert wk.command("reset_actors") == 0  # (ignored by default like on any worker: zero_actor_ignored_command)
    wk.command("update_config zero_actor_ignored_command=keep_alive")
    for call in (lambda: wk.command("load_model x.pt"), lambda: wk.set_weights(wa), lambda: wk.load_model("x.pt", wk.desc, wa), lambda: wk.command("reset_actors")):
        with pytest.raises(mz.MzError, match="match"):
            call()
    stats, lines = wk.play()
    assert {parse_line(l, False)["PB"] for l in lines} == {"old", "new"} and all({parse_line(l, False)[k] for k in ("PB", "PW")} == {"old", "new"} for l in lines)
    assert [l.replace("PB[old]", "PB[A]").replace("PW[new]", "PW[B]").replace("PB[new]", "PB[B]").replace("PW[old]", "PW[A]") for l in lines] == play("ttt")[0]
    wk.close()
    plain = mz.Worker(T.full_conf(X.ROWS["ttt"][0], 4), desc_of(mz, X.ROWS["ttt"][1]), wa)
    with pytest.raises(mz.MzError, match="not a match"):
        mz.MatchWorker.stats(plain)
    plain.close()


# ---------------------------------------------------------------------------------------------
# refusals, by key
# ---------------------------------------------------------------------------------------------
REFUSALS = [
    ("zero_num_parallel_games=3:mz_match_games=10", "zero_num_parallel_games"),
    ("zero_num_parallel_games=0:mz_match_games=10", "zero_num_parallel_games"),
    ("zero_num_parallel_games=4:mz_match_games=3", "mz_match_games"),
    ("zero_num_parallel_games=4", "mz_match_games"),
    ("zero_num_parallel_games=4:mz_match_games=4:mz_manual_step=true", "mz_manual_step"),
    ("zero_num_parallel_games=4:mz_match_games=4:actor_mcts_think_batch_size=2", "actor_mcts_think_batch_size"),
    ("zero_num_parallel_games=4:mz_match_games=4:zero_actor_intermediate_sequence_length=4", "zero_actor_intermediate_sequence_length"),
    ("zero_num_parallel_games=4:mz_match_games=4:mz_match_precision_b=fp8", "mz_match_precision_b"),
]


@pytest.mark.parametrize("keys,named", REFUSALS, ids=[r[0].split(":")[-1] for r in REFUSALS])
def test_refused_by_key(mz, oracle, keys, named):
    wa, wb = X.row_weights(oracle, "ttt")
    with pytest.raises(mz.MzError) as e:
        mz.MatchWorker("env_game=tictactoe:actor_num_simulation=8:" + keys, desc_of(mz, X.ROWS["ttt"][1]), wa, wb)
    assert named in str(e.value) and "match" in str(e.value)


def test_refused_atari_and_different_plans(mz, oracle):
    d = desc_of(mz, T.ATARI32)
    w = mz.generate_weights(d, 1)
    with pytest.raises(mz.MzError) as e:
        mz.MatchWorker(T._atari(3) + ":actor_num_simulation=8:zero_num_parallel_games=4:mz_match_games=4", d, w, w)
    assert "env_game=atari" in str(e.value) and "match" in str(e.value)
    # NoGo 9x9 x 64 has a simulation kernel for f32 towers only (sim_nogo.hip): the two precisions resolve to different plans; in lock-step they agree
    d = desc_of(mz, ("nogo_9x9", 18, 9, 9, 64, 9, 9, 1, 1, 82, 16, 1, "alphazero"))
    w = mz.generate_weights(d, 1)
    conf = "env_game=nogo:env_board_size=9:actor_num_simulation=8:zero_num_parallel_games=4:mz_match_games=4:mz_match_precision_b=bf16x3"
    with pytest.raises(mz.MzError) as e:
        mz.MatchWorker(conf, d, w, w)
    assert "mz_match_precision_a" in str(e.value) and "mz_match_precision_b" in str(e.value) and "match" in str(e.value) and "plans" in str(e.value)
    wk = mz.MatchWorker(conf + LOCKSTEP, d, w, w)
    wk.command("start")
    assert wk.run_cycles(9) == 9
    wk.close()
