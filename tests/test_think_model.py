"""The batched think model of tests/think_model.py (ZeroActor::step under virtual loss, written from the reference's text) on the CPU: with a batch of one
it is the search model of tests/search_model.py; its rows show what they are there for, asserted on the model's own trace; and each wrong reading of the
text named in think_model.READINGS changes a record of some row, so the rows tell the model from it.  tests/test_gpu_think.py runs the same rows against
the HIP worker.  The reference's own ZeroActor::step does not link here (its headers need Boost), so no recorded trace of it stands behind the model: the
model stands on the text.  Nothing here compares with a tolerance."""
import ctypes as C

import numpy as np
import pytest

import search_model as S
import test_search_model as T
import think_model as TM

ROT = ":actor_use_random_rotation_features=true"
KEY = "actor_mcts_think_batch_size"

# name -> (configuration, network, weight seed, moves, batch sizes, gain on the value head or None).  TicTacToe: duplicates below the root, terminal leaves,
# last steps shorter than the batch; the resign row's threshold lies between the root's mean with and without the virtual loss of the last path; Go and
# Othello draw a rotation per walk.  Weight seeds for which the model raises no AmbiguousOrder.
TTT2 = ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9, 16, 1, "alphazero")  # 2 blocks x 16 channels
ROWS = {
    "ttt": ("env_game=tictactoe:actor_num_simulation=16", TTT2, 1, 6, (2, 3, 16), None),
    "ttt_resign": ("env_game=tictactoe:actor_num_simulation=16:actor_resign_threshold=-0.15", TTT2, 1, 6, (2, 3, 16), None),
    "go_rot": ("env_game=go:env_board_size=9:actor_num_simulation=24" + ROT, T.GO8, 1, 2, (4, 8), None),
    "othello_rot": ("env_game=othello:env_board_size=8:actor_num_simulation=24" + ROT, T.OTH8, 1, 2, (4, 8), None),
}
AZ_PUCT_ROWS = [(n, s) for n, c in T.CASES.items() if "puct" in n and c[1][12] == "alphazero" for s in c[2]]


def rotate(a, rot, n):
    """getPositionByRotating (utils/rotation.h:53-95); the pass keeps its index"""
    if a == n * n:
        return a
    c = (n - 1) / 2.0
    x, y = a % n - c, a // n - c
    rx, ry = [(x, y), (y, -x), (-x, -y), (-y, x), (x, -y), (-y, -x), (-x, y), (y, x)][rot]
    return int((ry + c) * n + (rx + c))


class RotEnv(T.OracleEnvAdapter):
    """the oracle's Go or Othello behind the environment of think_model: features under a rotation, and where an action's prior is found under it"""

    def clone(self): return RotEnv(self.o, self.conf, self.hist)
    def features(self, rot=0): return self.e.features(rot)
    def side(self): return int(dict(x.split("=") for x in self.conf.split(":"))["env_board_size"])
    def rotate_action(self, a, rot): return rotate(a, rot, self.side())


def rotation_stream(oracle, seed, count=1 << 16):
    """randInt() % 8 of the generator every game of a one-stream worker draws from (seeded program_seed + 0, actor_group.cpp:66-70)"""
    out = np.zeros(count, np.float64)
    oracle.lib().mzo_rng_vector(seed, 0, count, 1, 0.0, out.ctypes.data_as(C.POINTER(C.c_double)))
    it = iter(out)
    return lambda: int(next(it)) % 8


def row_env(oracle, conf):
    kv = T.model_cfg(conf)[2]
    if kv.get("actor_use_random_rotation_features") == "true":
        return RotEnv(oracle, ":".join(f"{k}={kv[k]}" for k in ("env_game", "env_board_size")))
    return T.make_env(oracle, conf)


def row_net(oracle, desc_args, wseed, vgain=None):
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    return T.NetAdapter(oracle.OracleNet(od, T.case_weights(oracle, desc_args, wseed, vgain)))


_CACHE = {}


def think_row(oracle, name, B, reading=None, games=1, max_steps=None, moves=None, first_noise=None):
    """(records per game, the searches) of a row: computed once and shared with tests/test_gpu_think.py.  One game: think_model.play; several:
    think_model.play_pool, the games of one worker on one RNG stream"""
    key = (name, B, reading, games, max_steps, moves, None if first_noise is None else first_noise.tobytes())
    if key not in _CACHE:
        conf, desc_args, wseed, row_moves, _, vgain = ROWS[name]
        cfg, _, kv = T.model_cfg(conf)
        rot = kv.get("actor_use_random_rotation_features") == "true"
        draw = rotation_stream(oracle, int(kv["program_seed"])) if rot else None
        net, searches = row_net(oracle, desc_args, wseed, vgain), []
        if games == 1:
            recs = [TM.play(cfg, row_env(oracle, conf), net, moves or row_moves, B, draw, first_noise, reading=reading, max_steps=max_steps, searches=searches)]
        else:
            recs = TM.play_pool(cfg, [row_env(oracle, conf) for _ in range(games)], net, moves or row_moves, B, draw, first_noise, searches=searches)
        _CACHE[key] = (recs, searches)
    return _CACHE[key]


def searches_of(searches):
    """every Search of a think_row result, whichever of play / play_pool made it"""
    return [s for x in searches for s in (x.values() if isinstance(x, dict) else [x])]


def strings(rec):
    return [(r["action"], r["P"], r["V"], r["R"], r["resign"]) for r in rec]


@pytest.mark.parametrize("name,wseed", AZ_PUCT_ROWS, ids=lambda x: str(x))
def test_batch_of_one_is_the_search_model(oracle, name, wseed):
    """every AlphaZero PUCT row of test_search_model.CASES (the think model plays no MuZero): a step of one walk never sees a virtual loss"""
    conf, desc_args, _, moves, _, vgain = T.CASES[name]
    cfg = T.model_cfg(conf)[0]
    net = row_net(oracle, desc_args, wseed, vgain)
    searches = []
    mine = TM.play(cfg, T.make_env(oracle, conf), net, moves, 1, searches=searches)
    assert strings(mine) == strings(S.play(cfg, T.make_env(oracle, conf), net, moves))
    assert all(s.steps == s.walks == s.queries == cfg.actor_num_simulation + 1 for s in searches)


def test_rotation_table_is_the_planes_own(oracle):
    """rotate() against the oracle's planes: a single stone at s shows at rotate(s) under every rotation, which is where getRotateAction finds its prior"""
    for rot in range(8):
        for s in (0, 5, 13, 40, 77, 80):
            e = oracle.OracleEnv("env_game=go:env_board_size=9")
            e.reset()
            e.act(s, 1)
            assert set(np.flatnonzero(e.features(rot).reshape(18, 81)[:16].sum(0))) == {rotate(s, rot, 9)}
    assert all(rotate(81, r, 9) == 81 for r in range(8))


def _shows(searches):
    f = dict(duplicate_below_root=0, step_without_duplicate=0, short_last_step=0, terminal_query=0, rotation_for_duplicate=0)
    for s in searches_of(searches):
        for e in s.trace:
            dups = [p for p, q in zip(e["paths"], e["query"]) if not q]
            f["duplicate_below_root"] += any(len(p) > 1 for p in dups)
            f["step_without_duplicate"] += not dups
            f["terminal_query"] += sum(1 for p, q in zip(e["paths"], e["query"]) if q and len(p) > 1 and s.t.nkids[p[-1]] == 0)
            f["rotation_for_duplicate"] += any(r != 0 for r, q in zip(e["rot"], e["query"]) if not q)
        f["short_last_step"] += len(s.trace[-1]["paths"]) < s.B
        assert len(s.trace[0]["paths"]) == min(s.B, s.cfg.actor_num_simulation + 1) and s.trace[0]["query"] == [True] + [False] * (len(s.trace[0]["paths"]) - 1)
        assert s.queries == s.cfg.actor_num_simulation + 1 and all(v == 0 for v in s.t.vl)
    return f


def test_rows_show_what_they_are_for(oracle):
    """asserted on the model's own trace: a step with a duplicate at a leaf below the root, a step with none, a last step shorter than the batch and a
    terminal leaf as a query on TicTacToe; a rotation drawn for a duplicate on Go and Othello; the first step is one query and bs - 1 duplicates of it"""
    for B in ROWS["ttt"][4]:
        f = _shows(think_row(oracle, "ttt", B)[1])
        assert f["duplicate_below_root"] and f["step_without_duplicate"] and f["short_last_step"] and f["terminal_query"], (B, f)
    for name in ("go_rot", "othello_rot"):
        for B in ROWS[name][4]:
            assert _shows(think_row(oracle, name, B)[1])["rotation_for_duplicate"], (name, B)
    assert _shows(think_row(oracle, "othello_rot", 8)[1])["duplicate_below_root"]


# reading -> the rows (name, batch) whose records it changes
TELLS = {
    "remove_one": [("ttt", 2), ("ttt", 3), ("ttt", 16)],
    "duplicates_are_queries": [("ttt", 2), ("ttt", 16), ("go_rot", 4), ("othello_rot", 8)],
    "no_draw_for_duplicates": [("go_rot", 4), ("go_rot", 8), ("othello_rot", 4), ("othello_rot", 8)],
    "done_after_removal": [("ttt_resign", 2), ("ttt_resign", 3), ("ttt_resign", 16)],
    "n_without_vl": [("ttt", 2), ("ttt", 16), ("go_rot", 8)],
    "init_q_skips_count0": [("ttt", 2), ("ttt", 3)],
}


@pytest.mark.parametrize("reading", TM.READINGS)
def test_rows_tell_the_model_from_a_wrong_reading(oracle, reading):
    assert set(TELLS) == set(TM.READINGS)
    for name, B in TELLS[reading]:
        right, wrong = think_row(oracle, name, B)[0][0], think_row(oracle, name, B, reading)[0][0]
        assert strings(right) != strings(wrong), f"{name} with a batch of {B} does not tell the model from '{reading}'"


def test_pool_of_games_on_one_stream(oracle):
    """three games without rotation are three times the single game; with rotation the games take their draws in turn and differ"""
    one = think_row(oracle, "ttt", 3)[0][0]
    assert [strings(r) for r in think_row(oracle, "ttt", 3, games=3)[0]] == [strings(one)] * 3
    pool = think_row(oracle, "othello_rot", 4, games=3)[0]
    assert len({str(strings(r)) for r in pool}) > 1


def test_time_limit_cuts_between_steps(oracle):
    """a think stopped after two steps decides on 1 + B simulations with no virtual loss left; it is not the whole search's decision"""
    recs, searches = think_row(oracle, "ttt", 3, max_steps=2, moves=1)
    s = searches_of(searches)[0]
    assert s.steps == 2 and s.t.num_simulation() == 1 + 3 and all(v == 0 for v in s.t.vl)
    assert sum(int(c) for c in recs[0][0]["P"].values()) == 3
    assert strings(recs[0]) != strings(think_row(oracle, "ttt", 3, moves=1)[0][0])
