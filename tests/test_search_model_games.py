"""What the Gomoku, Hex, NoGo and Havannah rows and the Go and Othello whole-game rows of tests/test_search_model.py (GAME_CASES, GAME_NOISY) are for,
pinned on the CPU with the model alone: the model plays them in the rules models' environment, so nothing here compares two searches.  Each test is a condition a row must meet for its GPU run
(tests/test_gpu_search_model_games.py) to see what it is there to see — a row that backed up no terminal leaf would pass whatever sign the worker gives
a terminal value — and the last one ties the environment the model played in (tests/rule_envs.py over the four rules models) to the product's host
engine, position by position."""
import numpy as np
import pytest

from go_rules import Go
from othello_rules import Othello
import rule_envs
import search_model as S
import test_search_model as T


def _game(name):
    return rule_envs.parse(T.full_conf(T.GAME_CASES[name][0]))[0]


def _actions(oracle, name, wseed):
    return [m[0] for m in T.model_of(oracle, name, wseed)[0]]


@pytest.mark.parametrize("name,wseed", T.ALL_GAME_CASES)
def test_game_row_runs_through_the_model(oracle, name, wseed):
    """No committed (row, seed) raises AmbiguousOrder (it would fail here); a first-moves row plays its three moves; a whole-game row ends at a terminal
    position, without a resignation, having backed up at least 50 terminal leaves inside its searches under PUCT and at least one under Gumbel (the
    adapter counts the eval_score() calls: the search asks for the score at a terminal leaf and nowhere else)"""
    conf, _, _, moves, _, vgain = T.GAME_CASES[name]
    played, resigned, finished = T.model_of(oracle, name, wseed)
    env = T.model_env_of(oracle, name, wseed)
    assert env.hist == [m[0] for m in played]
    if name in T.WHOLE_GAMES:
        leaves = len(env.stats["terminal_leaves"])
        print(f"{name} seed {wseed}: {len(played)} moves, {leaves} terminal leaves, result {float(env.score()):g}")
        assert env.terminal() and finished and not resigned and 0 < len(played) < moves
        assert leaves >= (1 if T.model_cfg(conf)[0].actor_use_gumbel else 50)
        assert all(p[3] == "0" for p in played)  # the R tag of a board game
    elif vgain is None:
        assert len(played) == moves and not resigned and not finished


def test_every_game_has_its_rows():
    """every search as PUCT and as Gumbel; an n = 50 Gumbel row per game; whole games on the four instances and on the small boards; 2 and 4 games"""
    names = set(T.GAME_CASES)
    for b in ("hex11", "gomoku15", "gomoku15oo", "nogo9", "hav8", "hav4"):
        assert {f"{b}_puct_n16", f"{b}_gumbel_n16"} <= names
    assert {"hex11_gumbel_n50", "gomoku15_gumbel_n50", "nogo9_gumbel_n50", "hav8_gumbel_n50"} <= names
    for b in ("hav4", "hav8", "nogo9", "hex11", "gomoku15", "hex4", "hex4_noswap", "hex5", "hex5_noswap", "nogo4", "gomoku5", "gomoku6", "gomoku6_freestyle"):
        assert {f"{b}_game_puct", f"{b}_game_gumbel"} <= names
    for b in ("go4", "go5", "go5_sit", "go7", "go9", "go9c8", "oth8", "oth4", "oth6"):
        assert {f"{b}_game_puct", f"{b}_game_gumbel"} <= names
    assert {"go4_game_puct_n50", "oth4_game_puct_n50"} <= names
    for name, (conf, desc, seeds, moves, games, vgain) in T.GAME_CASES.items():
        cfg, muzero, kv = T.model_cfg(conf)
        assert not muzero and seeds and desc[9] == rule_envs.policy_size(T.full_conf(conf)) and desc[8] == 1 and desc[10] == 16
        assert desc[4] == (8 if name.startswith(("go9c8", "oth8")) else 32) and (desc[4] == 32 or desc in (T.GO8, T.OTH8))
        assert (cfg.actor_num_simulation, cfg.actor_gumbel_sample_size) in ((16, 16), (50, 16))
        whole = name in T.WHOLE_GAMES
        assert games == (2 if whole else 4) and (cfg.actor_resign_threshold == -2.0) == whole
        assert T.has_sim_instance(conf) == (not whole or name.startswith(("hav4", "hav8", "nogo9", "hex11", "gomoku15", "go7", "go9", "oth8")))
        if name in T.GO_ROWS:  # a komi at which both colours win; one row under the situational rule
            assert kv["env_go_komi"] in ("0.5", "1.0") and (kv.get("env_go_ko_rule") == "situational") == name.startswith("go5_sit")


def test_game_rows_show_what_they_are_for(oracle):
    """Over the whole-game rows: each game is won by Black and by White, Gomoku is also drawn (the full board); a Hex row and a Havannah row take the swap
    and one of each declines it where it is offered; a NoGo row searches from a root with fewer than 16 legal moves (the Gumbel sample shrinks); and the
    freestyle Gomoku row is won by six in a row, which the exactly-five rule does not count."""
    results, swap = {}, {}
    few_nogo = False
    for name in [n for n in T.WHOLE_GAMES if n not in T.GO_ROWS + T.OTHELLO_ROWS]:
        conf = T.GAME_CASES[name][0]
        game, _, kw = rule_envs.parse(T.full_conf(conf))
        for wseed in T.GAME_CASES[name][2]:
            env, acts = T.model_env_of(oracle, name, wseed), _actions(oracle, name, wseed)
            results.setdefault(game, set()).add(float(env.score()))
            if kw.get("swap"):
                swap.setdefault(game, set()).add(acts[0] == acts[1])
            if game == "nogo":
                e = rule_envs.RuleEnv(T.full_conf(conf))
                for a in acts:
                    few_nogo = few_nogo or 0 < int(np.sum(e.legal())) < 16
                    e.act(a, e.turn())
    assert results == {"gomoku": {1.0, -1.0, 0.0}, "hex": {1.0, -1.0}, "nogo": {1.0, -1.0}, "havannah": {1.0, -1.0}}
    assert swap == {"hex": {True, False}, "havannah": {True, False}}
    assert few_nogo
    # the swap inside the first-moves rows of the simulation-kernel instances too
    assert any(_actions(oracle, "hex11_puct_n16", s)[0] == _actions(oracle, "hex11_puct_n16", s)[1] for s in T.GAME_CASES["hex11_puct_n16"][2])
    assert any(_actions(oracle, "hav8_puct_n16", s)[0] == _actions(oracle, "hav8_puct_n16", s)[1] for s in T.GAME_CASES["hav8_puct_n16"][2])
    # six in a row: the last stone of the freestyle game completes a line of six and no line of five
    m = T.model_env_of(oracle, "gomoku6_freestyle_game_gumbel", T.GAME_CASES["gomoku6_freestyle_game_gumbel"][2][0]).model
    lines = [m.line(m.actions[-1], dx, dy) for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1))]
    assert not m.exactly_five and m.winner and 6 in lines and 5 not in lines


def _two_passes(hist, n):
    return len(hist) >= 2 and hist[-1] == hist[-2] == n * n


def test_go_and_othello_rows_show_what_they_are_for(oracle):
    """Counted by the adapter over the Go rows: at least 50 terminal leaves backed up per PUCT row (leaves past the move cap, at the end of a game as long as
    the cap, among them), a two-pass leaf, a leaf past the cap, terminal values of both signs and a drawn one (komi 1 on 4x4), a node inside a search whose
    legal mask is smaller than the history-free rules give (a superko refusal in the tree), games won by either colour.  Over the Othello rows: a forced
    pass inside a tree, terminal leaves of both signs, a drawn game."""
    seen = {g: dict(two_pass=0, past_cap=0, values=set(), superko=0, forced=0, results=set()) for g in ("go", "othello")}
    for name in T.GO_ROWS + T.OTHELLO_ROWS:
        conf = T.GAME_CASES[name][0]
        game, n, _ = rule_envs.parse(T.full_conf(conf))
        for wseed in T.GAME_CASES[name][2]:
            env, s = T.model_env_of(oracle, name, wseed), seen[game]
            leaves = env.stats["terminal_leaves"]
            if not T.model_cfg(conf)[0].actor_use_gumbel:
                assert len(leaves) >= 50, (name, wseed, len(leaves))
            s["two_pass"] += sum(_two_passes(h, n) for h, _ in leaves)
            s["past_cap"] += sum(game == "go" and len(h) > 2 * n * n and not _two_passes(h, n) for h, _ in leaves)
            s["values"] |= {float(v) for _, v in leaves}
            s["superko"] += env.stats["superko_in_tree"]
            s["forced"] += env.stats["forced_pass_in_tree"]
            s["results"].add(float(env.score()))
    print(seen)
    go, oth = seen["go"], seen["othello"]
    assert go["two_pass"] >= 1 and go["past_cap"] >= 1 and go["values"] == {1.0, -1.0, 0.0} and go["superko"] >= 1 and {1.0, -1.0} <= go["results"]
    assert oth["forced"] >= 1 and {1.0, -1.0} <= oth["values"] and oth["results"] == {1.0, -1.0, 0.0}


# ---- wrong readings of the rules, each of which the rows tell from the model ----------------------------------------------------------------------
class SimpleKoGo(Go):
    """superko reduced to the simple ko: only the position of two plies ago is refused"""
    def refusal(self, a, player=None):
        r = super().refusal(a, player)
        return None if isinstance(r, tuple) and r[1] != 2 else r


class NoKomiGo(Go):
    """komi left out of the result"""
    def eval_score(self, resign=False):
        b, w = self.areas()
        return super().eval_score(True) if resign else 1.0 if b > w else -1.0 if b < w else 0.0


class OtherKoRuleGo(Go):
    """the situational rule in place of the positional one"""
    def key(self, board, to_move): return (tuple(board), to_move)


class CapOffByOneGo(Go):
    """the move cap with >= in place of >"""
    def is_terminal(self): return super().is_terminal() or len(self.actions) >= 2 * self.P


class PassAlwaysLegalOthello(Othello):
    """the pass legal while a placing move exists"""
    def is_legal(self, a, player=None): return a == self.P or super().is_legal(a, player)


class DrawIsALossOthello(Othello):
    """equal disc counts scored as White's win"""
    def eval_score(self, resign=False):
        v = super().eval_score(resign)
        return -1.0 if v == 0.0 and not resign and not self.can_place(1) and not self.can_place(2) else v


def with_model(model_class):
    """the adapter over a mutant rules model, configured like the row"""
    class Mutant(rule_envs.RuleEnv):
        def __init__(self, conf, _from=None):
            super().__init__(conf, _from=_from)
            if _from is None:
                self.model = model_class(self.n, **rule_envs.parse(conf)[2])
    return Mutant


# mutant -> the rows (first weight seed) of which at least one must play another game
RULE_MUTANTS = {SimpleKoGo: ("go5_sit_game_puct", "go7_game_puct", "go4_game_puct_n50"), NoKomiGo: ("go4_game_puct", "go5_sit_game_puct"),
                OtherKoRuleGo: ("go5_game_puct",), CapOffByOneGo: ("go5_sit_game_puct",),
                PassAlwaysLegalOthello: ("oth4_game_puct",), DrawIsALossOthello: ("oth4_game_gumbel", "oth6_game_gumbel")}


@pytest.mark.parametrize("mutant", list(RULE_MUTANTS), ids=lambda m: m.__name__)
def test_go_and_othello_rows_would_see_a_wrong_reading_of_the_rules(oracle, mutant):
    """with the mutant rules in the environment the search plays in, the model plays another game (other moves, or other P / V strings) on at least one
    row: a worker with that mistake on all its paths would differ from the model there"""
    differs = []
    for name in RULE_MUTANTS[mutant]:
        wseed = T.GAME_CASES[name][2][-1 if name == "go5_sit_game_puct" else 0]
        differs.append(_mutant_game(oracle, name, wseed, with_model(mutant))[0] != T.model_of(oracle, name, wseed)[0])
    print(mutant.__name__, dict(zip(RULE_MUTANTS[mutant], differs)))
    assert any(differs)


class WrongSign(rule_envs.RuleEnv):
    """the terminal value seen from the wrong player"""
    def score(self): return np.float32(-super().score())


class DrawIsALoss(rule_envs.RuleEnv):
    """a full board without a winner scored as White's win"""
    def score(self): return super().score() if self.model.winner else np.float32(-1)


def _mutant_game(oracle, name, wseed, mutant):
    conf, desc_args, _, moves, _, vgain = T.GAME_CASES[name]
    return T.expected_from_model(oracle, conf, desc_args, wseed, moves, weights=T.case_weights(oracle, desc_args, wseed, vgain), env=mutant(T.full_conf(conf)))


def test_whole_game_rows_would_see_a_wrong_terminal_value(oracle):
    """What the rows are for, tried on the model: with the terminal value negated in the environment the search plays in, every whole-game row on a
    board without a simulation-kernel instance plays another game under PUCT (other moves, or other V strings), and so does the Havannah edge 4 row —
    all but Gomoku 5x5, whose terminal leaves are all draws; with Gomoku's draw backed up as a loss that row does.  A worker that made either mistake on all three of its paths alike
    would therefore differ from the model in these rows."""
    rows = [n for n in T.WHOLE_GAMES if n.endswith("_puct") and n not in T.GO_ROWS + T.OTHELLO_ROWS and (n == "hav4_game_puct" or not T.has_sim_instance(T.GAME_CASES[n][0]))]
    assert len(rows) == 9
    for name in rows:
        wseed = T.GAME_CASES[name][2][0]
        if name == "gomoku5_game_puct":  # every terminal leaf of this row is the full board: a zero has no sign
            assert {float(s) for _, s in T.model_env_of(oracle, name, wseed).stats["terminal_leaves"]} == {0.0}
            continue
        assert _mutant_game(oracle, name, wseed, WrongSign)[0] != T.model_of(oracle, name, wseed)[0], name
    assert float(T.model_env_of(oracle, "gomoku5_game_puct", 1).score()) == 0.0
    assert _mutant_game(oracle, "gomoku5_game_puct", 1, DrawIsALoss)[0] != T.model_of(oracle, "gomoku5_game_puct", 1)[0]


def test_gumbel_rows_list_every_root_child(oracle):
    """The P tag of a Gumbel search names every root child that the -38 cut keeps.  On the first moves of the NoGo 9x9 and Havannah edge 8 rows it names
    exactly the legal actions — 81 of the 82 policy entries, 169 of the 225 — so a candidate for the pass slot or for a cut-off cell would be one entry more."""
    for name, legal, size in (("nogo9_gumbel_n16", 81, 82), ("hav8_gumbel_n16", 169, 225), ("hav4_gumbel_n16", 37, 49)):
        conf, desc_args, seeds = T.GAME_CASES[name][:3]
        first = T.model_of(oracle, name, seeds[0])[0][0]
        mask = T.make_env(oracle, conf).legal()
        assert len(mask) == size == desc_args[9] and int(np.sum(mask)) == legal
        assert sorted(first[1]) == [a for a in range(size) if mask[a]], name


def test_resign_row_resigns_and_plays(oracle):
    """the default threshold with the value head times 32: over its seeds the model resigns within its three moves, and plays a move before it does"""
    name = "hex11_puct_n16_resign"
    assert T.model_cfg(T.GAME_CASES[name][0])[0].actor_resign_threshold == S.Cfg().actor_resign_threshold
    outcomes = [T.model_of(oracle, name, s) for s in T.GAME_CASES[name][2]]
    assert all(o[1] and o[2] and len(o[0]) < 3 for o in outcomes) and any(len(o[0]) > 0 for o in outcomes) and any(len(o[0]) == 0 for o in outcomes)


@pytest.mark.parametrize("name", list(T.GAME_NOISY))
def test_noisy_game_rows(oracle, name):
    """eight noise vectors, none of which raises AmbiguousOrder, that lead to more than one first move; Havannah's root has 169 children on the 225-cell array"""
    conf = T.GAME_NOISY[name][0]
    nc = int(np.sum(T.make_env(oracle, conf).legal()))
    assert nc == {"hex11": 121, "hav8_dirichlet": 169}[name] and rule_envs.policy_size(T.full_conf(conf)) == {"hex11": 121, "hav8_dirichlet": 225}[name]
    models = [T.noisy_model(oracle, name, g) for g in range(T.NOISY_GAMES)]
    assert all(len(m[0]) == 1 and not m[1] for m in models)
    assert len({m[0][0][0] for m in models}) > 1


def _same_position(mine, theirs, where):
    assert mine.turn() == theirs.turn(), where
    assert np.array_equal(mine.legal(), theirs.legal_mask()), where
    assert mine.terminal() == theirs.is_terminal(), where
    assert mine.score() == np.float32(theirs.eval_score()), where
    f, g = mine.features(), theirs.features(0)
    assert f.dtype == g.dtype == np.float32 and f.shape == g.shape and np.array_equal(f, g), where


@pytest.mark.parametrize("name,wseed", T.ALL_GAME_CASES)
def test_adapter_equals_host_engine_on_the_models_games(mz, oracle, name, wseed):
    """On every position the model's game passes through, the adapter and the product's host engine (configured by the same string) agree on the player
    to move, the legal mask, the terminal flag, the score and the planes at rotation 0; and on every terminal leaf the model's searches backed up they
    agree that it is terminal and on its score."""
    conf = T.full_conf(T.GAME_CASES[name][0])
    mine, theirs = rule_envs.RuleEnv(conf), mz.Env(conf)
    acts = _actions(oracle, name, wseed)
    for k, a in enumerate(acts):
        _same_position(mine, theirs, f"{name} seed {wseed} before move {k}")
        p = mine.turn()
        mine.act(a, p)
        assert theirs.act(a, p), (name, wseed, k, a)
    _same_position(mine, theirs, f"{name} seed {wseed} after the last move")
    for hist, score in sorted(set(T.model_env_of(oracle, name, wseed).stats["terminal_leaves"])):
        theirs = mz.Env(conf)
        for a in hist:
            assert theirs.act(a), (name, wseed, hist)
        assert theirs.is_terminal() and np.float32(theirs.eval_score()) == score, (name, wseed, hist)
