"""tests/tree_model.py on the CPU: the renderer of the reference's tree SGF and the breadth-first entry list pinned by literals written out by hand from
actor/tree.h:79-110 and actor/mcts.cpp:63-75, told from three wrong readings of that text, and the condition on the inputs under which the rows of
tests/test_gpu_tree.py may be compared with a model whose network differs from the device's in its last bits: every selection of the model's search is decided
by a margin far above what those bits can move (tree_model.Margins).  The table of rows (TREE_ROWS) and the model trees are shared with tests/test_gpu_tree.py."""
import re

import numpy as np
import pytest

import search_model as S
import test_search_model as T
import test_think_model as M
import think_model as TM
import tree_model as R

f32 = np.float32


# ---------------------------------------------------------------------------------------------
# a. the hand-built tree.  Root (White's -1) with four children: A and B expanded, C a visited leaf (a terminal position), D unvisited.  A has two visited
# leaves G and H, B one unvisited child.  (Two visited grandchildren, not one: with one, no node of the tree has more than one displayed child and at most one
# expanded one, and the reading "parentheses by displayed children" could not be told from the text.)
# ---------------------------------------------------------------------------------------------
def hand_tree():
    t = S.Tree(S.Cfg())
    t.reset(S.WHITE)
    t.expand(0, [(3, S.BLACK, 0.5, 1.5), (7, S.BLACK, 0.25, -0.75), (0, S.BLACK, 0.125, -2.0), (8, S.BLACK, 0.125, -2.0)])
    t.expand(1, [(1, S.WHITE, 0.75, 0.5), (2, S.WHITE, 0.25, -0.5)])
    t.expand(2, [(5, S.WHITE, 1.0, 0.0)])
    #        root    A        B      C     D   G       H      I
    count = [5,      3,       1,     1,    0,  1,      1,     0]
    mean = [-0.05,   0.12345, -0.9,  1.0,  0,  0.0626, -0.5,  0]
    value = [0.125,  -0.3,    0.9,   1.0,  0,  0.0626, -0.5,  0]
    reward = [0,     0,       0,     0.5,  0,  0,      0,     0]
    noise = [0,      0.25,    0,     0,    0,  0,      0,     0]
    for i in range(8):
        t.count[i], t.mean[i], t.value[i], t.reward[i], t.noise[i] = f32(count[i]), f32(mean[i]), f32(value[i]), f32(reward[i]), f32(noise[i])
    return t


ENV = "(;GM[tictactoe]RE[0];B[4])"
ROOT_T = "p = 0.0000, p_logit = 0.0000, p_noise = 0.0000, v = 0.1250, r = 0.0000, mean = -0.0500, count = 5.0000"
A_T = "p = 0.5000, p_logit = 1.5000, p_noise = 0.2500, v = -0.3000, r = 0.0000, mean = 0.1235, count = 3.0000"
B_T = "p = 0.2500, p_logit = -0.7500, p_noise = 0.0000, v = 0.9000, r = 0.0000, mean = -0.9000, count = 1.0000"
C_T = "p = 0.1250, p_logit = -2.0000, p_noise = 0.0000, v = 1.0000, r = 0.5000, mean = 1.0000, count = 1.0000"
D_T = "p = 0.1250, p_logit = -2.0000, p_noise = 0.0000, v = 0.0000, r = 0.0000, mean = 0.0000, count = 0.0000"
G_T = "p = 0.7500, p_logit = 0.5000, p_noise = 0.0000, v = 0.0626, r = 0.0000, mean = 0.0626, count = 1.0000"
H_T = "p = 0.2500, p_logit = -0.5000, p_noise = 0.0000, v = -0.5000, r = 0.0000, mean = -0.5000, count = 1.0000"
I_T = "p = 1.0000, p_logit = 0.0000, p_noise = 0.0000, v = 0.0000, r = 0.0000, mean = 0.0000, count = 0.0000"
# the root has two expanded children: every displayed child of it in parentheses; A has none: its two displayed children follow each other bare
EXPECT = ("(;GM[tictactoe]RE[0];B[4]C[" + ROOT_T + "]" + "(B[3]C[" + A_T + "]W[1]C[" + G_T + "]W[2]C[" + H_T + "])" + "(B[7]C[" + B_T + "])" + "(B[0]C[" + C_T + "])" + ")")


def test_render_equals_the_literal():
    assert R.render(hand_tree(), ENV) == EXPECT


def test_render_differs_from_three_wrong_readings():
    t = hand_tree()
    by_displayed = EXPECT.replace("W[1]C[" + G_T + "]W[2]C[" + H_T + "]", "(W[1]C[" + G_T + "])(W[2]C[" + H_T + "])")
    assert R.render(t, ENV, paren_by="displayed") == by_displayed != EXPECT
    unvisited = ("(;GM[tictactoe]RE[0];B[4]C[" + ROOT_T + "]" + "(B[3]C[" + A_T + "]W[1]C[" + G_T + "]W[2]C[" + H_T + "])" + "(B[7]C[" + B_T + "]W[5]C[" + I_T + "])"
                 + "(B[0]C[" + C_T + "])" + "(B[8]C[" + D_T + "])" + ")")
    assert R.render(t, ENV, show_unvisited=True) == unvisited != EXPECT
    six = R.render(t, ENV, digits=6)
    assert "mean = 0.123450, count = 3.000000" in six and six != EXPECT and re.sub(r"(\.\d{4})\d\d", r"\1", six) != EXPECT  # (0.12345 rounds up at four digits)


def test_entries_order_is_pinned():
    e = R.entries(hand_tree())
    assert e["parent"].tolist() == [-1, 0, 0, 0, 1, 1]
    assert e["ordinal"].tolist() == [0, 0, 1, 2, 0, 1]
    assert e["depth"].tolist() == [0, 1, 1, 1, 2, 2]
    assert e["action"].tolist() == [-1, 3, 7, 0, 1, 2]
    assert e["player"].tolist() == [2, 1, 1, 1, 2, 2]
    assert e["num_children"].tolist() == [4, 2, 1, 0, 0, 0]
    assert e["count"].tolist() == [5, 3, 1, 1, 1, 1] and e["count"].dtype == np.float32
    assert e["mean"].tolist() == [f32(x) for x in (-0.05, 0.12345, -0.9, 1.0, 0.0626, -0.5)]
    assert set(e) == set(R.INTS) | set(R.FLOATS)


# ---------------------------------------------------------------------------------------------
# b. the rows of tests/test_gpu_tree.py: name -> (family, configuration, network, weight seed, batch sizes of the batched think or None).  The configurations
# and networks are those of test_search_model.CASES / GAME_CASES and test_think_model.ROWS; the weight seeds are chosen here, on the CPU, by scanning seeds
# from 1 upwards until the model raises no AmbiguousOrder and the row's selection margins hold (test_rows_have_their_selection_margin).
# ---------------------------------------------------------------------------------------------
def _case(family, name, wseed):
    conf, desc_args = T.row(name)[:2]
    return (family, conf, desc_args, wseed, None, None)


def _think(family, name, wseed, batches, vgain=None):
    conf, desc_args = M.ROWS[name][:2]
    return (family, conf, desc_args, wseed, batches, vgain)


# The rows of the batched think carry a gain of 32 on the value head's last layer (helpers.sharpen, as test_search_model's resign row does): the 8-channel
# test networks value all children of a root within 1e-3 of each other, and under virtual loss a step's walks choose among visited siblings whose scores
# then lie 1e-4 apart — no weight seed from 1 to 200 meets the margin without the gain.
THINK_GAIN = 32
TREE_ROWS = {
    "ttt_puct": _case("TicTacToe PUCT", "ttt_puct_n16", 1),
    "go_rot": _think("9x9 Go PUCT with random rotations", "go_rot", 1, (1,)),
    "go_puct": _case("9x9 Go PUCT", "go_puct_n24", 2),
    "go_gumbel": _case("Go Gumbel", "go_gumbel_n50_m16", 2),
    "go_mz_puct": _case("Go MuZero PUCT", "go_mz_puct_n24", 2),
    "go_mz_gumbel": _case("Go MuZero Gumbel", "go_mz_gumbel_n33_m6", 2),
    "othello_gumbel": _case("Othello Gumbel", "othello_gumbel_n16_m16", 1),
    "atari_gumbel": _case("the Atari-shaped Gumbel row", "atari_gumbel_n16_m4", 2),
    "gomoku15": _case("Gomoku 15", "gomoku15_puct_n16", 2),
    "hex11": _case("Hex 11", "hex11_puct_n16", 2),
    "nogo9": _case("NoGo 9", "nogo9_puct_n16", 1),
    "hav8": _case("Havannah 8", "hav8_puct_n16", 2),
    "go_rot_think": _think("batched think", "go_rot", 3, (4, 16), THINK_GAIN),
    "othello_rot_think4": _think("batched think", "othello_rot", 3, (4,), THINK_GAIN),
    "othello_rot_think16": _think("batched think", "othello_rot", 245, (16,), THINK_GAIN),
}
# Othello with a batch of 16: no weight seed from 1 to 299 meets the margin, with a gain of 32 or of 128 — seed 245 comes closest, 1.71e-3 against the bound of
# 1.76e-3.  The row still runs on the GPU under the same comparison; it is the one row that does so without the condition, and the margin test says its figure.
NO_MARGIN = ("othello_rot_think16",)
FAMILIES = ("TicTacToe PUCT", "9x9 Go PUCT with random rotations", "Go Gumbel", "Go MuZero PUCT", "Go MuZero Gumbel", "Othello Gumbel",
            "the Atari-shaped Gumbel row", "Gomoku 15", "Hex 11", "NoGo 9", "Havannah 8")
FAMILY_ROWS = [n for n, r in TREE_ROWS.items() if r[0] in FAMILIES]
ATARI_GAMES = 2


def row_weights(oracle, name, wseed=None):
    _, _, desc_args, seed, _, vgain = TREE_ROWS[name]
    return T.case_weights(oracle, desc_args, seed if wseed is None else wseed, vgain)


def atari_seeds(oracle, name, wseed=None):
    """the seeds the games of an Atari-shaped pool draw when they are created (their SD tags), from the oracle's pool of the same configuration"""
    _, conf, desc_args = TREE_ROWS[name][:3]
    od = oracle.make_desc(*desc_args[:10], vh=desc_args[10], dv=desc_args[11], type_name=desc_args[12])
    og = oracle.OracleGroup(T.full_conf(conf, ATARI_GAMES), od, row_weights(oracle, name, wseed))
    return [int(T.SEED.search(r).group(1)) for r in og.peek_records(ATARI_GAMES)]


def new_search(oracle, name, B=1, env_seed=None, wseed=None):
    """a think_model.Search of the row's first move, to be stepped by the caller (AlphaZero PUCT rows): B = 1 makes a step one simulation"""
    _, conf, desc_args, seed, _, vgain = TREE_ROWS[name]
    cfg, muzero, kv = T.model_cfg(conf)
    assert not muzero and not cfg.actor_use_gumbel
    rot = kv.get("actor_use_random_rotation_features") == "true"
    draw = M.rotation_stream(oracle, int(kv["program_seed"])) if rot else None
    env = M.row_env(oracle, conf) if rot else T.make_env(oracle, conf, env_seed)
    return TM.Search(cfg, env, M.row_net(oracle, desc_args, seed if wseed is None else wseed, vgain), B, draw)


_TREES = {}


def model_tree(oracle, name, B=None, env_seed=None, wseed=None):
    """(the model's tree after the whole search of the row's first move, the index of the chosen root child, the margins of the search), computed once"""
    key = (name, B, env_seed, wseed)
    if key not in _TREES:
        _, conf, desc_args, seed, batches, vgain = TREE_ROWS[name]
        cfg, muzero, _ = T.model_cfg(conf)
        with R.Margins() as m:
            if batches is not None:
                s = new_search(oracle, name, B or 1, wseed=wseed)
                d = s.think()
                t, sel = s.t, d["selected"]
            else:
                net = M.row_net(oracle, desc_args, seed if wseed is None else wseed, vgain)
                t, sel, _ = S.search(cfg, T.make_env(oracle, conf, env_seed), net, muzero)
        _TREES[key] = (t, sel, m)
    return _TREES[key]


def row_margins(oracle, name, wseed=None):
    """[(batch size or None, env seed or None, Margins)] of every search of a row that tests/test_gpu_tree.py compares with the device"""
    conf, batches = TREE_ROWS[name][1], TREE_ROWS[name][4]
    if T.is_atari(conf):
        return [(None, sd, model_tree(oracle, name, env_seed=sd, wseed=wseed)[2]) for sd in atari_seeds(oracle, name, wseed)]
    return [(B, None, model_tree(oracle, name, B, wseed=wseed)[2]) for B in (batches or (None,))]


def holds(cfg, m):
    return m.score >= R.score_bound(cfg)


@pytest.mark.parametrize("name", list(TREE_ROWS))
def test_rows_have_their_selection_margin(oracle, name):
    """the condition on the inputs: every PUCT selection of the model's search whose scores are not equal by construction (tree_model.Margins) is decided by
    at least 16 (puct_init + 1) sqrt(n) TOL"""
    cfg = T.model_cfg(TREE_ROWS[name][1])[0]
    for B, sd, m in row_margins(oracle, name):
        print(f"{name} B={B} seed={sd}: {m.selections} selections, {m.scored} of them scored, score margin {m.score:.3e} (bound {R.score_bound(cfg):.3e})")
        assert m.scored > 0 and (holds(cfg, m) or name in NO_MARGIN), (name, B, sd, m.score)
    assert name not in NO_MARGIN or not all(holds(cfg, m) for _, _, m in row_margins(oracle, name)), "the row meets the margin now: take it off NO_MARGIN"


def test_every_family_keeps_a_row():
    assert {r[0] for r in TREE_ROWS.values()} >= set(FAMILIES)
