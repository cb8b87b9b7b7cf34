"""The symmetry-averaging model of tests/think_sym_model.py (mz_think_symmetries=8) on the CPU: with a network whose outputs are the same under every
symmetry by construction it plays the plain search of tests/think_model.py; with an ordinary network it does not; and on every row that
tests/test_gpu_think_sym.py runs against the HIP worker, reading the policy through the planes' table (inv) instead of getRotateAction's (fwd) changes the
game, so the rows tell the two apart.  The rows are defined here and shared with the GPU file.  Nothing here compares with a tolerance."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import test_search_model as T
import test_think_model as M
import think_model as TM
import think_sym_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "mz_think_symmetries"
NO_RESIGN = ":actor_resign_threshold=-2"
N16 = ":actor_num_simulation=16" + NO_RESIGN
GO19 = ("go_19x19", 18, 19, 19, 8, 19, 19, 1, 1, 362, 16, 1, "alphazero")  # one block x 8 channels

# name -> (configuration, network, weight seed, moves, batch sizes, board side).  TicTacToe: the smallest table, one word per plane; 9x9 Go: two words and
# the pass under every rotation; 8x8 Othello: the pass on a four-plane game; Gomoku 15x15: four words per plane; 19x19 Go: six words, the last one partial.
# Three moves from the empty board (on which the eight views are one and a row shows nothing); the 19x19 row has two.
ROWS = {
    "ttt": ("env_game=tictactoe" + N16, M.TTT2, 1, 3, (2, 8), 3),
    "go9": ("env_game=go:env_board_size=9" + N16, T.GO8, 1, 3, (2, 8), 9),
    "othello8": ("env_game=othello:env_board_size=8" + N16, T.OTH8, 1, 3, (2, 8), 8),
    "gomoku15": (T._gomoku(15)[0] + N16, T._gomoku(15)[1], 2, 3, (2, 8), 15),
    "go19": ("env_game=go:env_board_size=19:actor_num_simulation=8" + NO_RESIGN, GO19, 2, 2, (4,), 19),  # (weight seed 1 opens with a pass: the board stays empty)
}
ALL = [(n, b, r) for n, row in ROWS.items() for b in row[4] for r in (True, False)]

_SORT = []


def std_sort_fn():
    """the real libstdc++ std::sort of a candidate list (tests/csrc/ref_sort.cpp, as tests/test_gpu_godev.py builds it): policies -> order"""
    if not _SORT:
        so = os.path.join(tempfile.mkdtemp(prefix="refsort"), "libref_sort.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "csrc", "ref_sort.cpp")], check=True, timeout=120)
        lib = C.CDLL(so)
        lib.ref_sort.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]

        def run(policy):
            p = np.ascontiguousarray(policy, np.float32)
            out = np.zeros(len(p), np.int32)
            lib.ref_sort(p.ctypes.data_as(C.POINTER(C.c_float)), len(p), out.ctypes.data_as(C.POINTER(C.c_int)))
            return [int(i) for i in out]
        _SORT.append(run)
    return _SORT[0]


def row_conf(name, rot):
    return ROWS[name][0] + (M.ROT if rot else "")


def sym_env(oracle, name, rot, swap=False):
    """the rules model of tests/rule_envs.py behind the eight views"""
    return SM.SymEnv(T.make_env(oracle, row_conf(name, rot), rules=True), ROWS[name][5], swap)


_CACHE = {}


def sym_row(oracle, name, B, rot, swap=False, moves=None, games=1, first_noise=None, net=None, plain=False):
    """(records per game, the searches, network rows computed) of a row: computed once and shared with tests/test_gpu_think_sym.py.  plain: think_model as
    it is (one view per leaf) on the same environment, network and sort"""
    key = (name, B, rot, swap, moves, games, None if first_noise is None else tuple(x.tobytes() for x in first_noise), id(net), plain)
    if key not in _CACHE:
        conf, desc_args, wseed, row_moves = ROWS[name][:4]
        conf = row_conf(name, rot)
        cfg, _, kv = T.model_cfg(conf)
        draw = M.rotation_stream(oracle, int(kv["program_seed"])) if rot else None
        base = net if net is not None else M.row_net(oracle, desc_args, wseed)
        searches = []
        if plain:
            envs = [PlainRot(T.make_env(oracle, conf, rules=True), ROWS[name][5]) for _ in range(games)]
            the_net = base
        else:
            envs = [sym_env(oracle, name, rot, swap) for _ in range(games)]
            the_net = SM.SymNet(base)
        with SM.std_sort(std_sort_fn()):
            if games == 1:
                recs = [TM.play(cfg, envs[0], the_net, moves or row_moves, B, draw, None if first_noise is None else first_noise[0], searches=searches)]
            else:
                recs = TM.play_pool(cfg, envs, the_net, moves or row_moves, B, draw, first_noise, searches=searches)
        _CACHE[key] = (recs, searches, 0 if plain else the_net.rows)
    return _CACHE[key]


class PlainRot:
    """a rules environment with the one view think_model asks for: features(rot) and rotate_action(a, rot) from the views of SymEnv"""

    def __init__(self, env, side, _sym=None):
        self.sym = _sym if _sym is not None else SM.SymEnv(env, side)

    def clone(self): return PlainRot(None, None, self.sym.clone())
    def act(self, a, player): return self.sym.act(a, player)
    def num_players(self): return self.sym.num_players()
    def turn(self): return self.sym.turn()
    def legal(self): return self.sym.legal()
    def terminal(self): return self.sym.terminal()
    def eval_score(self): return self.sym.eval_score()
    def reward(self): return self.sym.reward()
    def features(self, rot=0): return self.sym.view(rot)
    def rotate_action(self, a, rot): return SM.rotate_point(rot, a, self.sym.side) if a < self.sym.side ** 2 else a


class InvariantNet:
    """a network whose outputs do not depend on the planes and are the same under every symmetry of the board: policy and logit of an action are functions
    of its distance from the centre (the pass has values of its own), multiples of 2^-10 below 1, so that the sum of eight of them is exact; the value is 1/4"""

    def __init__(self, side, A):
        d = np.array([(2 * (a % side) - (side - 1)) ** 2 + (2 * (a // side) - (side - 1)) ** 2 if a < side * side else 3 for a in range(A)])
        self.p = ((1 + d) / 1024.0).astype(np.float32)
        self.l = (-(d / 1024.0)).astype(np.float32)
        assert d.max() + 1 < 1024

    def forward(self, feat):
        return self.p.copy(), self.l.copy(), np.float32(0.25)


@pytest.mark.parametrize("name,B,rot", [("ttt", 2, False), ("ttt", 8, True), ("go9", 8, True), ("othello8", 2, True)], ids=lambda x: str(x))
def test_reduces_to_the_plain_search(oracle, name, B, rot):
    """with an invariant network the average is each view's own output, bit for bit, and the games are think_model's — the rotation drawn per walk included"""
    net = InvariantNet(ROWS[name][5], ROWS[name][1][9])
    mine = sym_row(oracle, name, B, rot, net=net)
    plain = sym_row(oracle, name, B, rot, net=net, plain=True)
    assert [M.strings(r) for r in mine[0]] == [M.strings(r) for r in plain[0]] and len(mine[0][0]) == ROWS[name][3]
    assert signature(mine)[1] == signature(plain)[1], "the trees, floats as bits"
    a, b = M.searches_of(mine[1]), M.searches_of(plain[1])
    assert [(s.steps, s.walks, s.queries) for s in a] == [(s.steps, s.walks, s.queries) for s in b]
    assert [e["rot"] for s in a for e in s.trace] == [e["rot"] for s in b for e in s.trace], "one rotation is drawn per walk, as in the plain search"
    terminal = sum(1 for s in a for e in s.trace for p, q in zip(e["paths"], e["query"]) if q and s.t.nkids[p[-1]] == 0)
    assert mine[2] == 8 * (sum(s.queries for s in a) - terminal)


@pytest.mark.parametrize("name,B,rot", [("ttt", 2, False), ("go9", 8, True), ("othello8", 2, True)], ids=lambda x: str(x))
def test_an_ordinary_network_is_not_invariant(oracle, name, B, rot):
    assert M.strings(sym_row(oracle, name, B, rot)[0][0]) != M.strings(sym_row(oracle, name, B, rot, plain=True)[0][0])


# one (B, rot) per game of the GPU rows: the row whose records a swapped table changes
SWAP_TELLS = [("ttt", 2, False), ("ttt", 8, True), ("go9", 2, True), ("go9", 8, False), ("othello8", 2, False), ("othello8", 8, True), ("gomoku15", 2, True), ("go19", 4, False)]


def signature(row):
    """what tests/test_gpu_think_sym.py compares of a row: the records as strings, and after every search every node of the tree with its floats as bits"""
    import tree_model as R
    trees = [{k: v.tobytes() for k, v in R.entries(s.t).items()} for s in M.searches_of(row[1])]
    return [M.strings(r) for r in row[0]], trees


@pytest.mark.parametrize("name,B,rot", SWAP_TELLS, ids=lambda x: str(x))
def test_rows_tell_a_swapped_table(oracle, name, B, rot):
    """the policy read through inv instead of fwd: the two differ at the quarter turns (r = 1, 3), and a position that is not symmetric shows it — in the
    records of 9x9 and 19x19 Go and of Othello with a batch of 2, and on every row in the trees (priors and logits of the nodes, as bits), which the GPU rows
    compare node by node"""
    side, A = ROWS[name][5], ROWS[name][1][9]
    assert any(not np.array_equal(SM.fwd_table(side, A, r), SM.inv_table(side, A, r)) for r in range(8))
    right, wrong = signature(sym_row(oracle, name, B, rot)), signature(sym_row(oracle, name, B, rot, swap=True))
    print(f"{name} B={B} rot={rot}: records differ: {right[0] != wrong[0]}; searches whose trees differ: {sum(a != b for a, b in zip(right[1], wrong[1]))} of {len(right[1])}")
    assert right[1] != wrong[1], f"{name} with a batch of {B} does not tell fwd from inv"
    if name in ("go9", "go19") or (name, B) == ("othello8", 2):
        assert right[0] != wrong[0], f"{name} with a batch of {B}: the records do not tell fwd from inv"


def test_tables_are_the_planes_own(oracle):
    """a single stone at s shows at fwd_r[s] in the view of rotation r, on every board of the rows (the property test_think_model pins for its rotate());
    the pass keeps its index"""
    for name in ("ttt", "go9", "othello8", "gomoku15"):
        side, A = ROWS[name][5], ROWS[name][1][9]
        for s in (0, 1, side + 2, side * side - 2, 19, 26, 37, 44):  # (the last four: Black's first moves in Othello)
            e = sym_env(oracle, name, False)
            if s >= side * side or not e.legal()[s]:
                continue
            e.act(s, e.turn())
            before = sym_env(oracle, name, False)
            for r in range(8):
                diff = (e.view(r).reshape(-1, side * side)[:2] != before.view(r).reshape(-1, side * side)[:2]).any(0)
                assert SM.fwd_table(side, A, r)[s] in set(np.flatnonzero(diff)), (name, s, r)
        assert all(SM.fwd_table(side, A, r)[a] == a for r in range(8) for a in range(side * side, A))
