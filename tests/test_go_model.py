"""The host engine (minizero_amd/csrc/env.cpp) and the oracle's restatement (oracle/o_env.cpp) of Go, each held to the rules model of tests/go_rules.py,
which shares no code and no data structure with either: every action sequence of the smallest boards, and whole capture-seeking games on boards 2 to 19
(tests/rules_playouts.py) — legal mask, terminal flag, result (at every position, not only at the end), player to move, and the 18 planes under all 8
rotations.  The model itself is held to the outside anchors of tests/test_go_known_answers.py (its third `make_env` parameter).  Every comparison is exact."""
import numpy as np
import pytest

from go_rules import Go
import rules_playouts as R


def engines(mz, oracle, n, komi, rule):
    conf = f"env_game=go:env_board_size={n}:env_go_komi={komi}:env_go_ko_rule={rule}"
    return {"host engine": mz.Env(conf), "oracle": oracle.OracleEnv(conf)}


def check_position(model, envs, where, rotations=()):
    mask = model.legal_mask()
    for name, e in envs.items():
        assert e.turn() == model.turn, f"{name}: turn, {where}"
        assert e.is_terminal() == model.is_terminal(), f"{name}: terminal flag, {where}"
        assert e.eval_score(False) == model.eval_score(), f"{name}: result {e.eval_score(False)} != model {model.eval_score()}, {where}"
        assert e.eval_score(True) == model.eval_score(True), f"{name}: result after a resignation, {where}"
        assert np.array_equal(e.legal_mask(), mask), f"{name}: legal mask differs at {np.flatnonzero(e.legal_mask() != mask)}, {where}"
    for rot in rotations:
        f = model.features(rot)
        for name, e in envs.items():
            assert np.array_equal(e.features(rot), f), f"{name}: planes under rotation {rot}, {where}"


def exhaustive(model, envs, depth):
    """every action sequence from the start to `depth` actions: the per-depth numbers of sequences.  The engines have no undo: they replay the sequence."""
    counts = [0] * (depth + 1)
    seq = []

    def walk():
        counts[len(seq)] += 1
        for e in envs.values():
            e.reset()
            for a in seq:
                assert e.act(a), f"{a} refused after {seq}"
        check_position(model, envs, f"after {seq}")
        if len(seq) == depth or model.is_terminal():
            return
        mask = model.legal_mask()
        for a in np.flatnonzero(mask == 0):  # first, while the engines stand at `seq`; a refused act() changes nothing, as the next one shows
            for name, e in envs.items():
                assert not e.act(int(a)), f"{name} accepts {a} after {seq}"
        for a in np.flatnonzero(mask):
            assert model.act(int(a))
            seq.append(int(a))
            walk()
            seq.pop()
            model.undo()
    walk()
    return counts


@pytest.mark.parametrize("rule", ["positional", "situational"])
@pytest.mark.parametrize("n,depth", [(2, 7), (3, 4)])
def test_every_sequence_of_the_smallest_boards(mz, oracle, n, depth, rule):
    model = Go(n, 0.5, rule)
    counts = exhaustive(model, engines(mz, oracle, n, 0.5, rule), depth)
    print(f"go {n}x{n} {rule}: sequences per depth {counts}")
    assert counts[1] == n * n + 1 and counts[2] == (n * n) * n * n + 1 * (n * n + 1)  # a stone leaves n * n - 1 points and the pass; a pass leaves everything
    assert model.actions == [] and model.history == [] and model.seen == set()         # undo() took everything back


def test_undo_restores_the_model():
    """undo() after every kind of action — capture, pass, a repeated position under a pass — leaves exactly the state before"""
    for name in ("go3_pos_komi9", "go5_sit"):
        n, rule, komi, _, _, _ = R.GO_ROWS[name]
        for _, actions, _ in R.go_games(name)[:6]:
            g = Go(n, komi, rule)
            for a in actions:
                before = (list(g.board), g.turn, list(g.actions), list(g.history), set(g.seen))
                assert g.act(a)
                c = g.clone()
                g.undo()
                assert (g.board, g.turn, g.actions, g.history, g.seen) == before
                assert g.act(a) and (g.board, g.turn, g.actions, g.history, g.seen) == (c.board, c.turn, c.actions, c.history, c.seen)


@pytest.mark.parametrize("name", list(R.GO_ROWS))
def test_capture_seeking_playouts(mz, oracle, name):
    """whole games played by the model: after every action both engines equal the model, planes under all 8 rotations included"""
    n, rule, komi, _, _, _ = R.GO_ROWS[name]
    for seed, actions, _ in R.go_games(name):
        model, envs = Go(n, komi, rule), engines(mz, oracle, n, komi, rule)
        check_position(model, envs, f"{name} seed {seed} at the start", range(8))
        for i, a in enumerate(actions):
            assert model.act(a)
            for e_name, e in envs.items():
                assert e.act(a), f"{e_name} refuses action {i} = {a} of {name} seed {seed}"
            check_position(model, envs, f"{name} seed {seed} after {actions[:i + 1]}", range(8))
        assert model.is_terminal()


def test_what_the_playout_table_shows():
    """Conditions on the table, counted on the model alone: without them the comparisons above and on the device (tests/test_gpu_go_model.py) would not have
    met the cases they are there for.  The seeds of tests/rules_playouts.py were chosen until all of them hold."""
    rows = {name: R.go_row_summary(name) for name in R.GO_ROWS}
    for name, s in rows.items():
        print(name, s)
    board = {name: R.GO_ROWS[name][0] for name in rows}
    total = lambda key, names=rows: sum(rows[x][key] for x in names)
    assert max(s["max_capture"] for name, s in rows.items() if board[name] >= 9) >= 4
    assert total("multi_block_captures") >= 1
    assert total("suicide_single") >= 1 and total("suicide_multi") >= 1
    assert total("simple_ko") >= 1
    assert total("long_superko", [x for x in rows if board[x] <= 5]) >= 1
    assert total("ko_rules_differ") >= 1
    assert total("ended_by_passes") >= 1 and total("ended_by_cap") >= 1
    assert total("black_wins") >= 1 and total("white_wins") >= 1 and total("draws") >= 1
    (_, actions, ev), = R.go_games("go19_pos_nopass")
    assert len(actions) == 2 * 19 * 19 + 1 == 723 and ev["passes"] == 0 and 361 not in actions
    for n in (2, 3, 5, 8, 9, 11, 13, 16, 19):
        assert {R.GO_ROWS[x][1] for x in rows if board[x] == n} == {"positional", "situational"}, f"board {n} needs both ko rules"
    assert {7.5, 0.5, 9.0} <= {R.GO_ROWS[x][2] for x in rows}
    # 3x3 with komi 9: Black owning the board is a draw, and that is where the table's draws come from
    assert rows["go3_pos_komi9"]["draws"] >= 1 and rows["go3_pos_komi9"]["black_wins"] == 0


def hand_cases():
    """[(name, board, ko rule, actions, steps from the end that matter)]: the sequences of tests/hand_go.py, each confirmed on the model to be what it claims"""
    import hand_go as HG
    out = []
    # a chain through all six words of 19x19, captured whole by Black's last stone
    actions, chain = HG.winding_chain()
    g = Go(19, 7.5)
    for a in actions[:-1]:
        assert g.act(a), a
    assert all(g.board[p] == 2 for p in chain) and g.block(chain[0]) == (set(chain), {actions[-1]}) and g.turn == 1
    assert {p // 64 for p in chain} == {0, 1, 2, 3, 4, 5}
    for w in range(1, 6):  # two adjacent stones of the chain on either side of every word boundary
        assert any(q in chain and q // 64 == w for p in chain if p // 64 == w - 1 for q in g.neighbours(p)), w
    assert [len(b) for b in g.place(actions[-1], 1)[1]] == [len(chain)] and g.act(actions[-1]) and not any(g.board[p] for p in chain)
    out.append(("winding chain", 19, "positional", actions, 2))
    # one stone, four blocks
    actions, white = HG.four_blocks()
    g = Go(HG.FOUR_N, 7.5)
    for a in actions[:-1]:
        assert g.act(a), a
    assert not g._quiet(HG.FOUR_CENTRE, 1) and sorted(map(sorted, g.place(HG.FOUR_CENTRE, 1)[1])) == sorted([p] for p in white)
    assert {p // 64 for p in white} == {0, 1} and g.refusal(HG.FOUR_CENTRE, 2) == "suicide" and g.act(actions[-1])
    out.append(("four blocks", HG.FOUR_N, "positional", actions, 2))
    # the snapback
    for rule in ("positional", "situational"):
        actions, b, a = HG.snapback()
        g = Go(HG.SNAP_N, 0.5, rule)
        for x in actions:
            assert g.act(x), x
        assert actions[-1] == a and g.board[a] == 1 and g.block(a)[1] == {b}
        assert [len(c) for c in g.place(b, 2)[1]] == [1] and g.act(b)
        assert g.block(b) == ({b, 1, 8, 9, 10}, {a}) and g.refusal(a) is None  # no ko: what it captures is more than what was taken
        assert [len(c) for c in g.place(a, 1)[1]] == [5] and g.act(a)
        out.append((f"snapback, {rule}", HG.SNAP_N, rule, actions + [b, a], 3))
    # the long cycle and the position that tells the ko rules apart: the refusal is in the last position's legal mask
    for rule in ("positional", "situational"):
        g = Go(HG.CYCLE_N, 0.5, rule)
        for x in HG.CYCLE:
            assert g.act(x), x
        assert g.refusal(HG.CYCLE_POINT) == ("superko", HG.CYCLE_AGE)
        out.append((f"eight-ply cycle, {rule}", HG.CYCLE_N, rule, HG.CYCLE, 1))
        g = Go(HG.DIFFER_N, 0.5, rule)
        for x in HG.KO_RULES_DIFFER:
            assert g.act(x), x
        assert g.refusal(HG.DIFFER_POINT) == (None if rule == "situational" else ("superko", HG.DIFFER_AGE))
        assert tuple(g.place(HG.DIFFER_POINT, 1)[0]) == g.history[-HG.DIFFER_AGE]
        out.append((f"ko rules differ, {rule}", HG.DIFFER_N, rule, HG.KO_RULES_DIFFER, 1))
    return out


def test_hand_sequences_on_both_engines(mz, oracle):
    """the sequences of tests/hand_go.py — confirmed on the model by hand_cases() — on the host engine and the oracle, every position of each"""
    for name, n, rule, actions, _ in hand_cases():
        model, envs = Go(n, 0.5, rule), engines(mz, oracle, n, 0.5, rule)
        for i, a in enumerate(actions):
            assert model.act(a)
            for e in envs.values():
                assert e.act(a)
            check_position(model, envs, f"{name} after {actions[:i + 1]}", (0, 5))
