"""GPU tests of the learner-side sampler (loader.cpp, loader_kernels.hip, DataLoader) against tests/loader_model.py: every row of tests/loader_model_cases.py is
loaded into mz.DataLoader and every sample of its batches is held to the model — the planes (the seven board games: the Python rules models behind
tests/rule_envs.py; Atari: the OBS tag decoded here), the policy, value and reward targets and the
in-game action planes bit for bit, the action planes past a game's end by what every draw satisfies, the loss scale within (N + 16) * 2^-24.

The sampler does not report the rotation it drew.  Rf = the rotations under which the model's planes are the returned planes; a sample passes only if ONE
r in Rf explains the policy of every unrolled step and every in-game action plane.  tests/test_loader_model.py shows on the CPU that the rows' positions are
asymmetric but for a few, that the model agrees with the oracle's loader where both exist, and that the rows tell wrong readings from the model."""
import numpy as np
import pytest

import loader_model as M
import loader_model_cases as C
from test_loader_model import check_batch

pytestmark = pytest.mark.gpu

# per new game one row that also loads real self-play lines of the worker (8 simulations): row -> (planes, policy size, games, cycles)
SELFPLAY = {"gomoku9_mz3": (4, 81, 3, 9 * 86), "hex5_mz5": (4, 25, 3, 9 * 28), "nogo9_mz3": (18, 82, 3, 9 * 82), "havannah4_az": (20, 49, 3, 9 * 38)}


def _selfplay_lines(mz, name):
    cfg = M.Cfg(C.conf_of(name))
    planes, actions, games, cycles = SELFPLAY[name]
    side = 2 * cfg.n - 1 if cfg.game == "havannah" else cfg.n
    gm = C.records(name)[-1].split("GM[")[1].split("]")[0]
    typ = "muzero" if cfg.muzero else "alphazero"
    d = mz.make_desc(gm, planes, side, side, 32, side, side, 1, 1, actions, vh=32, dv=1, type_name=typ)
    env = ":".join(x for x in C.conf_of(name).split(":") if x.startswith("env_"))
    wk = mz.Worker(f"{env}:nn_type_name={typ}:actor_num_simulation=8:zero_num_parallel_games={games}:program_seed=21:nn_file_name=x.pt:actor_resign_threshold=-2", d, mz.generate_weights(d, 21))
    wk.command("start")
    assert wk.run_cycles(cycles) == cycles
    lines = wk.pop_lines()[:games]
    wk.close()
    assert len(lines) == games and all(l.startswith("SelfPlay") and "P[" in l for l in lines)
    return lines


def _load(mz, name, tmp_path, extra=()):
    conf, recs = C.conf_of(name), list(C.records(name)) + list(extra)
    dl = mz.DataLoader(conf)
    dl.initialize()
    if name in C.PER_ROWS:  # the path on which the reference computes the priority sum
        assert dl.load_data_from_file(C.write_file(str(tmp_path / "1.sgf"), [C.bare(r) for r in recs])) == len(recs), mz.last_error()
    else:
        for r in recs:
            assert dl.add_record(r) == 1, mz.last_error()
    m = M.LoaderModel(conf).load(recs)
    assert dl.num_games() == m.num_games() and dl.num_data() == m.num_data()
    cfg, U = m.cfg, m.cfg.unroll
    assert dl.shapes() == (cfg.batch, C.buffers(cfg)[0].shape[1], U * cfg.action_size, (U + 1) * cfg.policy_size, (U + 1) * cfg.value_size, U * cfg.value_size)
    return dl, m


def _missing(m, name, seen):
    """what the row is there for and no batch has sampled yet"""
    out = []
    partial = [g for g, r in enumerate(m.records) if r.tags.get("DLEN") and r.data_range()[0] > 0 and r.data_range()[1] > r.data_range()[0]]
    if partial and not any(g in partial and pos > m.data_range(g)[0] for g, pos in seen):
        out.append("a position past a partial DLEN's start")
    if m.cfg.muzero and not any(pos + m.cfg.unroll > len(m.records[g]) for g, pos in seen):
        out.append("an absorbing step")
    if "swap=" in C.ROWS[name] and not any(g == 0 and pos >= 2 for g, pos in seen):
        out.append("a position after the swap")
    return out


@pytest.mark.parametrize("name", list(C.ROWS))
def test_batches_equal_the_model(mz, tmp_path, name):
    """three batches (more, up to the row's cap, until what the row is there for was sampled) of every row, every sample on every array; in Gomoku and NoGo rows
    at least half of a batch's samples have exactly one feature rotation; in prioritised rows one update_priority with fixed values and a batch after it"""
    extra = _selfplay_lines(mz, name) if name in SELFPLAY else ()
    dl, m = _load(mz, name, tmp_path, extra)
    seen = []
    for it in range(max(3, C.cap(name))):
        bufs = C.buffers(m.cfg)
        dl.sample_data(*bufs)
        check_batch(m, bufs, f"{name} batch {it}")
        if name in C.ROTATED_NEW:
            one = sum(len(m.feature_rotations(int(g), int(pos), f)) == 1 for f, (g, pos) in zip(bufs[0], bufs[6]))
            assert 2 * one >= m.cfg.batch, f"{name} batch {it}: only {one} of {m.cfg.batch} samples pin the rotation"
        seen += [(int(g), int(pos)) for g, pos in bufs[6]]
        if it >= 2 and not _missing(m, name, seen):
            break
    assert not _missing(m, name, seen), f"{name}: never sampled in {it + 1} batches: {_missing(m, name, seen)}"
    if extra:
        first = m.num_games() - len(extra)
        assert any(g >= first for g, _ in seen), "no sample from the worker's own records"
    if name in C.PER_ROWS:
        for k in range(2):
            vals = C.fixed_values(m.cfg, salt=k)
            dl.update_priority(bufs[6], vals)
            m.update_priority(bufs[6], vals)
            bufs = C.buffers(m.cfg)
            dl.sample_data(*bufs)
            check_batch(m, bufs, f"{name} after update_priority {k}")
        assert not np.allclose(bufs[5], 1.0), "importance weights of prioritised replay"


@pytest.mark.parametrize("name", C.FREQUENCY_ROWS)
def test_sampling_frequencies(mz, tmp_path, name):
    """the (game, position) counts of the product's own draws against priority / sum: chi-square <= dof + 5 sqrt(2 dof)"""
    dl, m = _load(mz, name, tmp_path)
    counts = {}
    bufs = C.buffers(m.cfg)
    for _ in range(C.batches_for_frequencies(m)):
        dl.sample_data(*bufs)
        for g, p in bufs[6]:
            counts[(int(g), int(p))] = counts.get((int(g), int(p)), 0) + 1
    stat, dof, bound = C.chi_square(m, counts)
    print(f"{name}: chi-square {stat:.1f}, dof {dof}, bound {bound:.1f}")
    assert stat <= bound, f"chi-square {stat:.1f} with {dof} degrees of freedom, bound {bound:.1f}"
