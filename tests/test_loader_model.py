"""CPU tests of the sampler's model (tests/loader_model.py) and of its case table (tests/loader_model_cases.py): the model against the oracle's loader on the
games both know (the two were derived separately from the reference: agreement is the evidence that the model read the promotions correctly), the Atari
planes three ways, the power of the cases against deliberately wrong readings, the conditions the GPU test (tests/test_gpu_loader_model.py) relies on,
and the sampling frequencies of the oracle's loader.

Targets and action planes are compared as float32 bit patterns.  The loss scale is compared with the relative bound (N + 16) * 2^-24, N the positions
summed: the reference's float sum of N positive terms is within (N - 1) * 2^-24 of the exact one, its pow() results, the division and the product add a
few ulp each, and alpha, beta <= 1 do not amplify a relative error."""
import numpy as np
import pytest

import loader_model as M
import loader_model_cases as C
from atari_synth import AtariSynth


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _model(name, wrong=None):
    return M.LoaderModel(C.conf_of(name), wrong).load(C.records(name))


def _oracle_loader(oracle, name, tmp_path):
    ol = oracle.OracleLoader(C.conf_of(name))
    ol.load_data_from_file(C.write_file(str(tmp_path / "1.sgf"), C.records(name)))
    return ol


def _positions(m):
    return [(g, p) for g in range(m.num_games()) for p in range(m.data_range(g)[0], m.data_range(g)[1] + 1)]


def check_batch(m, bufs, tag, planes=None):
    """every sample of one batch against the model; `planes`(g, pos, features) -> the rotations the planes allow (None: the model's own planes)"""
    feats, act, pol, val, rew, scale, si = bufs
    for b, (g, pos) in enumerate(si):
        g, pos = int(g), int(pos)
        where = f"{tag}, sample {b}, (game {g}, position {pos})"
        a, z = m.data_range(g)
        assert a <= pos <= z, f"{where}: outside the data range {a}-{z}"
        rots = m.feature_rotations(g, pos, feats[b]) if planes is None else planes(g, pos, feats[b])
        assert rots, f"{where}: features are the model's planes under no rotation"
        rot, bad = m.explain(g, pos, rots, act[b], pol[b], val[b], rew[b])
        assert not bad, f"{where}: {'; '.join(bad)}"
        want = float(m.loss_scale(g, pos))
        assert abs(float(scale[b]) - want) <= m.scale_bound() * abs(want), f"{where}: loss_scale {scale[b]!r}, the model has {want!r} (bound {m.scale_bound():.3g} relative)"


@pytest.mark.parametrize("name", C.ORACLE_GAMES)
def test_model_equals_the_oracle(oracle, tmp_path, name):
    """three batches of the oracle's loader, then one update_priority with fixed values on both sides and another batch: policy, value, reward and in-game
    action planes bit for bit, loss scales within the bound; the planes too: Atari's from the OBS tag, the board games' from the rules models"""
    m, ol = _model(name), _oracle_loader(oracle, name, tmp_path)
    assert ol.num_games() == m.num_games() and ol.num_data() == m.num_data() > 0
    for it in range(4):
        bufs = C.buffers(m.cfg)
        ol.sample_data(*bufs)
        check_batch(m, bufs, f"{name} batch {it}")
        if it == 2:
            vals = C.fixed_values(m.cfg)
            ol.update_priority(bufs[6], vals)
            m.update_priority(bufs[6], vals)
    if name in C.PER_ROWS:
        assert not np.allclose(bufs[5], 1.0), "importance weights of prioritised replay"


@pytest.mark.parametrize("name", C.ATARI_ROWS)
def test_atari_planes_three_ways(oracle, tmp_path, name):
    """for every position of the data ranges: the planes decoded from OBS are the planes of AtariSynth(SD) replayed; and the oracle's sampled features are both"""
    m = _model(name)
    for g, rec in enumerate(m.records):
        a, z = m.data_range(g)
        env = AtariSynth(int(rec.tags["SD"]), m.cfg.episode_length)
        for pos in range(z + 1):
            if pos >= a:
                assert all(s is not None for s in m.screens(g)[max(0, pos - 7):pos + 1]), f"game {g}, position {pos}: OBS does not hold the screens"
                assert np.array_equal(_bits(m.planes(g, pos)), _bits(env.features())), f"game {g}, position {pos}: OBS planes differ from the replay of SD"
            if pos < len(rec):
                env.act(rec.actions[pos])
    ol = _oracle_loader(oracle, name, tmp_path)
    seen = set()
    for it in range(3):
        bufs = C.buffers(m.cfg)
        ol.sample_data(*bufs)
        for f, (g, pos) in zip(bufs[0], bufs[6]):
            assert np.array_equal(_bits(f), _bits(m.planes(int(g), int(pos)))), f"batch {it}: the oracle's planes of (game {g}, position {pos}) differ from OBS"
            assert np.array_equal(_bits(f), _bits(m.atari_planes(int(g), int(pos), replay=True)))
            seen.add((int(g), int(pos)))
    assert len(seen) >= 10


# which rows a wrong reading concerns, and what is compared there
_BOARD_ROT = [n for n in C.ROWS if M.Cfg(C.conf_of(n)).game in M.ROTATING]
_BOARD_ROT_MZ = [n for n in _BOARD_ROT if M.Cfg(C.conf_of(n)).muzero]
CONCERNS = {"policy_inverse_rotation": (_BOARD_ROT, "policy"), "policy_not_rotated": (_BOARD_ROT, "policy"), "counts_not_permuted": (_BOARD_ROT, "policy"),
            "action_not_rotated": (_BOARD_ROT_MZ, "action"), "nstep_off_by_one": (C.ATARI_ROWS, "value"), "l_cut_ignored": (C.ATARI_ROWS, "value"),
            "bootstrap_at_l": (C.ATARI_ROWS, "value"), "screens_from_start": (C.ATARI_ROWS, "planes"),
            "value_of_mover": ([n for n in C.ROWS if n not in C.ATARI_ROWS], "value"), "priority_without_text": (C.PER_ROWS, "update")}


def _differs(name, wrong, what):
    """the number of (position, rotation) samples of the row on which the wrong reading gives another array than the model"""
    m, w = _model(name), _model(name, wrong)
    n = 0
    if what == "update":
        rng = np.random.default_rng(1)
        pos = _positions(m)
        si = np.array([pos[i] for i in rng.choice(len(pos), m.cfg.batch)], np.int32)
        for x in (m, w):
            x.update_priority(si, C.fixed_values(m.cfg))
        return sum(not np.array_equal(_bits(m.value(g, p)), _bits(w.value(g, p))) or m.prio[g][p] != w.prio[g][p] for g, p in pos)
    for g, p in _positions(m):
        if what == "value":
            n += not np.array_equal(_bits(m.value(g, p)), _bits(w.value(g, p)))
        elif what == "planes":
            n += not np.array_equal(_bits(m.planes(g, p)), _bits(w.planes(g, p)))
        else:
            f = (lambda x, r: x.policy(g, p, r)) if what == "policy" else (lambda x, r: x.action_plane(g, p, r))
            n += sum(not np.array_equal(f(m, r), f(w, r)) for r in m.cfg.rotations)
    return n


def test_the_cases_tell_every_wrong_reading_from_the_model():
    """each deliberately wrong variant differs from the model on at least one sample of EVERY row that concerns it (more than the one the issue asks for)"""
    assert set(CONCERNS) == set(M.WRONG)
    report = {}
    for wrong, (rows, what) in CONCERNS.items():
        assert rows, wrong
        report[wrong] = {name: _differs(name, wrong, what) for name in rows}
    for wrong, per_row in report.items():
        print(f"{wrong}: detected on {sum(per_row.values())} samples of {len(per_row)} rows")
    missed = {w: [n for n, k in per_row.items() if k == 0] for w, per_row in report.items()}
    # what the row of 6-step games cannot show: no life is lost in so short a game, and its OBS holds every screen (start and end aligned alike)
    allowed = {w: {"atari_n1_short"} for w in ("l_cut_ignored", "bootstrap_at_l", "screens_from_start")}
    for w, rows in missed.items():
        assert set(rows) <= allowed.get(w, set()), f"{w} passes unnoticed on {rows}"
        assert len(rows) < len(CONCERNS[w][0]), f"{w} is detected nowhere"


@pytest.mark.parametrize("name", C.ROTATED_NEW)
def test_few_positions_are_symmetric(name):
    """at most 1 position in 10 of the data ranges has fewer than 8 distinct rotations of its planes: the joint rotation rule of the GPU test then pins the
    rotation of the policy and of the action planes on at least half of any batch, short of a sampler that prefers the symmetric ones"""
    m = _model(name)
    pos = _positions(m)
    sym = [(g, p) for g, p in pos if len({m.planes(g, p, r).tobytes() for r in range(8)}) < 8]
    assert 10 * len(sym) <= len(pos), f"{len(sym)} of {len(pos)} positions are symmetric: {sym}"


@pytest.mark.parametrize("name", [n for n in C.ROWS if C.spec_of(n)["kind"] != "oracle"])
def test_written_p_tags_have_ties_single_entries_and_gaps(name):
    tie, single, none = C.p_tag_kinds(C.records(name))
    assert tie and single and none, (tie, single, none)
    recs = [M.Record(r) for r in C.records(name)]
    assert all(r.ok for r in recs)
    assert any(r.tags.get("DLEN") and r.data_range()[0] > 0 for r in recs), "no game with a partial DLEN"
    cfg = M.Cfg(C.conf_of(name))
    if cfg.muzero:
        assert any(len(r) < cfg.unroll for r in recs), "no game shorter than the unrolling"
        assert all(r.info(i, "V") and r.info(i, "R") == "0" for r in recs for i in range(len(r)))
    if cfg.game == "hex" or name == "havannah4_az":
        assert recs[0].actions[0] == recs[0].actions[1], "the first record does not take the swap"


@pytest.mark.parametrize("name", [n for n in C.ROWS if C.spec_of(n)["kind"] == "oracle"])
def test_self_play_p_tags_have_single_and_several_entries(name):
    """the oracle's self-play writes what its search found: ties are left to the written rows, but every row has tags of one entry and tags of several"""
    tags = [t for r in C.records(name) for t in C.P_TAG.findall(r)]
    assert any("," not in t for t in tags) and sum("," in t for t in tags) >= 10


def test_atari_rows_hold_what_they_are_there_for():
    """L tags with lives > 0 inside an n-step window, a bootstrap index on an L step, an intermediate sequence whose OBS holds only the tail, a game shorter
    than 8 steps, both discounts, n-step 1, 3 and 5, alpha 0.5 and 1.0, beta 0.4 and 1.0 — on positions of the data ranges"""
    seen = {k: set() for k in ("l_in_window", "bootstrap_on_l", "tail_only", "short", "discount", "n_step", "alpha", "beta")}
    for name in C.ATARI_ROWS:
        m = _model(name)
        assert name in C.PER_ROWS
        for k, v in (("discount", m.cfg.discount), ("n_step", m.cfg.n_step), ("alpha", m.cfg.alpha), ("beta", m.cfg.beta)):
            seen[k].add(round(float(v), 3))
        for g, rec in enumerate(m.records):
            lives = {i: int(rec.info(i, "L")) for i in range(len(rec)) if rec.info(i, "L")}
            a, z = m.data_range(g)
            for pos in range(a, z + 1):
                if any(lives.get(i, 0) > 0 for i in range(pos, min(pos + m.cfg.n_step, len(rec)))):
                    seen["l_in_window"].add(name)
                if pos + m.cfg.n_step in lives:
                    seen["bootstrap_on_l"].add(name)
            frames = sum(s is not None for s in m.screens(g))
            if a > 0 and frames < len(rec) + 1:
                assert all(s is None for s in m.screens(g)[:len(rec) + 1 - frames]), "the screens are the last ones"
                seen["tail_only"].add(name)
            if len(rec) < 8:
                seen["short"].add(name)
    assert {"atari_n3", "atari_n5"} <= seen["l_in_window"] and {"atari_n3", "atari_n5"} <= seen["bootstrap_on_l"], seen
    assert seen["tail_only"] and seen["short"], seen
    assert seen["discount"] == {0.997, 0.9} and seen["n_step"] == {1, 3, 5} and seen["alpha"] == {0.5, 1.0} and seen["beta"] == {0.4, 1.0}, seen


def test_parser_reads_escapes_tags_and_selfplay_lines():
    r = M.Record("SelfPlay false 3 3 1 (;GM[x]SZ[4]C[a\\]b]RE[-1]DLEN[1-2];B[3]P[3:2,1:2]V[0.5]R[0];W[16]L[2];B[0]R[1]) #")
    assert r.ok and r.tags == {"GM": "x", "SZ": "4", "C": "a]b", "RE": "-1", "DLEN": "1-2"} and r.actions == [3, 16, 0] and r.data_range() == (1, 2)
    assert r.moves[0][2] == {"P": "3:2,1:2", "V": "0.5", "R": "0"} and r.moves[1] == ["W", 16, {"L": "2"}] and r.info(2, "V") == ""
    assert not M.Record("(;GM[x];B[1]").ok and M.Record("(;GM[x];B[1];W[2])").data_range() == (0, 1) and M.Record("(;GM[x])").data_range() == (0, 0)
    # std::stof rounds the decimal text once; the nearest double of this text lies on the other side of a float32 tie
    assert M.stof("0.1") == np.float32(0.1) and M.stof("16777217.0000000001") == np.float32(16777218) and M.to_string(np.float32(1) / np.float32(3)) == "0.333333"


@pytest.mark.parametrize("name", C.FREQUENCY_ROWS)
def test_oracle_sampling_frequencies(oracle, tmp_path, name):
    """the (game, position) counts of the oracle's loader against priority / sum: chi-square <= dof + 5 sqrt(2 dof)"""
    m, ol = _model(name), _oracle_loader(oracle, name, tmp_path)
    counts = {}
    bufs = C.buffers(m.cfg)
    for _ in range(C.batches_for_frequencies(m)):
        ol.sample_data(*bufs)
        for g, p in bufs[6]:
            counts[(int(g), int(p))] = counts.get((int(g), int(p)), 0) + 1
    stat, dof, bound = C.chi_square(m, counts)
    assert stat <= bound, f"chi-square {stat:.1f} with {dof} degrees of freedom, bound {bound:.1f}"
    print(f"{name}: chi-square {stat:.1f}, dof {dof}, bound {bound:.1f}")
