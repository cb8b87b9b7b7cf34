"""Lending in the one-game-per-CU simulation kernel (sim_help.h, sim_az_body.h): a game that is ahead of another game of its XCD computes half of ONE tower of
that game — it takes the offer the slower game opens at every simulation — and goes on with its own simulation.  The lent tower is the pair tower of the tail
help, the same k-ordered chain per output as the solo tower, so nothing a record can show may change: records with lending == records with MZ_NO_SPEC=256 (no
lending) == records with MZ_NO_SPEC=32 (no help at all) == the oracle's.

The case is the one of test_gpu_tail_help.py: BASELINE configs[1]'s network and search with 32 games, four per XCD, MZ_SIM_HELP_MIN=8 (launches of >= 8
simulations help), and MZ_SIM_LEND_LEAD=1: a game lends as soon as it is one simulation ahead.  Whether a given game lends depends on GPU timing; the test fails
if fewer than 1 % of the simulations that ran the network had a lent tower (a condition on the input, not a measurement).

A second case has 64 games, eight per XCD (the input of test_gpu_quad_help.py), so that tail helpers, quad towers and volunteers meet in one launch — among them
the finished workgroup that claims a slot beside a taken offer and has to skip the volunteer's command.  With a lead of 1 the games end so close together that
hardly a game gets its three helpers (2 to 13 quad towers in the runs made), so this case runs with the default lead, MZ_SIM_LEND_LEAD=16, and FAILS unless the
run had lent towers (at least 1 % again), tail helpers' pair towers, quad towers, and a game that went from pair to quad towers within a launch.  Observed on an
MI355X in three runs: 747 to 772 lent towers of about 27 400 network simulations (2.7 to 2.8 %), 389 to 428 with a tail helper, 21 to 30 of them quad towers, 7 to
10 games that went from pair to quad.

A time-out of any wait of the protocol raises the pool's error flag, which the worker checks at every cycle: a run whose flag is not 0 fails its child process.
Each run is a child process (MZ_SIM_PROF, MZ_NO_SPEC, MZ_SIM_HELP_MIN and MZ_SIM_LEND_LEAD are read when the worker first launches; the profile is printed when
it closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = [401, 17 + 30]  # a whole move (launches of 1 + 16 + 384 simulations) and the first launches of the next

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import minizero_amd as mz
conf, wseed, chunks, games = json.loads(sys.argv[2])
d = mz.DESCS["c2"]()
wk = mz.Worker(conf, d, mz.generate_weights(d, wseed))
wk.command("start")
for c in chunks:
    assert wk.run_cycles(c) == c  # (raises when the pool's error flag is set)
st = wk.stats()
out = {"lines": wk.pop_lines(), "records": wk.peek_records(games), "sim_launches": st["sim_launches"], "leaf_evals": st["leaf_evals"], "lanes": wk.lanes()}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""


def _child(conf, wseed, games, no_spec, lead=1):
    env = dict(os.environ, MZ_SIM_PROF="1", MZ_SIM_HELP_MIN="8", MZ_SIM_LEND_LEAD=str(lead))
    env.pop("MZ_NO_SPEC", None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf, wseed, CHUNKS, games])], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"lending: (\d+) of the (\d+) simulations that ran the network had a tower lent", r.stderr)
    out["lent"] = int(m.group(1)) if m else 0
    m = re.search(r"tail help: (\d+) of the (\d+) simulations that ran the network had a pair tower", r.stderr)
    out["pair"] = int(m.group(1)) if m else 0
    m = re.search(r"tail help, quad towers: (\d+) of the (\d+) simulations that ran the network had a quad tower .* (\d+) games went from pair to quad towers", r.stderr)
    out["quad"], out["upgraded"] = (int(m.group(1)), int(m.group(3))) if m else (0, 0)
    out["prof"] = [l for l in r.stderr.splitlines() if "tail help" in l or "lending" in l or "idles at the end" in l]
    return out


def _conf(mz, games):
    head, tail = mz.CONFIGS["c2"].split("zero_num_parallel_games=")
    return head + f"zero_num_parallel_games={games}" + (":" + tail.split(":", 1)[1] if ":" in tail else "") + ":program_seed=1:nn_file_name=x.pt"


def _oracle(mz, oracle, games, wseed):
    w = mz.generate_weights(mz.DESCS["c2"](), wseed)
    og = oracle.OracleGroup(_conf(mz, games) + ":zero_num_threads=1", oracle.desc_c2(), w)
    og.cycles(sum(CHUNKS))
    return og.lines(), og.peek_records(games)


def _report(name, r, games):
    ran = r["sims"] - r["skipped"]
    print(f"{name}: {r['lent']} of the {ran} simulations that ran the network had a lent tower ({100.0 * r['lent'] / max(1, ran):.2f} %), {r['pair']} a tail helper's "
          f"(quad: {r['quad']}, {r['upgraded']} games went from pair to quad towers); {r['skipped']} of {r['sims']} simulations had a terminal leaf")
    for l in r["prof"]:
        print("   " + l)
    total = sum(CHUNKS)
    assert r["sim_launches"] > 0 and r["sims"] == total * games and r["leaf_evals"] == total * games


def test_lending_keeps_the_records(mz, oracle):
    games, wseed = 32, 0
    olines, orecs = _oracle(mz, oracle, games, wseed)
    conf = _conf(mz, games) + ":zero_num_threads=2"
    on = _child(conf, wseed, games, 0)
    off = _child(conf, wseed, games, 256)
    none = _child(conf, wseed, games, 32)
    for name, r in (("lending", on), ("MZ_NO_SPEC=256", off), ("MZ_NO_SPEC=32", none)):
        _report(name, r, games)
        assert r["lines"] == olines, f"{name}: the popped lines differ from the oracle's"
        for g in range(games):
            assert r["records"][g] == orecs[g], f"{name}, game {g}: the record differs from the oracle's"
    assert on["records"] == off["records"] == none["records"] and on["lines"] == off["lines"] == none["lines"]
    assert on["leaf_evals"] == off["leaf_evals"] == none["leaf_evals"] and on["sims"] == off["sims"] == none["sims"] and on["skipped"] == off["skipped"] == none["skipped"]
    assert off["lent"] == 0 and none["lent"] == 0 and none["pair"] == 0
    assert on["skipped"] > 0 and on["lent"] >= 0.01 * (on["sims"] - on["skipped"]), "the input never takes the branch under test"


def test_lending_beside_tail_helpers_and_quad_towers(mz, oracle):
    games, wseed = 64, 0
    olines, orecs = _oracle(mz, oracle, games, wseed)
    on = _child(_conf(mz, games) + ":zero_num_threads=2", wseed, games, 0, lead=16)
    _report("lending, 64 games, lead 16", on, games)
    assert on["lines"] == olines
    for g in range(games):
        assert on["records"][g] == orecs[g], f"game {g}: the record with lending differs from the oracle's"
    assert on["lent"] >= 0.01 * (on["sims"] - on["skipped"]), "the input never takes the branch under test"
    assert on["pair"] > on["quad"] > 0 and on["upgraded"] > 0, "the input never has volunteers, tail helpers and quad towers in one run"
