"""The value-first order of the one-game-per-CU simulation kernel (sim_az_body.h): behind the heads the backup runs at once on the value alone, the walk of
simulation s + 1 starts when it is done, and candidates + expand of simulation s run beside that walk on waves that have no part in it.  The walk joins the
expand where it could see the difference — at the leaf of simulation s, in front of its own leaf, in front of the root noise — so nothing a record can show may
change: records of the default run == records with MZ_NO_SPEC=64 (today's order) == records with both first launch parts in one launch == the oracle's.

The case is BASELINE configs[1]'s network and search (9x9 Go, 6 blocks x 64 channels, n = 400: the sim_kernel<9,9,20,64,2> instance) with 8 games, four on each
of two XCDs: paths of 31 levels on average, helper segments beyond level 16, remembered paths.  The profile's counts keep the test from passing without the
branch under test: they are properties of the search and of the launch's switches, not of timing (no assertion is made on the number of waits).

Each run is a child process (MZ_SIM_PROF and MZ_NO_SPEC are read when the worker first launches; the profile is printed when it closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = 8
CHUNKS = [401, 47]  # a whole move (launches of 1 + 16 + 384 simulations) and the first launches of the next

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import minizero_amd as mz
conf, wseed, chunks, games = json.loads(sys.argv[2])
d = mz.DESCS["c2"]()
wk = mz.Worker(conf, d, mz.generate_weights(d, wseed))
wk.command("start")
for c in chunks:
    assert wk.run_cycles(c) == c
st = wk.stats()
out = {"lines": wk.pop_lines(), "records": wk.peek_records(games), "sim_launches": st["sim_launches"], "leaf_evals": st["leaf_evals"]}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""


def _child(conf, wseed, no_spec):
    env = dict(os.environ, MZ_SIM_PROF="1")
    env.pop("MZ_NO_SPEC", None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf, wseed, CHUNKS, GAMES])], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"value first: (\d+) of (\d+) simulations in the new order; (\d+) walks arrived at the previous simulation's leaf, (\d+) waited there", r.stderr)
    assert m, "no value-first line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["new_order"], out["arrived"], out["waited"] = int(m.group(1)), int(m.group(3)), int(m.group(4))
    out["prof"] = [l for l in r.stderr.splitlines() if "value first" in l or "cand+expand" in l or "heads" in l]
    return out


def test_value_first_keeps_the_records(mz, oracle):
    d, od = mz.DESCS["c2"](), oracle.desc_c2()
    wseed = 0
    w = mz.generate_weights(d, wseed)
    head, tail = mz.CONFIGS["c2"].split("zero_num_parallel_games=")
    conf = head + f"zero_num_parallel_games={GAMES}" + (":" + tail.split(":", 1)[1] if ":" in tail else "") + ":program_seed=1:nn_file_name=x.pt"
    total = sum(CHUNKS)
    og = oracle.OracleGroup(conf + ":zero_num_threads=1", od, w)
    og.cycles(total)
    olines, orecs = og.lines(), og.peek_records(GAMES)

    new = _child(conf + ":zero_num_threads=2", wseed, 0)
    old = _child(conf + ":zero_num_threads=2", wseed, 64)
    one = _child(conf + ":zero_num_threads=2:mz_sim_split=false", wseed, 0)  # slot 1 behind slot 0 in one launch: the join in front of the root noise
    runs = (("default", new), ("MZ_NO_SPEC=64", old), ("mz_sim_split=false", one))
    for name, r in runs:
        print(f"{name}: {r['new_order']} of {r['sims']} simulations in the new order, {r['skipped']} terminal leaves, "
              f"{r['arrived']} walks arrived at the previous leaf, {r['waited']} waited there")
        for l in r["prof"]:
            print("   " + l)
        assert r["sim_launches"] > 0 and r["sims"] == total * GAMES and r["leaf_evals"] == total * GAMES
    for name, r in runs:
        assert r["lines"] == olines, f"{name}: the lines differ from the oracle's"
        for g in range(GAMES):
            assert r["records"][g] == orecs[g], f"{name}, game {g}: the record differs from the oracle's"
    assert new["records"] == old["records"] == one["records"]
    assert new["new_order"] == new["sims"] and new["skipped"] > 0, "the default run does not take the order under test, or never meets a terminal leaf"
    assert new["arrived"] > 0, "no walk ever arrived at the previous simulation's leaf: the join is not exercised"
    assert one["new_order"] == one["sims"]
    assert one["sim_launches"] < new["sim_launches"], "mz_sim_split=false did not put slot 1 behind slot 0 in one launch"
    assert old["new_order"] == 0
