"""Tail help of the one-game-per-CU simulation kernel (sim_help.h, sim_az_body.h): a workgroup whose game has finished the launch's simulations computes half of
the tower of a game of its XCD that is still running.  The pair tower is the same k-ordered chain per output as the solo tower, so nothing a record can show may
change: records with help == records with MZ_NO_SPEC=32 (no help) == the oracle's.

The case is BASELINE configs[1]'s network and search (9x9 Go, 6 blocks x 64 channels, n = 400: the sim_kernel<9,9,20,64,2> instance, the only one that helps)
with 32 games, four per XCD.  With untrained weights about a fifth of the simulations end at a terminal leaf (two passes) and skip the network, so the games of
a launch finish at different times and the early ones find a straggler to help.  Whether a given game is helped depends on GPU timing; MZ_SIM_HELP_MIN=8 makes
helping eager (launches of >= 8 simulations help, a game is claimed while it has >= 2 left), and the test fails if no simulation took the branch.

Each run is a child process (MZ_SIM_PROF, MZ_NO_SPEC and MZ_SIM_HELP_MIN are read when the worker first launches; the profile is printed when it closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = 32
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
    assert wk.run_cycles(c) == c
st = wk.stats()
out = {"lines": wk.pop_lines(), "records": wk.peek_records(games), "sim_launches": st["sim_launches"], "leaf_evals": st["leaf_evals"], "lanes": wk.lanes()}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""


def _child(conf, wseed, no_spec):
    env = dict(os.environ, MZ_SIM_PROF="1", MZ_SIM_HELP_MIN="8")
    env.pop("MZ_NO_SPEC", None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf, wseed, CHUNKS, GAMES])], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"tail help: (\d+) of the (\d+) simulations that ran the network had a pair tower", r.stderr)
    out["pair"] = int(m.group(1)) if m else 0
    out["prof"] = [l for l in r.stderr.splitlines() if "tail help" in l or "idles at the end" in l]
    return out


def test_tail_help_keeps_the_records(mz, oracle):
    d, od = mz.DESCS["c2"](), oracle.desc_c2()
    wseed = 0
    w = mz.generate_weights(d, wseed)
    head, tail = mz.CONFIGS["c2"].split("zero_num_parallel_games=")
    conf = head + f"zero_num_parallel_games={GAMES}" + (":" + tail.split(":", 1)[1] if ":" in tail else "") + ":program_seed=1:nn_file_name=x.pt"
    total = sum(CHUNKS)
    og = oracle.OracleGroup(conf + ":zero_num_threads=1", od, w)
    og.cycles(total)
    olines, orecs = og.lines(), og.peek_records(GAMES)

    on = _child(conf + ":zero_num_threads=2", wseed, 0)
    off = _child(conf + ":zero_num_threads=2", wseed, 32)
    for name, r in (("help", on), ("MZ_NO_SPEC=32", off)):
        ran = r["sims"] - r["skipped"]
        print(f"{name}: {r['pair']} of the {ran} simulations that ran the network had a pair tower ({100.0 * r['pair'] / max(1, ran):.2f} %); "
              f"{r['skipped']} of {r['sims']} simulations had a terminal leaf")
        for l in r["prof"]:
            print("   " + l)
        assert r["sim_launches"] > 0 and r["sims"] == total * GAMES and r["leaf_evals"] == total * GAMES
    assert on["lines"] == olines and off["lines"] == olines
    for g in range(GAMES):
        assert on["records"][g] == orecs[g], f"game {g}: the record with help differs from the oracle's"
        assert off["records"][g] == orecs[g], f"game {g}: the record without help differs from the oracle's"
    assert on["records"] == off["records"]
    assert off["pair"] == 0
    assert on["skipped"] > 0 and on["pair"] > 0 and on["pair"] >= 0.01 * (on["sims"] - on["skipped"]), "the input never takes the branch under test"
