"""Tail help with up to three helpers per game (sim_help.h towerBodyQuad, sim_az_body.h simHelpTail): a finished workgroup that finds no running game of its XCD
without a helper takes slot 2 or 3 of a helped one, and a game whose three slots are claimed runs its towers on four workgroups.  The quad tower is the same
k-ordered chain per output as the solo tower, so nothing a record can show may change: records with help == records with MZ_NO_SPEC=32 (no help) == the oracle's.

The case is tests/test_gpu_tail_help.py's (BASELINE configs[1]'s network and search, MZ_SIM_HELP_MIN=8) with 64 games, eight per XCD: with four per XCD three
finished neighbours for one straggler are rare.  Whether a game gets its three helpers depends on GPU timing; the test FAILS if no simulation ran a quad tower,
and if no game went from pair to quad towers within a launch (the dump counts both).  Observed with 64 games on an MI355X: 68 and 73 of about 27 000 network
simulations on four workgroups, 11 and 15 games that went from pair to quad towers (one stream, 16 streams); both cases passed in each of the two runs made.  A second case runs the bench's mode, mz_rng_streams=16, at the same size.

Each run is a child process (MZ_SIM_PROF, MZ_NO_SPEC and MZ_SIM_HELP_MIN are read when the worker first launches; the profile is printed when it closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = 64
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
    out["helped"] = int(m.group(1)) if m else 0
    m = re.search(r"tail help, quad towers: (\d+) of the (\d+) simulations that ran the network had a quad tower .* (\d+) games went from pair to quad towers", r.stderr)
    out["quad"], out["upgraded"] = (int(m.group(1)), int(m.group(3))) if m else (0, 0)
    out["prof"] = [l for l in r.stderr.splitlines() if "tail help" in l or "idles at the end" in l]
    return out


@pytest.mark.parametrize("streams", [1, 16])
def test_quad_help_keeps_the_records(mz, oracle, streams):
    d, od = mz.DESCS["c2"](), oracle.desc_c2()
    wseed = 0
    w = mz.generate_weights(d, wseed)
    head, tail = mz.CONFIGS["c2"].split("zero_num_parallel_games=")
    conf = head + f"zero_num_parallel_games={GAMES}" + (":" + tail.split(":", 1)[1] if ":" in tail else "") + ":program_seed=1:nn_file_name=x.pt"
    total = sum(CHUNKS)
    og = oracle.OracleGroup(conf + ":zero_num_threads=1" + (f":oracle_throughput_threads={streams}" if streams > 1 else ""), od, w)
    og.cycles(total)
    olines, orecs = og.lines(), og.peek_records(GAMES)

    wconf = conf + (f":mz_rng_streams={streams}" if streams > 1 else "") + ":zero_num_threads=2"
    on = _child(wconf, wseed, 0)
    off = _child(wconf, wseed, 32)
    for name, r in (("help", on), ("MZ_NO_SPEC=32", off)):
        ran = r["sims"] - r["skipped"]
        print(f"{name}: {r['helped']} of the {ran} simulations that ran the network had a helper, {r['quad']} of them three; {r['upgraded']} games went from pair to quad towers; "
              f"{r['skipped']} of {r['sims']} simulations had a terminal leaf")
        for l in r["prof"]:
            print("   " + l)
        assert r["sim_launches"] > 0 and r["sims"] == total * GAMES and r["leaf_evals"] == total * GAMES
    assert on["lines"] == olines and off["lines"] == olines
    for g in range(GAMES):
        assert on["records"][g] == orecs[g], f"game {g}: the record with help differs from the oracle's"
        assert off["records"][g] == orecs[g], f"game {g}: the record without help differs from the oracle's"
    assert on["records"] == off["records"]
    assert off["helped"] == 0 and off["quad"] == 0
    assert on["skipped"] > 0 and on["helped"] > on["quad"] > 0 and on["upgraded"] > 0, "the input never takes the branch under test"
