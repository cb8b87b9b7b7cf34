"""A simulation whose leaf is a terminal position has no children and backs up the game result (ref zero_actor.cpp:80-86), so the per-game simulation
kernels do not run planes, tower and heads for it (sim_az_body.h sim_kernel, sim_wide.inc).  Nothing a record can show may change: the records with the
skip == the records with MZ_NO_SPEC=16 (the network runs at every leaf, as before) == the oracle's, on inputs where terminal leaves really occur, and
the kernel skips exactly the simulations whose leaf the oracle finds terminal.

Each run is a child process (MZ_SIM_PROF and MZ_NO_SPEC are read when the worker first launches; the profile is printed when the worker closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import minizero_amd as mz
conf, args, wseed, cycles = json.loads(sys.argv[2])
d = mz.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
wk = mz.Worker(conf, d, mz.generate_weights(d, wseed))
wk.command("start")
assert wk.run_cycles(cycles) == cycles
st = wk.stats()
out = {"lines": wk.pop_lines(), "sim_launches": st["sim_launches"], "leaf_evals": st["leaf_evals"]}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""

# (configuration, network, program seed, weight seed, games, cycles): small cases of the three rule sets behind sim_kernel whose searches reach the end of the game
CASES = {
    "tictactoe": (None, ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9, 256, 1, "alphazero"), 1, 0, 8, 17 * 120),
    "othello": ("env_game=othello:env_board_size=8:actor_num_simulation=16:zero_num_parallel_games=4",
                ("othello_8x8", 4, 8, 8, 8, 8, 8, 1, 1, 65, 16, 1, "alphazero"), 11, 3, 4, 17 * 70),
    "go": ("env_game=go:env_board_size=9:actor_num_simulation=12:zero_num_parallel_games=5:actor_use_dirichlet_noise=false",
           ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1, "alphazero"), 11, 3, 5, 2600),
}


def _child(conf, args, wseed, cycles, no_spec):
    env = dict(os.environ, MZ_SIM_PROF="1")
    env.pop("MZ_NO_SPEC", None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf, list(args), wseed, cycles])], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_terminal_leaves_skip_the_network(mz, oracle, case):
    conf, args, seed, wseed, games, cycles = CASES[case]
    conf = (conf or mz.CONFIGS["c1"]) + f":program_seed={seed}:nn_file_name=x.pt"
    od = oracle.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12])
    w = mz.generate_weights(mz.make_desc(*args[:10], vh=args[10], dv=args[11], type_name=args[12]), wseed)
    og = oracle.OracleGroup(conf + ":zero_num_threads=1", od, w)
    og.set_trace(True)
    og.cycles(cycles)
    olines = og.lines()
    # the oracle looks at the leaf of cycle c's simulation in cycle c + 1 (the `E` line: an empty candidate list = a terminal leaf), the kernel within the
    # simulation: one more cycle, so that the trace covers the leaves of all `cycles` simulations of every game
    og.cycles(1)
    ev = [l.split(" ") for l in og.trace() if l.startswith("E ")]
    ev = [f for f in ev if int(f[1]) <= cycles]
    assert len(ev) == cycles * games
    terminal = sum(1 for f in ev if f[3] == "cand=")
    print(f"{case}: oracle: {terminal} of {len(ev)} simulations have a terminal leaf ({100.0 * terminal / len(ev):.2f} %), {len(olines)} finished games")
    assert terminal >= 0.02 * len(ev), "the input never takes the branch under test"
    assert len(olines) >= 3

    skip = _child(conf + ":zero_num_threads=2", args, wseed, cycles, 0)
    full = _child(conf + ":zero_num_threads=2", args, wseed, cycles, 16)
    print(f"{case}: kernel: network skipped in {skip['skipped']} of {skip['sims']} simulations; with MZ_NO_SPEC=16 in {full['skipped']} of {full['sims']}")
    for r in (skip, full):
        assert r["sim_launches"] > 0 and r["sims"] == cycles * games and r["leaf_evals"] == cycles * games  # leaf_evals keeps the reference's meaning
    assert skip["lines"] == olines
    assert full["lines"] == olines
    assert skip["skipped"] == terminal
    assert full["skipped"] == 0
