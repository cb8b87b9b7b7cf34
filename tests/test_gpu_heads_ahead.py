"""The heads of sim_kernel<9,9,20,64,2> with their operands delivered ahead of the chains (net_body.h headsBodyAhead): the small launch-invariant weights in an LDS
block staged once per launch, the policy FC / value FC1 columns requested at the heads' entry, every x operand an LDS read at an immediate offset.  The chains,
their order and their fmaf are those of headsBody, so nothing a record can show may change: lines and records of the default run == MZ_NO_SPEC=512 (headsBody on
the same build) == the oracle's — on the synthetic weights, on sharpened ones (logits hundreds apart, saturating values), over a weight swap between two moves
(what the per-launch staging is for) and with the LDS block refused by the launch (the fallback a shape without room for it takes).

The MZ_SIM_PROF dump's count of simulations that ran the new heads keeps the tests from passing without the branch under test; it is a property of the launch's
switches, not of timing.  All runs: BASELINE configs[1]'s network and search (n = 400) on 8 games.  Each run is a child process (MZ_NO_SPEC, MZ_SIM_PROF and
MZ_SIM_HEADS_LDS are read when the worker launches; the profile is printed when it closes)."""
import json
import os
import re
import subprocess
import sys

import pytest

from helpers import sharpen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = 8
CHUNKS = [401, 47]  # a whole move (launches of 1 + 16 + 384 simulations) and the first launches of the next

CHILD = r"""
import json, os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import minizero_amd as mz
from helpers import sharpen
conf, wseed, gain, steps, games = json.loads(sys.argv[2])
d = mz.DESCS["c2"]()
def weights(seed):
    w = mz.generate_weights(d, seed)
    return sharpen(d, w, *gain) if gain else w
wk = mz.Worker(conf, d, weights(wseed))
wk.command("start")
for kind, arg in steps:
    if kind == "run":
        assert wk.run_cycles(arg) == arg
    else:  # ("load", [file, seed]): the caller has read the file and hands the content over, as tests/test_gpu_iteration.py's via="blob" does
        f, seed = arg
        from minizero_amd.export_weights import write_mzw
        write_mzw(f[:-3] + ".mzw", d, weights(seed))
        d2, w2 = mz.read_weights_once(f)
        wk.load_model(f, d2, w2)
st = wk.stats()
out = {"lines": wk.pop_lines(), "records": wk.peek_records(games), "sim_launches": st["sim_launches"], "leaf_evals": st["leaf_evals"]}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""


def _conf(mz, extra=""):
    head, tail = mz.CONFIGS["c2"].split("zero_num_parallel_games=")
    return head + f"zero_num_parallel_games={GAMES}" + (":" + tail.split(":", 1)[1] if ":" in tail else "") + extra + ":program_seed=1:nn_file_name=x.pt"


def _child(conf, wseed, gain, steps, no_spec=0, env_extra=None):
    env = dict(os.environ, MZ_SIM_PROF="1")
    for k in ("MZ_NO_SPEC", "MZ_SIM_HEADS_LDS"):
        env.pop(k, None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf + ":zero_num_threads=2", wseed, gain, steps, GAMES])], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"heads ahead: (\d+) of the (\d+) simulations that ran the network", r.stderr)
    assert m, "no heads-ahead line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["ahead"], out["ran"] = int(m.group(1)), int(m.group(2))
    out["prof"] = [l for l in r.stderr.splitlines() if "heads" in l]
    return out


_ORACLE = {}


def _oracle_run(mz, oracle, conf, gain, steps, tmp=None):
    """lines and records of the oracle for the same weights and steps; computed once per (gain, steps) and shared"""
    key = json.dumps([conf, gain, steps])
    if key not in _ORACLE:
        d, od = mz.DESCS["c2"](), oracle.desc_c2()

        def weights(seed):
            w = mz.generate_weights(d, seed)
            return sharpen(d, w, *gain) if gain else w
        og = oracle.OracleGroup(conf + ":zero_num_threads=1", od, weights(0))
        for kind, arg in steps:
            if kind == "run":
                assert og.cycles(arg) == arg
            else:
                og.command("load_model " + arg[0], weights(arg[1]))
        _ORACLE[key] = (og.lines(), og.peek_records(GAMES))
    return _ORACLE[key]


def _same_as_oracle(name, r, olines, orecs, total):
    print(f"{name}: new heads in {r['ahead']} of {r['ran']} simulations that ran the network, {r['skipped']} terminal leaves of {r['sims']}")
    for l in r["prof"]:
        print("   " + l)
    assert r["sim_launches"] > 0 and r["sims"] == total * GAMES and r["leaf_evals"] == total * GAMES and r["ran"] == r["sims"] - r["skipped"]
    assert r["lines"] == olines, f"{name}: the lines differ from the oracle's"
    for g in range(GAMES):
        assert r["records"][g] == orecs[g], f"{name}, game {g}: the record differs from the oracle's"


def _three_way(mz, oracle, conf, gain):
    steps = [["run", c] for c in CHUNKS]
    olines, orecs = _oracle_run(mz, oracle, conf, gain, steps)
    new = _child(conf, 0, gain, steps)
    old = _child(conf, 0, gain, steps, no_spec=512)
    for name, r in (("default", new), ("MZ_NO_SPEC=512", old)):
        _same_as_oracle(name, r, olines, orecs, sum(CHUNKS))
    assert new["lines"] == old["lines"] and new["records"] == old["records"]
    assert new["ahead"] == new["sims"] - new["skipped"] > 0, "the default run does not take the heads under test in every simulation that ran the network"
    assert old["ahead"] == 0, "MZ_NO_SPEC=512 did not switch the new heads off"
    return new


def test_synthetic_weights(mz, oracle):
    """generate_weights(c2, 0): default == MZ_NO_SPEC=512 == oracle; the run meets terminal leaves, so both sides of the skip pass the barriers beside the new body"""
    new = _three_way(mz, oracle, _conf(mz), None)
    assert new["skipped"] > 0, "the run never meets a terminal leaf"


def test_sharpened_weights(mz, oracle):
    """sharpen(1024, 8), no resignation: the regime of SHARP_SEARCHES["go9_6bx64_p1024_v8"]"""
    _three_way(mz, oracle, _conf(mz, ":actor_resign_threshold=-2"), [1024, 8])


def test_weight_swap_between_two_moves(mz, oracle, tmp_path):
    """seed 0, one move, seed 1 handed over as a blob, one move: the LDS block is staged per launch, so the second move's heads read the new weights"""
    f = os.path.join(str(tmp_path), "weight_iter_1.pt")
    steps = [["run", 401], ["load", [f, 1]], ["run", 401]]
    conf = _conf(mz)
    olines, orecs = _oracle_run(mz, oracle, conf, None, steps)
    r = _child(conf, 0, None, steps)
    _same_as_oracle("swap", r, olines, orecs, 802)
    assert r["ahead"] == r["ran"] > 0
    assert all("EV[weight_iter_1.pt]" in rec for rec in r["records"])


def test_lds_fallback(mz, oracle):
    """MZ_SIM_HEADS_LDS=0: the launch leaves the block out, as one without room for it does (heads_lds = 0 in the argument block): headsBody, the same records"""
    steps = [["run", c] for c in CHUNKS]
    conf = _conf(mz)
    olines, orecs = _oracle_run(mz, oracle, conf, None, steps)
    r = _child(conf, 0, None, steps, env_extra={"MZ_SIM_HEADS_LDS": "0"})
    _same_as_oracle("MZ_SIM_HEADS_LDS=0", r, olines, orecs, sum(CHUNKS))
    assert r["ahead"] == 0
