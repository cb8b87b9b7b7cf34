"""What the GPU tests of the board games without an oracle (test_gpu_gomoku.py, test_gpu_hex.py, test_gpu_nogo.py, test_gpu_havannah.py) share: the worker's
three execution paths held to each other, and a worker in a process of its own with the simulation kernels' profile dump (MZ_SIM_PROF) read back."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {"sim": "", "lockstep_device": ":mz_sim_kernel=false", "lockstep_host": ":mz_device_env=false"}
NO_RESIGN = ":actor_resign_threshold=-2"
GUMBEL = ":actor_use_dirichlet_noise=false:actor_use_gumbel=true:actor_use_gumbel_noise=true:actor_gumbel_sample_size=8"


def check_path_stats(st, path, cycles, expect_sim=True):
    if path == "sim" and expect_sim:
        assert st["sim_launches"] > 0 and st["sim_cycles"] > cycles // 2, ("the per-game simulation kernel did not run", st)
    else:
        assert st["sim_launches"] == 0, (path, st)
    if path != "lockstep_host":
        assert st["ms_env"] == 0, (path, "the device rules were not resident", st)
    else:
        assert st["ms_env"] > 0, st


def run_paths(mz, conf, d, w, games, cycles, paths=("sim", "lockstep_device", "lockstep_host"), expect_sim=True):
    """The same configuration on each of `paths`: finished lines and the records as they stand are byte-identical; returns the first path's."""
    out = {}
    for path in paths:
        wk = mz.Worker(conf + PATHS[path], d, w)
        wk.command("start")
        assert wk.run_cycles(cycles) == cycles
        check_path_stats(wk.stats(), path, cycles, expect_sim)
        out[path] = (wk.pop_lines(), wk.peek_records(games))
        wk.close()
    first = out[paths[0]]
    for path in paths[1:]:
        assert out[path][0] == first[0], f"{path}: finished records differ from {paths[0]}'s"
        assert out[path][1] == first[1], f"{path}: records as they stand differ from {paths[0]}'s"
    return first


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
out = {"lines": wk.pop_lines(), "records": wk.peek_records(int(sys.argv[3])), "sim_launches": st["sim_launches"]}
wk.close()
print("RESULT " + json.dumps(out), flush=True)
"""


def child(conf, args, wseed, cycles, games, no_spec):
    env = dict(os.environ, MZ_SIM_PROF="1")
    env.pop("MZ_NO_SPEC", None)
    if no_spec:
        env["MZ_NO_SPEC"] = str(no_spec)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps([conf, list(args), wseed, cycles]), str(games)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"worker process failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    m = re.search(r"network skipped in (\d+) of (\d+) simulations", r.stderr)
    assert m, "no terminal-leaf line in the MZ_SIM_PROF dump:\n" + r.stderr[-4000:]
    out["skipped"], out["sims"] = int(m.group(1)), int(m.group(2))
    return out
