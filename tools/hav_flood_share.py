#!/usr/bin/env python3
"""Havannah: the share of leaves whose win test reaches the flood of the complement.  Plays `moves` moves of 256 games of havannah8x64 on
the host rules (mz_device_env=false: the same leaves as the device rules see — the records of the paths are equal) with MZ_HAV_PROF=1, under which the
host engine counts its win tests, those past the ring's two gates and those that flood; the counts are printed when the process ends.
    MZ_HAV_PROF=1 python tools/hav_flood_share.py [moves] [simulations]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minizero_amd as mz

moves = int(sys.argv[1]) if len(sys.argv) > 1 else 40
sims = int(sys.argv[2]) if len(sys.argv) > 2 else 100
assert os.environ.get("MZ_HAV_PROF"), "set MZ_HAV_PROF=1"
d = mz.DESCS["havannah8x64"]()
conf = mz.CONFIGS["havannah8x64"].replace("actor_num_simulation=400", f"actor_num_simulation={sims}") + ":mz_device_env=false:program_seed=1:nn_file_name=x.pt:actor_resign_threshold=-2"
wk = mz.Worker(conf, d, mz.generate_weights(d, 0))
wk.command("start")
assert wk.run_cycles(moves * (sims + 1)) == moves * (sims + 1)
print(f"{moves} moves of 256 games at n = {sims}, {len(wk.pop_lines())} games finished")
wk.close()
