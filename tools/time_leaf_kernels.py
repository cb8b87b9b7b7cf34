#!/usr/bin/env python3
"""Stand-alone cost of a device rules body per leaf: plays `moves` moves of 256 games in the lock-step mode (mz_sim_kernel=false), where every cycle is one launch of
the game's leaf kernel (one wave per leaf: leaf_kernel<-3> for Hex, leaf_kernel<-2> for Gomoku, leaf_kernel<-4> for NoGo, leaf_kernel<-5> for Havannah — go_dev.hip leaf_kernel<rules argument>), so that a kernel trace of the run holds one duration per cycle, in playing order.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_leaf_kernels.py run hex 100
    python tools/time_leaf_kernels.py report DIR 'leaf_kernel<-3>'
NoGo: `run nogo 70` — a 9x9 game lasts 70 .. 79 moves, so the last third of the run is the late positions (long chains: the most flood rounds).
Havannah: `run havannah 60` — edge size 8 on its 15x15 array; late positions have the large groups (the longest floods, and the ring test's complement flood).
`report` splits the launches of the named kernel into the first, middle and last third of the run (early, middle and late positions) and prints the median and the
mean duration of each."""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMES = {"hex": ("hex_11x11", 11, 4, 121), "gomoku": ("gomoku_15x15", 15, 4, 225), "nogo": ("nogo_9x9", 9, 18, 82),
         "havannah": ("havannah8x8", 15, 20, 225)}  # name, board, planes, actions


def run(game, moves, sims=16, games=256):
    import minizero_amd as mz
    name, n, planes, actions = GAMES[game]
    d = mz.make_desc(name, planes, n, n, 64, n, n, 1, 6, actions)
    conf = f"env_game={game}:actor_resign_threshold=-2:actor_num_simulation={sims}:zero_num_parallel_games={games}:mz_sim_kernel=false:program_seed=1:nn_file_name=x.pt"
    wk = mz.Worker(conf, d, mz.generate_weights(d, 0))
    wk.command("start")
    cycles = moves * (sims + 1)
    assert wk.run_cycles(cycles) == cycles
    st = wk.stats()
    print(f"{game}: {moves} moves of {games} games, {len(wk.pop_lines())} games finished, ms_env {st['ms_env']}")
    wk.close()


def report(directory, kernel):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if kernel in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    k = len(rows) // 3
    for label, part in (("early", rows[:k]), ("middle", rows[k:2 * k]), ("late", rows[2 * k:])):
        ns = [d for _, d in part]
        print(f"{kernel} {label:6s} launches {len(ns):5d} median {statistics.median(ns) / 1e3:7.2f} us mean {statistics.mean(ns) / 1e3:7.2f} us max {max(ns) / 1e3:7.2f} us")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]))
    else:
        report(sys.argv[2], sys.argv[3])
