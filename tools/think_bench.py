"""Wall time of one think() from the empty board through the per-actor surface (mz_manual_step=true), per actor_mcts_think_batch_size.
One JSON line per batch size: {"tag", "board", "n", "B", "ms": [one per run], "steps", "walks", "queries"}.  The time runs from mz_worker_reset_search to the
cycle that completes the search (the call returns when the device has finished).  B = 1 runs on the per-game simulation kernel where it has room for n (its LDS tables grow with n: n = 1600 does not fit) and
lock-step otherwise (--b1-extra :mz_sim_kernel=false).  Another build of the library is measured by pointing MZ_LIBMZGPU at it (a build
from before the batched think ignores the key: measure it with --B 1).

    python tools/think_bench.py --board 9 --n 1600 --B 1,8,16,32,64 --runs 5 --tag new

--tree adds "tree_ms": the wall time of one read-out of the visited tree (Worker.tree: the read-out kernel twice, for the size and for the entries, and the
copies) after each of the timed thinks, and "tree_entries", the entries it returned.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minizero_amd as mz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--n", type=int, default=1600)
    ap.add_argument("--B", default="1,8,16,32,64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--tag", default="new")
    ap.add_argument("--tree", action="store_true", help="also time one read-out of the visited tree after every think")
    ap.add_argument("--b1-extra", default="", help="configuration keys added for B = 1 only, e.g. :mz_sim_kernel=false where the simulation kernel has no room for n")
    a = ap.parse_args()
    s = a.board
    d = mz.make_desc(f"go_{s}x{s}", 18, s, s, a.channels, s, s, 1, a.blocks, s * s + 1)
    w = mz.generate_weights(d, 0)
    for B in (int(x) for x in a.B.split(",")):
        conf = (f"env_game=go:env_board_size={s}:actor_num_simulation={a.n}:zero_num_parallel_games=1:mz_manual_step=true:program_seed=1:nn_file_name=bench.pt"
                f":zero_num_threads=1:actor_mcts_think_batch_size={B}" + (a.b1_extra if B == 1 else ""))
        wk = mz.Worker(conf, d, w)
        wk.command("start")
        ms, tree_ms, tree_entries = [], [], 0
        for run in range(a.runs + 1):  # the first think warms up (code objects, buffers)
            wk.reset_search()
            t0 = time.perf_counter()
            while not wk.search_done():
                wk.run_cycles(a.n + 2)
            if run:
                ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            if a.tree:
                t1 = time.perf_counter()
                tree_entries = len(wk.tree(0)["parent"])
                if run:
                    tree_ms.append(round((time.perf_counter() - t1) * 1e3, 3))
        steps, walks, queries = wk.think_stats() if hasattr(wk.L, "mz_worker_think_stats") else (0, 0, 0)
        sim_launches = wk.stats()["sim_launches"]
        wk.close()
        row = dict(tag=a.tag, board=s, n=a.n, B=B, extra=a.b1_extra if B == 1 else "", sim_launches=sim_launches, ms=ms, steps=steps, walks=walks, queries=queries)
        if a.tree:
            row.update(tree_ms=tree_ms, tree_entries=tree_entries)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
