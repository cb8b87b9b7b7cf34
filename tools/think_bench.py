"""Wall time of one think() from the empty board through the per-actor surface (mz_manual_step=true), per actor_mcts_think_batch_size.
One JSON line per batch size: {"tag", "board", "n", "B", "ms": [one per run], "steps", "walks", "queries"}.  The time runs from mz_worker_reset_search to the
cycle that completes the search (the call returns when the device has finished).  B = 1 runs on the per-game simulation kernel where it has room for n (its LDS tables grow with n: n = 1600 does not fit) and
lock-step otherwise (--b1-extra :mz_sim_kernel=false).  Another build of the library is measured by pointing MZ_LIBMZGPU at it (a build
from before the batched think ignores the key: measure it with --B 1).

    python tools/think_bench.py --board 9 --n 1600 --B 1,8,16,32,64 --runs 5 --tag new

--tree adds "tree_ms": the wall time of one read-out of the visited tree (Worker.tree: the read-out kernel twice, for the size and for the entries, and the
copies) after each of the timed thinks, and "tree_entries", the entries it returned.

--game-moves K --reuse on|off plays K moves of ONE game from the empty board by think(with_play) — reset_search, the search, search_action, act — with
mz_think_reuse_tree on or off, for every batch size of --B (>= 2), --runs times (a new worker each, after one warm-up game).  One JSON line per batch size:
"ms_per_move" (one per run: the wall time of the game over its moves, the re-roots inside), "sims_per_move" (queries over moves), "kept_share" (visits of
the kept roots over moves * (n + 1)), "reroots", "kept", "moves".  --policy-gain G multiplies the policy head's last layer by G: the synthetic weights
give a nearly flat prior and keep little; a sharpened prior keeps one line, as a trained network does.

    python tools/think_bench.py --board 9 --n 1600 --B 32 --game-moves 30 --reuse on --runs 5

--symmetries 8 sets mz_think_symmetries=8 (every leaf evaluated under the eight symmetries of the board and averaged; B >= 2) in either mode and adds
"rows", the network rows computed; with 1, the default, the key is left out of the configuration, so that a build from before it can be measured.

    python tools/think_bench.py --board 19 --n 400 --B 8,16,32,64 --symmetries 8 --runs 5
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minizero_amd as mz  # noqa: E402


def sharpen_policy(d, w, gain):
    """the blob with the policy head's last layer (weight and bias) times gain; the AlphaZero layout ends: policy_fc, value_conv (+ 5 per-channel vectors),
    value_fc1, value_fc (minizero_amd/csrc/weights.cpp)"""
    import numpy as np
    w = np.array(w, np.float32)
    assert w.size == mz.param_count(d)
    hw, A, VH, C = d.hidden_channel_height * d.hidden_channel_width, d.action_size, d.num_value_hidden_channels, d.num_hidden_channels
    pc = (A + hw - 1) // hw
    end = w.size - (VH + 1) - (hw * VH + VH) - (C + 5)
    start = end - (A * pc * hw + A)
    # the layout is recomputed here, so it is checked against the library's own count: the trunk before the policy head (stem + 2 convolutions per block,
    # each with 5 per-channel vectors) and the policy head's 1x1 convolution must end exactly where policy_fc is taken to start
    trunk = (C * d.num_input_channels * 9 + 5 * C) + 2 * d.num_blocks * (C * C * 9 + 5 * C)
    assert d.type == 0 and start == trunk + (pc * C + 5 * pc), "the weight layout is not the one sharpen_policy was written for"
    w[start:end] *= np.float32(gain)
    return w


def sym_key(a):
    return f":mz_think_symmetries={a.symmetries}" if a.symmetries != 1 else ""


def play_game(a, d, w, B, reuse):
    s = a.board
    conf = (f"env_game=go:env_board_size={s}:actor_num_simulation={a.n}:zero_num_parallel_games=1:mz_manual_step=true:program_seed=1:nn_file_name=bench.pt"
            f":zero_num_threads=1:actor_use_dirichlet_noise=false:actor_resign_threshold=-2:actor_select_action_by_count=true:actor_select_action_by_softmax_count=false"
            f":actor_mcts_think_batch_size={B}" + (":mz_think_reuse_tree=true" if reuse else "") + sym_key(a))
    wk = mz.Worker(conf, d, w)
    wk.command("start")
    moves = 0
    t0 = time.perf_counter()
    for _ in range(a.game_moves):
        while not wk.search_done():
            wk.run_cycles(a.n + 2)
        act, player, _ = wk.search_action(0)
        if not wk.act(0, act, player):
            break
        moves += 1
        if wk.env_query(0, 0):
            break
        wk.reset_search()
    ms = (time.perf_counter() - t0) * 1e3
    out = dict(ms=ms, moves=moves, think=wk.think_stats(), reuse=wk.think_reuse_stats() if reuse else (0, 0, 0))
    wk.close()
    return out


def game_mode(a, d, w):
    reuse = a.reuse == "on"
    for B in (int(x) for x in a.B.split(",")):
        runs = [play_game(a, d, w, B, reuse) for _ in range(a.runs + 1)][1:]  # the first game warms up (code objects, buffers)
        r = runs[-1]
        row = dict(tag=a.tag, board=a.board, n=a.n, B=B, reuse=a.reuse, policy_gain=a.policy_gain, moves=r["moves"],
                   ms_per_move=[round(x["ms"] / max(1, x["moves"]), 3) for x in runs], sims_per_move=round(r["think"][2] / max(1, r["moves"]), 1),
                   kept_share=round(r["reuse"][2] / (max(1, r["moves"]) * (a.n + 1)), 4), reroots=r["reuse"][0], kept=r["reuse"][1], symmetries=a.symmetries)
        print(json.dumps(row), flush=True)


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
    ap.add_argument("--game-moves", type=int, default=0, help="play this many moves of one game by think(with_play) instead of timing single thinks")
    ap.add_argument("--reuse", choices=("on", "off"), default="off", help="mz_think_reuse_tree of the game mode")
    ap.add_argument("--symmetries", type=int, choices=(1, 8), default=1, help="mz_think_symmetries: 8 evaluates every leaf under the board's eight symmetries (B >= 2)")
    ap.add_argument("--policy-gain", type=float, default=1.0, help="the policy head's last layer times this (game mode)")
    a = ap.parse_args()
    s = a.board
    d = mz.make_desc(f"go_{s}x{s}", 18, s, s, a.channels, s, s, 1, a.blocks, s * s + 1)
    w = mz.generate_weights(d, 0)
    if a.game_moves > 0:
        return game_mode(a, d, sharpen_policy(d, w, a.policy_gain) if a.policy_gain != 1.0 else w)
    for B in (int(x) for x in a.B.split(",")):
        conf = (f"env_game=go:env_board_size={s}:actor_num_simulation={a.n}:zero_num_parallel_games=1:mz_manual_step=true:program_seed=1:nn_file_name=bench.pt"
                f":zero_num_threads=1:actor_mcts_think_batch_size={B}" + (a.b1_extra if B == 1 else "") + sym_key(a))
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
        rows = wk.think_symmetry_stats()[1] if hasattr(wk.L, "mz_worker_think_symmetry_stats") else queries
        wk.close()
        row = dict(tag=a.tag, board=s, n=a.n, B=B, extra=a.b1_extra if B == 1 else "", sim_launches=sim_launches, ms=ms, steps=steps, walks=walks, queries=queries,
                   symmetries=a.symmetries, rows=rows)
        if a.tree:
            row.update(tree_ms=tree_ms, tree_entries=tree_entries)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
