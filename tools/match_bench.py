"""Match play at the benchmark's shape: BASELINE configs[1] (9x9 Go, 6 blocks x 64 channels, n = 400), G = 256 slots in two lanes, N = 512 counted games,
actor_select_action_by_softmax_count=true so that the games differ.

    a   the same weights on both sides, f32 against f32: the control — whatever Elo it shows is the noise of the colours and of N games
    b   the same weights, f32 (side A) against bf16x3 (side B): does the faster tower play at another strength?

    python tools/match_bench.py --part a [--seed 3]      one match in this process: one JSON line
    python tools/match_bench.py [--seeds 1,2,3,4,5] [--games 256] [--match-games 512] [--bench-ms MS] [--out profiles/x.json]
                                                         both parts under every seed, the parts alternated, a fresh process per match; --bench-ms: bench.py's
                                                         ms per step of the same session, quoted beside.  Everything in the output file is written here.

Per match: W / D / L of side A by colour, Elo +- standard error (minizero_amd.match_elo), who resigned how often, wall time, ms per step (a step = one
move of every game = n + 1 cycles; a match runs two lanes without tail help), the share of filler games, and how many different games and opening
prefixes the 512 lines hold.  Per part over the seeds ("summary"): the Elo figures with their mean and standard deviation beside the trinomial error —
the control's spread is the yardstick part b is read against — and the range of the step time.  Synthetic weights play weakly: what part b can show on
them is "no difference larger than the control's own spread", no more.  Nothing here is a gate."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = {"a": ("f32", "f32"), "b": ("f32", "bf16x3")}


def run_part(part, games, match_games, sims, seed):
    import minizero_amd as mz
    d = mz.DESCS["c2"]()
    w = mz.generate_weights(d, 0)
    pa, pb = PARTS[part]
    conf = (f"env_game=go:env_board_size=9:actor_num_simulation={sims}:zero_num_parallel_games={games}:mz_match_games={match_games}:program_seed={seed}"
            f":nn_file_name=bench.pt:actor_select_action_by_softmax_count=true:mz_match_precision_a={pa}:mz_match_precision_b={pb}"
            f":mz_match_name_a={pa}:mz_match_name_b={pb}{'_b' if pa == pb else ''}")
    wk = mz.MatchWorker(conf, d, w, w)
    wk.command("start")
    k = wk.cycles_per_move()
    wk.run_cycles(k)  # (the first step carries the first launches' set-up: not timed)
    t0, s0 = time.perf_counter(), wk.stats()["steps"]
    lines = []
    while not wk.stats()["done"]:
        wk.run_cycles(k)
        lines += wk.pop_lines(wait=False)
    dt = time.perf_counter() - t0
    st, ws = wk.stats(), wk.worker_stats()
    lines += wk.pop_lines()
    wk.close()
    # what the lines themselves say: are the games different games, and which side resigned (an unfinished game: the player to move gave up, so the
    # winner's colour is the sign of the result and the resigner is the other colour's side)
    seqs = [tuple(re.findall(r";[BW]\[(\d+)\]", l)) for l in lines]
    distinct = {"games": len(set(seqs))}
    for depth in (1, 2, 4, 8):
        distinct[f"prefix_{depth}"] = len({q[:depth] for q in seqs})
    resigned_by = {pa: 0, pb + ("_b" if pa == pb else ""): 0}
    for l in lines:
        if "." not in re.search(r"RE\[([^\]]*)\]", l).group(1):
            resigned_by[re.search(r"PW\[(\w+)\]" if float(l.split(" ")[4]) > 0 else r"PB\[(\w+)\]", l).group(1)] += 1
    lines = len(lines)
    elo = mz.match_elo(st)
    steps = st["steps"] - s0
    return dict(part=part, precision_a=pa, precision_b=pb, games=games, match_games=match_games, num_simulation=sims, program_seed=seed, lines=lines,
                a_first=st["a_first"], a_second=st["a_second"], resignations=st["resignations"], resigned_by=resigned_by, distinct=distinct, moves=st["moves"], filler_games=st["filler_games"],
                filler_share=st["filler_games"] / (st["filler_games"] + st["games_started"]), elo=elo["elo"], elo_se=elo["se"], score=elo["score"],
                elo_first=elo["first"]["elo"], elo_first_se=elo["first"]["se"], elo_second=elo["second"]["elo"], elo_second_se=elo["second"]["se"],
                within_two_se_of_zero=abs(elo["elo"]) <= 2 * elo["se"], steps=st["steps"], wall_s=dt, ms_per_step=dt / max(1, steps) * 1e3,
                kernel_ms_per_step=ws["ms_forward"] / max(1, st["steps"]),  # the slower lane's simulation-kernel time per step (hipEvent), first step included
                sim_launches=ws["sim_launches"], lanes=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=list(PARTS))
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--match-games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", default="1,2,3,4,5", help="program seeds of the full run, every part under each")
    ap.add_argument("--bench-ms", type=float, default=None, help="bench.py's ms_per_step of the same session")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part:
        print(json.dumps(run_part(a.part, a.games, a.match_games, a.sims, a.seed)), flush=True)
        return
    out = {"written_by": "tools/match_bench.py (every section)", "bench_py_ms_per_step": a.bench_ms, "parts": {p: [] for p in PARTS}, "summary": {}}
    for seed in (int(x) for x in a.seeds.split(",")):
        for part in PARTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--games", str(a.games), "--match-games", str(a.match_games), "--sims", str(a.sims),
                                "--seed", str(seed)], capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0:
                sys.exit(f"part {part}, seed {seed} failed:\n{r.stderr[-3000:]}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            if a.bench_ms:
                res["ms_per_step_over_bench_py"] = res["ms_per_step"] / a.bench_ms
            out["parts"][part].append(res)
            print(json.dumps(res), flush=True)
    for part, runs in out["parts"].items():
        elo, ms = [r["elo"] for r in runs], [r["ms_per_step"] for r in runs]
        out["summary"][part] = dict(precisions=list(PARTS[part]), seeds=[r["program_seed"] for r in runs], elo=elo, elo_mean=statistics.mean(elo),
                                    elo_sd_over_seeds=statistics.stdev(elo) if len(elo) > 1 else None, trinomial_se=[r["elo_se"] for r in runs],
                                    ms_per_step=ms, ms_per_step_min=min(ms), ms_per_step_max=max(ms),
                                    kernel_ms_per_step=[r["kernel_ms_per_step"] for r in runs],
                                    over_bench_py=[min(ms) / a.bench_ms, max(ms) / a.bench_ms] if a.bench_ms else None,
                                    filler_share=[r["filler_share"] for r in runs], resigned_by=[r["resigned_by"] for r in runs])
    print(json.dumps(out["summary"]), flush=True)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
