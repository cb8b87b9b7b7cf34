"""Cost of the external evaluator's hand-over, in ms per lock-step cycle, on BASELINE configs[1]'s shape (9x9 Go, 6 blocks x 64 channels, 256 games,
n = 400): four timed moves from the empty board after one warm-up move.

    a       Worker with a network of its own on the lock-step resident plan (mz_sim_kernel=false); with --parent-lib the PARENT commit's build of the library
    b       ExternalWorker whose forward() is the library's own Net (mz_net_forward_az on the hand-over buffers): b - a = two kernels and two host waits per cycle
    c_f32   ExternalWorker on a plain torch module of the same shape under TorchEvaluator, float32
    c_bf16  the same module and tensors in bfloat16

    python tools/ext_eval_bench.py --case b                      one case in this process: one JSON line, ms per cycle of every timed move
    python tools/ext_eval_bench.py --rounds 3 [--parent-lib ab/old.so] [--cases a,b,c_f32,c_bf16] [--out profiles/x.json]
                                                                 the cases alternated, a fresh process each; per case the median and the spread over all timed moves

MZ_LIBMZGPU names the library of a process, so the parent's build is measured by its own child processes.  Nothing here is a gate."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMES, N, MOVES = 256, 400, 4
CONF = (f"env_game=go:env_board_size=9:actor_num_simulation={N}:zero_num_parallel_games={GAMES}:program_seed=1:nn_file_name=bench.pt:zero_num_threads=1"
        ":mz_sim_kernel=false")


def torch_module(torch, dtype):
    """the reference's AlphaZero network shape (6 x 64 on 9x9, 2 policy planes, 256 value-hidden units), random weights; returns (logits, value)"""
    nn = torch.nn

    class Block(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.c1, self.b1, self.c2, self.b2 = nn.Conv2d(c, c, 3, padding=1), nn.BatchNorm2d(c), nn.Conv2d(c, c, 3, padding=1), nn.BatchNorm2d(c)

        def forward(self, x):
            return torch.relu(x + self.b2(self.c2(torch.relu(self.b1(self.c1(x))))))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.bn = nn.Conv2d(18, 64, 3, padding=1), nn.BatchNorm2d(64)
            self.blocks = nn.Sequential(*[Block(64) for _ in range(6)])
            self.pc, self.pbn, self.pfc = nn.Conv2d(64, 2, 1), nn.BatchNorm2d(2), nn.Linear(2 * 81, 82)
            self.vc, self.vbn, self.v1, self.v2 = nn.Conv2d(64, 1, 1), nn.BatchNorm2d(1), nn.Linear(81, 256), nn.Linear(256, 1)

        def forward(self, x):
            x = self.blocks(torch.relu(self.bn(self.stem(x))))
            p = self.pfc(torch.relu(self.pbn(self.pc(x))).flatten(1))
            v = torch.tanh(self.v2(torch.relu(self.v1(torch.relu(self.vbn(self.vc(x))).flatten(1)))))
            return p, v

    torch.manual_seed(0)
    return Net().to("cuda:0", dtype).eval()


def run_case(case):
    import minizero_amd as mz
    d = mz.DESCS["c2"]()
    keep = None
    if case == "a":
        wk = mz.Worker(CONF, d, mz.generate_weights(d, 0))
    elif case == "b":
        net = keep = mz.Net(d, mz.generate_weights(d, 0))
        L, ptr = mz.load(), []
        wk = mz.ExternalWorker(CONF, d, lambda rows: L.mz_net_forward_az(net.h, ptr[0], rows, ptr[1], ptr[2], ptr[3], mz.MZ_DEVICE))
        ptr.extend(wk.buffers())
    else:
        import torch
        dtype = {"c_f32": "f32", "c_bf16": "bf16"}[case]
        ev = keep = mz.TorchEvaluator(torch_module(torch, torch.float32 if dtype == "f32" else torch.bfloat16), GAMES, 18, 9, 9, 82, dtype, device="cuda:0")
        wk = ev.worker(CONF, d)
    wk.command("start")
    assert wk.run_cycles(N + 1) == N + 1  # warm-up: code objects, buffers, the convolution library's choice of kernels
    wk.command("reset_actors")
    ms = []
    for _ in range(MOVES):
        t0 = time.perf_counter()
        assert wk.run_cycles(N + 1) == N + 1
        ms.append(round((time.perf_counter() - t0) * 1e3 / (N + 1), 4))
    st = wk.stats()
    wk.close()
    del keep
    return dict(case=case, lib=os.environ.get("MZ_LIBMZGPU", ""), ms_per_cycle=ms, sim_launches=st["sim_launches"], lanes_cycles=st["cycles"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c_f32", "c_bf16"])
    ap.add_argument("--cases", default="a,b,c_f32,c_bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="the parent commit's libmzgpu.so for case a (default: this build)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case)), flush=True)
        return
    rows = {}
    for r in range(a.rounds):
        for case in a.cases.split(","):
            env = dict(os.environ)
            if case == "a" and a.parent_lib:
                env["MZ_LIBMZGPU"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], env=env, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:  # nothing more is started on the device after a process that failed there
                sys.stderr.write(p.stderr[-2000:])
                sys.exit(f"case {case} failed with status {p.returncode}")
            row = json.loads(p.stdout.strip().splitlines()[-1])
            rows.setdefault(case, []).append(row)
            print(f"round {r} {case}: {row['ms_per_cycle']}", flush=True)
    out = dict(shape="go 9x9, 6b x 64, 256 games, n = 400, 4 timed moves per process", rounds=a.rounds, parent_lib=a.parent_lib, cases={})
    for case, rs in rows.items():
        ms = [x for row in rs for x in row["ms_per_cycle"]]
        out["cases"][case] = dict(median_ms_per_cycle=round(statistics.median(ms), 4), min=min(ms), max=max(ms), all=[row["ms_per_cycle"] for row in rs])
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
