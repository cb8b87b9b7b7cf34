"""The HOST half of match play under ThreadSanitizer and AddressSanitizer + UBSan, on this machine, without a GPU: tests/csrc/match_check.cpp (a stand-alone
program with its own main) + the product's host sources as they are + tests/csrc/fake_device.cpp, built here with the variables tests/csrc/Makefile defines
for host_check (the Makefile is read, not edited).  The program plays a TicTacToe match in the lock-step mode on the host rules — two lanes, both networks in
each, T RNG streams on T host threads, so the step's host section runs the games side by side — and checks the tally and, for A = B, a plain worker's games
itself; here its lines, records and tally are held to tests/match_model.py on top.  A sanitizer report fails the test (exit code 66)."""
import os
import re
import subprocess

import pytest

import match_model as MM
import test_match_model as X
import test_search_model as T
from test_sanitizers import run

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BIN = os.path.join(HERE, "_bin")
MOVE = re.compile(r";([BW])\[(\d+)\]P\[([^\]]*)\]V\[([^\]]*)\]R\[([^\]]*)\]")


def makefile_vars():
    """the variables of tests/csrc/Makefile, := and ?= assignments with $(NAME) expanded"""
    out = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^([A-Z]+)\s*[:?]?=\s*(.*)$", line.rstrip("\n"))
        if m:
            out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda v: out.get(v.group(1), ""), m.group(2)).replace("$$", "$")
    return out


@pytest.fixture(scope="session")
def match_binaries():
    v = makefile_vars()
    assert "-fsanitize=thread" in v["TSAN"] and "-fsanitize=address,undefined" in v["ASAN"] and "worker.cpp" in v["HOSTSRC"]
    r = subprocess.run(["make", "-s", "-C", os.path.join(HERE, "..", "oracle"), "liboracle.so"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    os.makedirs(BIN, exist_ok=True)
    out = {}
    for kind in ("tsan", "asan"):
        exe = os.path.join(BIN, "match_check_" + kind)
        libs = v["LIBS"].replace("'", "")
        cmd = [v["CXX"]] + v["COMMON"].split() + v[kind.upper()].split() + ["match_check.cpp", "fake_device.cpp"] + v["HOSTSRC"].split() + libs.split() + ["-o", exe]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-3000:]
        out[kind] = exe
    return out


def play(binary, name, threads, same=False):
    conf, desc_args, seeds, G, N, _ = X.ROWS[name]
    full = T.full_conf(conf, G).replace("zero_num_threads=1", f"zero_num_threads={threads}") + f":mz_match_games={N}:mz_device_env=false:mz_rng_streams={threads}"
    tn = {"alphazero": 0, "muzero": 1}[desc_args[12]]
    out = run(binary, full, desc_args[0], *desc_args[1:12], tn, seeds[0], seeds[0] if same else seeds[1])
    lines = [l[2:] for l in out.splitlines() if l.startswith("L ")]
    records = [l[2:] for l in out.splitlines() if l.startswith("R ")]
    stats = dict(kv.split("=") for kv in next(l for l in out.splitlines() if l.startswith("S ")).split()[1:])
    plain = [l[2:] for l in out.splitlines() if l.startswith("P ")]
    return lines, records, stats, plain


def moves_of(text):
    return [(c, int(a), p, v, r) for c, a, p, v, r in MOVE.findall(text)]


@pytest.mark.parametrize("kind,threads", [("tsan", 1), ("tsan", 4), ("asan", 2)])
@pytest.mark.parametrize("name", ["ttt", "ttt_mz", "ttt_resign"])
def test_match_host_half_equals_model(oracle, match_binaries, name, kind, threads):
    lines, records, stats, _ = play(match_binaries[kind], name, threads)
    m_lines, m_stats, m_slots, _ = X.row_model(oracle, name)
    assert len(lines) == len(m_lines) == X.ROWS[name][4]
    for line, want in zip(lines, m_lines):
        assert line.startswith(want["head"] + " (;") and f"DLEN[{want['DLEN']}]PB[{want['PB']}]PW[{want['PW']}]" in line and f"RE[{want['RE']}]" in line, (line, want)
        assert moves_of(line) == want["moves"]
    for rec, sl in zip(records, m_slots):
        assert moves_of(rec) == sl.moves and f"PB[{MM.SIDES[sl.first]}]PW[{MM.SIDES[1 - sl.first]}]" in rec
    want = {k: (",".join(str(x) for x in v) if isinstance(v, list) else str(int(v))) for k, v in m_stats.items()}
    assert stats == want


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_equal_sides_play_a_plain_workers_games(match_binaries, kind):
    """A = B: checked move for move inside the program, against a plain worker created in the same process"""
    lines, _, stats, plain = play(match_binaries[kind], "ttt", 2, same=True)
    assert len(plain) == 1 and len(lines) == 10 and stats["games_finished"] == "10" and stats["done"] == "1"
