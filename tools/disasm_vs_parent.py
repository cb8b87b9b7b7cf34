#!/usr/bin/env python3
"""Device code of this tree against a parent commit, symbol by symbol (needs hipcc; no GPU).

Every .hip of minizero_amd/csrc is compiled in both trees with the Makefile's flags plus `--cuda-device-only -S`; the assembly is split per function symbol
(the instructions between the symbol's label and its end label, and the kernel descriptor block of a kernel).  Comment lines, `.ident` and `.file` are dropped,
the per-module numbering of local labels (.LBB<function>_<block>, .Lfunc_end<function>) is removed, and a symbol's own name inside its text is replaced by a
placeholder, so that a renamed function with the same body compares equal.  Texts are compared as text: nothing is searched for in them.

    tools/disasm_vs_parent.py [--parent REV|DIR] [--renames FILE] [--work DIR] [--jobs N] [--only a.hip b.hip]

--parent   a git revision (default HEAD: the working tree against its last commit) or a directory that holds a checkout of the parent
--renames  lines `old => new` over DEMANGLED names (substring replacement, applied in order; `#` starts a comment): a parent symbol is compared with the
           branch symbol of its renamed name
--work     where the two sets of .s files are kept (default: a temporary directory); an .s that is already there is not compiled again

Prints the counts (identical / different / missing / new) and, for every differing symbol, both sides' VGPRs, SGPRs, private segment, group segment and
instruction count.  Exit status 1 when a parent symbol is different or missing."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("minizero_amd", "csrc")


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M))
    flags = var["CXXFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: "" if m.group(1) == "EXTRA" else var.get(m.group(1), ""), flags)
    return var.get("HIPCC", "/opt/rocm/bin/hipcc"), flags.split()


def compile_tree(tree, out_dir, only, jobs):
    hipcc, flags = makefile_flags(tree)
    hipcc = os.environ.get("HIPCC", hipcc)
    os.makedirs(out_dir, exist_ok=True)
    names = sorted(f for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith(".hip") and (not only or f in only))

    def one(name):
        out = os.path.join(out_dir, name[:-4] + ".s")
        if not os.path.exists(out):
            r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", name, "-o", out + ".tmp"], cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"{tree}: {name}\n{r.stderr[-3000:]}")
            os.replace(out + ".tmp", out)
        return name, out
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, names))


LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")


def split_symbols(path):
    """{symbol: {'text': [...], 'stats': {...}}} of one assembly file"""
    syms, cur, kernel = {}, None, None
    sets = {}
    meta = []
    in_meta = False
    for raw in open(path):
        line = raw.rstrip()
        s = line.strip()
        if s.startswith(".amdgpu_metadata"):
            in_meta = True
            continue
        if s.startswith(".end_amdgpu_metadata"):
            in_meta = False
            continue
        if in_meta:
            meta.append(line)
            continue
        if not s or s.startswith(";") or s.startswith("//") or s.startswith(".ident") or s.startswith(".file"):
            continue
        line = re.sub(r"\s*;.*$", "", line)  # trailing comments
        m = re.match(r"^\t\.type\t(\S+),@function", line)
        if m:
            cur = m.group(1)
            syms[cur] = {"text": [], "stats": {}}
            continue
        if cur and re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        m = re.match(r"^\t\.amdhsa_kernel (\S+)", line)
        if m:
            kernel = m.group(1)
        if kernel:
            syms.setdefault(kernel, {"text": [], "stats": {}})["text"].append(line)
            if s.startswith(".end_amdhsa_kernel"):
                kernel = None
            continue
        m = re.match(r"^\t\.set (\S+)\.(num_vgpr|numbered_sgpr|private_seg_size), (.*)$", line)
        if m:
            sets.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
            continue
        if cur:
            syms[cur]["text"].append(line)
    # kernels: the metadata (an entry of amdhsa.kernels starts with "  - ", its own keys are indented by four; the arguments' keys lie deeper)
    entry = {}
    for raw in meta + ["  - .end: 0"]:
        m = re.match(r"^(  - |    )\.(\w+):\s*(\S+)", raw)
        if not m:
            continue
        if m.group(1) == "  - ":
            if entry.get("name") in syms:
                syms[entry["name"]]["stats"] = {"vgpr": entry.get("vgpr_count"), "sgpr": entry.get("sgpr_count"), "private": entry.get("private_segment_fixed_size"),
                                                "group": entry.get("group_segment_fixed_size")}
            entry = {}
        entry[m.group(2)] = m.group(3)
    # other functions: the .set directives (expressions over their callees where they call)
    for sym, d in syms.items():
        if not d["stats"]:
            st = sets.get(sym, {})
            d["stats"] = {"vgpr": st.get("num_vgpr"), "sgpr": st.get("numbered_sgpr"), "private": st.get("private_seg_size"), "group": None}
        d["stats"]["instructions"] = sum(1 for l in d["text"] if l.startswith("\t") and not l.lstrip().startswith("."))
        d["text"] = [LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), l).replace(sym, "<self>") for l in d["text"]]
    return syms


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "/opt/rocm/lib/llvm/bin/llvm-cxxfilt" if os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt") else "c++filt"
    names = list(names)
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"^void ", "", d) for n, d in zip(names, out)}


def load_renames(path):
    pairs = []
    if path:
        for line in open(path):
            line = line.split("#")[0].strip()
            if line:
                old, new = line.split("=>")
                pairs.append((old.strip(), new.strip()))
    return pairs


def fmt(st):
    return f"vgpr {st['vgpr']}, sgpr {st['sgpr']}, private {st['private']} B, group {st['group']} B, {st['instructions']} instructions"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--renames")
    ap.add_argument("--work")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=[])
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="disasm_vs_parent_")
    if os.path.isdir(a.parent):
        parent_tree = a.parent
    else:
        parent_tree = os.path.join(work, "parent_tree")
        if not os.path.isdir(parent_tree):
            os.makedirs(parent_tree)
            ar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], capture_output=True, check=True).stdout
            subprocess.run(["tar", "-x", "-C", parent_tree], input=ar, check=True)
    parent_s = compile_tree(parent_tree, os.path.join(work, "parent_s"), a.only, a.jobs)
    branch_s = compile_tree(ROOT, os.path.join(work, "branch_s"), a.only, a.jobs)
    renames = load_renames(a.renames)
    counts = {"identical": 0, "identical (renamed)": 0, "different": 0, "missing": 0, "new": 0}
    report = []
    for name in sorted(set(parent_s) | set(branch_s)):
        if name not in branch_s or name not in parent_s:
            report.append(f"{name}: only in the {'parent' if name in parent_s else 'branch'}")
            continue
        P, B = split_symbols(parent_s[name]), split_symbols(branch_s[name])
        dm = demangle(set(P) | set(B))
        by_name = {dm[s]: s for s in B}
        matched = set()
        for sym in sorted(P, key=lambda s: dm[s]):
            want = dm[sym]
            for old, new in renames:
                want = want.replace(old, new)
            other = by_name.get(want)
            tag = "" if want == dm[sym] else f"  [-> {want}]"
            if other is None:
                counts["missing"] += 1
                report.append(f"{name}: MISSING    {dm[sym]}{tag}")
                continue
            matched.add(other)
            if P[sym]["text"] == B[other]["text"]:
                counts["identical (renamed)" if tag else "identical"] += 1
                if tag:
                    report.append(f"{name}: identical  {dm[sym]}{tag}")
            else:
                counts["different"] += 1
                report.append(f"{name}: DIFFERENT  {dm[sym]}{tag}\n      parent: {fmt(P[sym]['stats'])}\n      branch: {fmt(B[other]['stats'])}")
        for sym in sorted(set(B) - matched, key=lambda s: dm[s]):
            counts["new"] += 1
            report.append(f"{name}: new        {dm[sym]}\n      branch: {fmt(B[sym]['stats'])}")
    print(f"parent {a.parent}: " + ", ".join(f"{v} {k}" for k, v in counts.items()))
    print("\n".join(report))
    return 1 if counts["different"] or counts["missing"] else 0


if __name__ == "__main__":
    sys.exit(main())
