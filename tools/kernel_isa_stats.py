#!/usr/bin/env python3
"""Static figures of one kernel instantiation, from the gfx950 assembly hipcc emits (no GPU needed).

    python tools/kernel_isa_stats.py video-anomaly-detection_amd/csrc/conv_mfma.hip \
        'conv3x3_mfma_pkernel<32, 2, 1, 4, 1, 1, 1, 1, 0, 0, 0>' [--json OUT] [--keep-asm FILE | --asm FILE]

The source is cross-compiled with the library's own flags (`-O3 --offload-arch=gfx950 --cuda-device-only -S`); the kernel is
the one whose demangled name contains the given text (exactly one must match).  Printed, and written as JSON with --json:

  * NumVgprs, NumSgprs, ScratchSize, LDS bytes and occupancy, from the resource comment hipcc writes behind the kernel;
  * readlane / writelane counts of the whole kernel (SGPR spills parked in VGPR lanes);
  * for the OUTERMOST LOOP - the backward branch with the longest span, which in the persistent kernels is the frame (or item)
    loop; its label and line span are printed so that the choice can be checked by eye - the static counts of MFMA, other VALU,
    v_readlane_b32, v_writelane_b32, s_nop, s_waitcnt, s_barrier, DS, buffer / global / scratch instructions and of
    exec-mask writes (s_and_saveexec / s_or_saveexec / s_mov / s_or / s_and / s_andn2 ... to exec).

Counts are STATIC (instructions in the text between the loop's label and its back edge, inner loops counted once): a path
behind a uniform branch is counted whether a given work-group takes it or not.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "video-anomaly-detection_amd" / "csrc"


def compile_asm(src: Path, out: Path) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{REPO / 'include'}", f"-I{CSRC}", "--cuda-device-only", "-S",
           str(src), "-o", str(out)]
    subprocess.run(cmd, check=True)


def demangle(names: list[str]) -> list[str]:
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return r.stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return names


def kernel_bodies(lines: list[str]) -> dict[str, tuple[int, int]]:
    """mangled name -> (first line after its label, line of its .Lfunc_end)"""
    out, cur, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            cur, start = m.group(1), i + 1
        elif cur is not None and re.match(r"^\.Lfunc_end\d+:", ln):
            out[cur] = (start, i)
            cur = None
    return out


def classify(op: str) -> str:
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op == "v_readlane_b32" or op == "v_readfirstlane_b32":
        return op
    if op == "v_writelane_b32":
        return op
    if op.startswith("v_"):
        return "valu"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith("buffer_") or op.startswith("global_") or op.startswith("flat_"):
        return "vmem"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def instructions(lines: list[str], lo: int, hi: int):
    for i in range(lo, hi):
        ln = lines[i].split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        yield i, ln.split()[0], ln


def count(lines: list[str], lo: int, hi: int) -> dict[str, int]:
    c = {k: 0 for k in ("mfma", "valu", "v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32", "s_nop", "s_waitcnt", "s_barrier",
                        "ds", "ds_write_b128", "vmem", "scratch", "salu", "exec_writes", "other", "total")}
    for _, op, ln in instructions(lines, lo, hi):
        c[classify(op)] += 1
        c["total"] += 1
        if op == "ds_write_b128":
            c["ds_write_b128"] += 1
        if "saveexec" in op or re.match(r"^s_\w+\s+exec(_lo|_hi)?\b", ln):
            c["exec_writes"] += 1
    return c


def outermost_loop(lines: list[str], lo: int, hi: int):
    labels = {}
    for i in range(lo, hi):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            labels[m.group(1)] = i
    best = None
    for i, op, ln in instructions(lines, lo, hi):
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = ln.split()[-1]
            if tgt in labels and labels[tgt] < i and (best is None or i - labels[tgt] > best[2] - best[1]):
                best = (tgt, labels[tgt], i)
    return best


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", type=Path)
    ap.add_argument("kernel", help="text the demangled kernel name must contain")
    ap.add_argument("--asm", type=Path, help="read this assembly instead of compiling")
    ap.add_argument("--keep-asm", type=Path, help="keep the assembly here")
    ap.add_argument("--json", type=Path, help="write the figures here as well")
    ap.add_argument("--label", default="", help="free text stored in the JSON (e.g. the commit)")
    a = ap.parse_args()

    if a.asm:
        text = a.asm.read_text()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = a.keep_asm or Path(td) / "k.s"
            compile_asm(a.source, out)
            text = out.read_text()
    lines = text.splitlines()
    bodies = kernel_bodies(lines)
    names = list(bodies)
    dem = demangle(names)
    want = a.kernel.replace(" ", "")
    hits = [(n, d) for n, d in zip(names, dem) if want in d.replace(" ", "")]
    if len(hits) != 1:
        print(f"{len(hits)} kernels match {a.kernel!r}:", file=sys.stderr)
        for _, d in (hits or list(zip(names, dem))):
            print("  " + d, file=sys.stderr)
        return 2
    name, shown = hits[0]
    lo, hi = bodies[name]

    res = {}
    for i in range(hi, min(hi + 80, len(lines))):
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", lines[i])
        if m:
            res[m.group(1)] = int(m.group(2))
    loop = outermost_loop(lines, lo, hi)
    whole = count(lines, lo, hi)
    result = {"source": str(a.source), "kernel": shown, "label": a.label, "resources": res,
              "kernel_total": {k: whole[k] for k in ("mfma", "valu", "v_readlane_b32", "v_writelane_b32", "scratch", "exec_writes", "total")}}
    if loop:
        tgt, l0, l1 = loop
        result["outermost_loop"] = {"label": tgt, "first_line": l0 + 1, "back_edge_line": l1 + 1, **count(lines, l0, l1 + 1)}
    print(json.dumps(result, indent=2))
    if a.json:
        a.json.write_text(json.dumps(result, indent=2) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
