#!/usr/bin/env python
"""Packed fp32 math per kernel, read off the compiler's assembly: every kernel source of airpose_amd/csrc is compiled device-only
for gfx950 with the flags the Makefile gives it (CXXFLAGS + FLAGS_<source>; the 16-bit sources a second time with -DAP_F16) and,
per kernel, the v_pk_{fma,mul,add}_f32 instructions are counted, how many of them carry an op_sel modifier, and the kernel's LDS
reads.  Packed fp32 math with op_sel on LDS operands is the signature of the wrong-answer hazard csrc/Makefile describes at
FLAGS_smplx; tests/test_packed_math_scan.py holds the committed list to the Makefile's flags.  Needs hipcc, no GPU.

The committed list holds the sources of the Makefile's SRCS and GRAD_SRCS.  A source linked through another *_SRCS variable
(linked_apart(): ROLL_SRCS) or from a directory below csrc (linked_below(): GUARD_UNITS) is scanned and printed with the rest and left
out of the list: the test that adds such a source scans it live instead (tests/test_roll_abi.py, tests/test_gradnorm_abi.py), and
those tests also hold that every .hip file of csrc and below is in one of the sets.

    python tools/packed_math_scan.py                   # the table, every source that is linked
    python tools/packed_math_scan.py --write           # ... and tests/packed_math_scan.json, the list the test reads
    python tools/packed_math_scan.py --drop-flag smplx # the table of ONE source without its FLAGS_ entry (what a flag removes)
"""
import argparse
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "airpose_amd", "csrc")
OUT = os.path.join(REPO, "tests", "packed_math_scan.json")
PACKED = re.compile(r"^\s+v_pk_(fma|mul|add)_f32\b")
LDS_READ = re.compile(r"^\s+ds_(read|load)\w*\b")


def makefile():
    """-> (hipcc, common flags, {source: its FLAGS_ entry}, the sources compiled twice, all kernel sources) from csrc/Makefile"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).split()
    arch = var("ARCH")[0]
    common = [f.replace("$(ARCH)", arch) for f in var("CXXFLAGS") if not f.startswith("-W")]
    flags = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*=\s*(.*)$", text, re.M)}
    h16 = [s[:-4] for s in var("H16SRCS")]
    rest = [s[:-4] for s in var("SRCS") + var("GRAD_SRCS") if s.endswith(".hip")]
    return os.environ.get("HIPCC", var("HIPCC")[0]), common, flags, h16, h16 + rest


def linked_apart():
    """-> the kernel sources (names without .hip) that the Makefile links through a *SRCS variable other than SRCS, GRAD_SRCS and
    H16SRCS (APISRCS is the host layer: no kernel, never scanned): scanned like the others, not part of the committed list"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    listed = set(makefile()[4])
    found = [s[:-4] for m in re.finditer(r"^(\w*SRCS)\s*\??=\s*(.*)$", text, re.M) if m.group(1) != "APISRCS"
             for s in m.group(2).split() if s.endswith(".hip")]
    return sorted(set(found) - listed)


def linked_below():
    """-> the kernel sources (paths below csrc without .hip) the Makefile links from a directory of their own, through a variable
    that is not named *SRCS (GUARD_UNITS: guard/grad_guard): scanned like the others, not part of the committed list either; the
    test that adds such a source scans it live (tests/test_gradnorm_abi.py)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    return sorted(s[:-4] for m in re.finditer(r"^(\w+_UNITS)\s*\??=\s*(.*)$", text, re.M) for s in m.group(2).split() if s.endswith(".hip"))


def demangle(names):
    llvm = os.path.join(os.path.dirname(os.path.realpath(makefile()[0])), "..", "llvm", "bin")
    filt = shutil.which("llvm-cxxfilt", path=llvm + os.pathsep + os.environ.get("PATH", "")) or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt] + list(names), check=True, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    """void k_bf16::conv<float, 3>(float*, ...) -> k_bf16::conv<float, 3>"""
    name = name.replace("(anonymous namespace)::", "")
    depth, cut = 0, len(name)
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            cut = i
            break
    return re.sub(r"^void ", "", name[:cut])


def scan(hipcc, args, src):
    """-> [dict(kernel, packed, op_sel, ds_reads)] of one compilation, kernels (.amdhsa_kernel) only, device functions left out"""
    asm = subprocess.run([hipcc] + args + ["--cuda-device-only", "-S", "-o", "-", src + ".hip"], cwd=CSRC, check=True,
                         capture_output=True, text=True).stdout
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    rows, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                rows[cur] = dict(packed=0, op_sel=0, ds_reads=0)
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            if PACKED.match(line):
                rows[cur]["packed"] += 1
                rows[cur]["op_sel"] += "op_sel" in line
            elif LDS_READ.match(line):
                rows[cur]["ds_reads"] += 1
    names = demangle(sorted(rows))
    return [dict(kernel=short(names[k]), **rows[k]) for k in sorted(rows)]


COLUMNS = ("source", "build", "flags", "kernel", "packed", "op_sel", "ds_reads")


def scan_sources(sources=None, drop_flags=False, jobs=None):
    """-> one dict of COLUMNS per kernel of `sources` (names without .hip; None: every kernel source of the Makefile), compiled with
    CXXFLAGS and, unless drop_flags, the source's FLAGS_ entry"""
    hipcc, common, flags, h16, srcs = makefile()
    todo = []
    for s in (srcs if sources is None else sources):
        own = [] if drop_flags else flags.get(s, [])
        todo.append((s, s, common + own, " ".join(own)))
        if s in h16:
            todo.append((s, s + " -DAP_F16", common + own + ["-DAP_F16"], " ".join(own)))
    with concurrent.futures.ThreadPoolExecutor(jobs or min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda j: scan(hipcc, j[2], j[0]), todo))
    return [dict(source=s + ".hip", build=tag, flags=own, **r) for (s, tag, _, own), rows in zip(todo, res) for r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write %s" % os.path.relpath(OUT, REPO))
    ap.add_argument("--drop-flag", metavar="SOURCE", help="scan only SOURCE, without its FLAGS_ entry")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    listed, apart = makefile()[4], linked_apart() + linked_below()
    table = scan_sources([a.drop_flag] if a.drop_flag else listed + apart, bool(a.drop_flag), a.j)
    print("%-34s %-72s %7s %7s %8s" % ("source", "kernel", "packed", "op_sel", "ds_reads"))
    for r in table:
        if r["packed"]:
            print("%-34s %-72s %7d %7d %8d" % (r["build"], r["kernel"][:72], r["packed"], r["op_sel"], r["ds_reads"]))
    clean = sorted(set(r["source"] for r in table) - set(r["source"] for r in table if r["packed"]))
    print("no packed fp32 math in any kernel of: " + " ".join(clean))
    if a.write and not a.drop_flag:
        with open(OUT, "w") as f:
            json.dump(dict(command="python tools/packed_math_scan.py --write", columns=list(COLUMNS),
                           kernels=[[r[c] for c in COLUMNS] for r in table if r["source"][:-4] in listed]), f, indent=0)
            f.write("\n")
        print("wrote", os.path.relpath(OUT, REPO), "(without the sources linked apart: %s)" % " ".join(apart) if apart else "")
    return 0


if __name__ == "__main__":
    sys.exit(main())
