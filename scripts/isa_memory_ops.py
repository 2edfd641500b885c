#!/usr/bin/env python3
"""Memory instructions by address space, and resources, of every kernel - read from the compiler's assembly, no device needed.

Compiles the .hip files of poselib_amd/csrc device-only for gfx950 with the flags of poselib_amd/csrc/Makefile and prints,
per kernel (and per device function the compiler kept as a symbol of its own): flat / global / scalar loads, flat / global
stores, flat / global atomics, VGPRs, SGPRs, scratch bytes, LDS bytes and occupancy.  A group kernel that reads a pointer it
fetched from its argument table without pl_global.h's globalised() shows up here with flat_* instructions.

    python scripts/isa_memory_ops.py                      # all six files, markdown table
    python scripts/isa_memory_ops.py pipeline gen_rel     # some of them
    python scripts/isa_memory_ops.py --json pipeline      # machine readable (tests/test_group_address_spaces.py)
    python scripts/isa_memory_ops.py --keep DIR ...       # keep the .s files in DIR (to compare two commits with cmp)
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poselib_amd", "csrc")
FILES = ["kernels", "gen_rel", "lm_cam", "focal", "sfocal", "pipeline", "ingest", "rank"]


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


def makefile_flags(name):
    """FLAGS of the Makefile with its variables expanded, plus what the rule of `name`.o adds between $(FLAGS) and -c."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    rule = re.search(r"^%s\.o:.*\n\t\$\(HIPCC\) \$\(FLAGS\)(.*?)-c %s\.hip" % (name, name), text, re.M)
    return flags + rule.group(1).split()


def compile_asm(hipcc, name, out_dir):
    out = os.path.join(out_dir, name + ".s")
    cmd = [hipcc] + makefile_flags(name) + ["--cuda-device-only", "-S", name + ".hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True)
    return out


LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
KINDS = (
    ("flat_ld", re.compile(r"^flat_load_")),
    ("flat_st", re.compile(r"^flat_store_")),
    ("flat_at", re.compile(r"^flat_atomic_")),
    ("glob_ld", re.compile(r"^global_load_")),
    ("glob_st", re.compile(r"^global_store_")),
    ("glob_at", re.compile(r"^global_atomic_")),
    ("scal_ld", re.compile(r"^s_(buffer_)?load_")),
)
RESOURCES = (
    ("vgpr", re.compile(r"^; NumVgprs: (\d+)")),
    ("sgpr", re.compile(r"^; TotalNumSgprs: (\d+)")),
    ("scratch", re.compile(r"^; ScratchSize: (\d+)")),
    ("lds", re.compile(r"^; LDSByteSize: (\d+)")),
    ("occupancy", re.compile(r"^; Occupancy: (\d+)")),
)


def parse(path):
    """-> {symbol: {kind: count, resource: value, "kernel": bool}} in file order"""
    syms, cur, last = {}, None, None
    kernels = set()
    for line in open(path):
        m = LABEL.match(line)
        if m and not m.group(1).startswith(".L"):
            cur = last = syms.setdefault(m.group(1), {k: 0 for k, _ in KINDS})
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s.startswith(".amdhsa_kernel "):
            kernels.add(s.split()[1])
        elif cur is not None and s and s[0] not in ".;":
            for k, rx in KINDS:
                if rx.match(s):
                    cur[k] += 1
                    break
        elif last is not None and s.startswith(";"):
            for k, rx in RESOURCES:
                m = rx.match(s)
                if m:
                    last[k] = int(m.group(1))
    out = {}
    for name, d in syms.items():
        if "vgpr" not in d:  # a data label, not a function
            continue
        d["kernel"] = name in kernels
        out[name] = d
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, full in zip(names, res):
        full = re.sub(r"^void ", "", full)
        # arguments off, template arguments kept: pl::k_lm<0>(pl::LMTask*, unsigned int) -> k_lm<0>
        depth, cut = 0, len(full)
        for i, ch in enumerate(full):
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0 and not full.startswith("(anonymous", i) and "lambda" not in full[i : i + 8]:
                cut = i
                break
        # (a lambda the compiler did not inline is a symbol of its own inside the kernel's name)
        short[n] = full[:cut].replace("pl::", "") + ("::lambda" if "lambda" in full[cut:] else "")
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", default=FILES, help="of: " + " ".join(FILES))
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--keep", metavar="DIR", help="write the assembly files here and keep them")
    ap.add_argument("--asm", metavar="DIR", help="do not compile: read NAME.s from here")
    a = ap.parse_args()
    for f in a.files:
        if f not in FILES:
            ap.error("unknown file " + f)
    tmp = None
    if a.asm:
        paths = {f: os.path.join(a.asm, f + ".s") for f in a.files}
    else:
        hipcc = find_hipcc()
        if not hipcc:
            sys.exit("hipcc not found")
        out_dir = a.keep or (tmp := tempfile.mkdtemp(prefix="isa_memory_ops_"))
        os.makedirs(out_dir, exist_ok=True)
        with ThreadPoolExecutor(len(a.files)) as ex:
            paths = dict(zip(a.files, ex.map(lambda f: compile_asm(hipcc, f, out_dir), a.files)))
    try:
        result = {}
        for f in a.files:
            syms = parse(paths[f])
            names = demangle(list(syms))
            result[f] = [dict(name=names[n], symbol=n, **d) for n, d in syms.items()]
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        json.dump(result, sys.stdout, indent=1)
        print()
        return
    cols = ["flat_ld", "flat_st", "flat_at", "glob_ld", "glob_st", "glob_at", "scal_ld", "vgpr", "sgpr", "scratch", "lds", "occupancy"]
    for f in a.files:
        print("### %s.hip\n" % f)
        print("| kernel | " + " | ".join(cols) + " |")
        print("|---|" + "---:|" * len(cols))
        for r in result[f]:
            label = "`%s`" % r["name"] + ("" if r["kernel"] else " (function)")
            print("| %s | " % label + " | ".join(str(r.get(c, "")) for c in cols) + " |")
        print()


if __name__ == "__main__":
    main()
