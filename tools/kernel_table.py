#!/usr/bin/env python3
"""Resource and instruction-stream table of every kernel of two builds, side by side (no GPU needed).

For a refactor of the HIP sources that must leave the generated code alone: build both trees with the Makefile's flags plus
--save-temps, e.g.

    make -C vla_adapter_amd/csrc -j16 CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --save-temps"

and point this script at the two csrc directories (it reads the device assembly `<unit>-hip-amdgcn-amd-amdhsa-gfx950.s`):

    tools/kernel_table.py PARENT_CSRC BRANCH_CSRC [--units gemm,gemm256,...] [--all]

Per kernel symbol: VGPR / AGPR / SGPR counts, LDS bytes, private-segment (scratch) bytes, spill counts - from the code-object
metadata - and the instruction count and a digest of the instruction stream (comments and debug directives stripped).  Rows
that are equal in both builds are summarised; rows that differ are printed in full.  Exit status 1 when a resource differs,
0 otherwise (a differing instruction stream alone is reported, with its instruction-count delta, not failed).
"""
import argparse
import glob
import hashlib
import os
import re
import sys

FIELDS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
          ("scratch", ".private_segment_fixed_size"), ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count")]


def parse_unit(path):
    """{kernel symbol: {"vgpr": .., ..., "insts": n, "digest": hex}} of one device assembly file."""
    text = open(path).read()
    out = {}
    # metadata: one YAML list entry per kernel under amdhsa.kernels
    meta = text[text.find("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if not name:
            continue
        row = {}
        for key, field in FIELDS:
            m = re.search(re.escape(field) + r":\s+(\d+)", entry)
            row[key] = int(m.group(1)) if m else 0
        out[name.group(1)] = row
    # instruction streams: from the symbol's label to its .Lfunc_end
    for name, row in out.items():
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        insts = []
        for line in (m.group(1) if m else "").splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":") or line.startswith("//"):
                continue
            insts.append(re.sub(r"\s+", " ", line))
        row["insts"] = sum(1 for i in insts if not i.endswith(":"))
        row["digest"] = hashlib.sha256("\n".join(insts).encode()).hexdigest()[:12]
    return out


def load(directory, units):
    table = {}
    for path in sorted(glob.glob(os.path.join(directory, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        unit = os.path.basename(path).split("-hip-")[0]
        if units and unit not in units:
            continue
        for name, row in parse_unit(path).items():
            table[(unit, name)] = row
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--units", default="", help="comma-separated translation units (default: all found)")
    ap.add_argument("--all", action="store_true", help="print every kernel, not only those that differ")
    a = ap.parse_args()
    units = set(u for u in a.units.split(",") if u)
    A, B = load(a.parent, units), load(a.branch, units)
    if not A or not B:
        sys.exit("no device assembly found (build with --save-temps)")
    both = set(u for u, _ in A) & set(u for u, _ in B)          # a unit built on one side only is not compared
    A = {k: v for k, v in A.items() if k[0] in both}
    B = {k: v for k, v in B.items() if k[0] in both}
    keys = [k for k, _ in FIELDS]
    res_diff, stream_diff, same = [], [], 0
    print("%-14s %-5s %5s %5s %5s %7s %7s %6s %6s %7s  %s" % ("unit", "build", *keys, "insts", "kernel"))
    for key in sorted(set(A) | set(B)):
        ra, rb = A.get(key), B.get(key)
        if ra is None or rb is None:
            res_diff.append(key)
            print("%-14s %-5s only in one build: %s" % (key[0], "parent" if ra else "branch", key[1]))
            continue
        r_eq = all(ra[k] == rb[k] for k in keys)
        s_eq = ra["digest"] == rb["digest"]
        if not r_eq:
            res_diff.append(key)
        elif not s_eq:
            stream_diff.append((key, rb["insts"] - ra["insts"]))
        else:
            same += 1
        if a.all or not (r_eq and s_eq):
            for tag, r in (("par", ra), ("br", rb)):
                print("%-14s %-5s %5d %5d %5d %7d %7d %6d %6d %7d  %s" % (key[0], tag, *[r[k] for k in keys], r["insts"], key[1]))
    print("\n%d kernels; %d identical (resources and instruction stream)" % (len(set(A) | set(B)), same))
    print("%d with equal resources and a different instruction stream:" % len(stream_diff))
    for (unit, name), d in stream_diff:
        print("  %-12s %+5d insts  %s" % (unit, d, name))
    print("%d with DIFFERENT RESOURCES%s" % (len(res_diff), ":" if res_diff else ""))
    for unit, name in res_diff:
        print("  %-12s %s" % (unit, name))
    sys.exit(1 if res_diff else 0)


if __name__ == "__main__":
    main()
