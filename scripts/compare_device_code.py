#!/usr/bin/env python3
"""Is the device code of two csrc trees the same?  (No GPU, no import of the package.)

    scripts/compare_device_code.py <csrc A> <csrc B> [--jobs N]

Every *.hip of both trees is compiled to gfx950 device assembly with its own Makefile's CXXFLAGS, INCLUDES and per-unit
`build/<unit>.o: CXXFLAGS += ...` options (read from the Makefile, so the two cannot drift).  `__hip_cuid_<hash>`, a hash
of the source text, becomes a fixed token; each file is then split at its function labels and `.amdhsa_kernel` blocks.
One JSON object per unit: functions (kernels) in A and in B, names in only one, names whose text differs, and whether
the rest of the file (metadata, LDS symbols) is equal.  Exit status 1 if anything differs.  The comparison is of text
only.  A refactor that must not move an instruction exports its parent (`git archive <rev> tap-net_amd/csrc include`)
and compares against it; profiles/ab_switches_device_code.json is such a run.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def make_flags(csrc):
    """(hipcc, common flags, {unit: extra flags}) as csrc/Makefile states them."""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, text, re.M).group(1).split()
    per_unit = {u: f.split() for u, f in re.findall(r"^build/(\w+)\.o:\s*CXXFLAGS\s*\+=\s*(.*)$", text, re.M)}
    return var("HIPCC")[0], var("CXXFLAGS") + var("INCLUDES"), per_unit


def compile_unit(csrc, unit, out):
    hipcc, flags, per_unit = make_flags(csrc)
    cmd = [hipcc, "--offload-arch=gfx950", "--offload-device-only", "-S", "-Wno-unused-command-line-argument"] + flags + per_unit.get(unit, [])
    subprocess.run(cmd + [unit + ".hip", "-o", out], cwd=csrc, check=True)
    return out


def split(path):
    """{function name: its lines, label to .Lfunc_end, the .amdhsa_kernel block included}, and the rest of the file."""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    names = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    parts, rest, cur = {}, [], None
    for line in text.splitlines():
        label = re.match(r"([^\s:]+):", line)
        if label and label.group(1) in names:
            cur = label.group(1)
        (parts.setdefault(cur, []) if cur else rest).append(line)
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
    return parts, rest


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    units = [sorted(f[:-4] for f in os.listdir(d) if f.endswith(".hip")) for d in (args.a, args.b)]
    differs = units[0] != units[1]
    if differs:
        print(json.dumps({"units_only_in_a": sorted(set(units[0]) - set(units[1])),
                          "units_only_in_b": sorted(set(units[1]) - set(units[0]))}))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max(1, min(16, args.jobs))) as pool:
        jobs = {(side, u): pool.submit(compile_unit, os.path.abspath(d), u, os.path.join(tmp, "%s_%s.s" % (side, u)))
                for side, d in (("a", args.a), ("b", args.b)) for u in sorted(set(units[0]) & set(units[1]))}
        for u in sorted(set(units[0]) & set(units[1])):
            (pa, ra), (pb, rb) = split(jobs["a", u].result()), split(jobs["b", u].result())
            row = {"unit": u, "kernels_a": len(pa), "kernels_b": len(pb), "only_in_a": sorted(set(pa) - set(pb)),
                   "only_in_b": sorted(set(pb) - set(pa)), "differ": sorted(k for k in set(pa) & set(pb) if pa[k] != pb[k]),
                   "rest_equal": ra == rb}
            differs |= bool(row["only_in_a"] or row["only_in_b"] or row["differ"]) or not row["rest_equal"]
            print(json.dumps(row), flush=True)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
