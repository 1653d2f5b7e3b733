#!/usr/bin/env python3
"""profiles/active_mask.md: does the unmasked path pay for the active mask, and what does an all-frozen launch cost.

Reads (1) the directory tools/ab_libs.sh wrote for  parent=<library built from the parent commit>  child=<this tree's library>  -- the
headline bench line of each library, alternating, on one box: `value` and `value_body_contacts_auto` of every repeat --, (2) the two
libraries themselves for the step kernels' registers, spills and scratch (tools/kernel_resources.py), (3) tools/time_active_mask.py's table.

    python tools/active_mask_report.py <ab dir> <parent.so> <child.so> [--launch <time_active_mask output>] [--note TEXT] [--out profiles/active_mask.md]"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def series(ab, name, key):
    out = []
    for f in sorted(glob.glob(os.path.join(ab, name + "_*.json"))):
        with open(f) as fh:
            d = json.load(fh)
        if key in d:
            out.append(d[key] / 1e6)
    return out


def resources(so):
    txt = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), so, "k_step"], capture_output=True, text=True, check=True).stdout
    return {l.split()[0]: l.split()[1:] for l in txt.splitlines()[1:] if l.strip()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ab")
    ap.add_argument("parent")
    ap.add_argument("child")
    ap.add_argument("--launch", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default=None, help="a paragraph appended under 'Notes' (e.g. an earlier session's figures)")
    a = ap.parse_args()
    lines = ["# The active mask: what the unmasked path pays, what an all-frozen launch costs", "",
             "## A/B against the parent commit's library", "",
             "`tools/ab_libs.sh`: `bench.py --no-cpu-baseline --no-info-line` (N = 8192, the headline workload) through `QS_LIB_PATH`, the two libraries "
             "alternating on one box; M env-steps/s of every repeat, in order.  `value` is the headline (`body_contacts=True`), "
             "`value_body_contacts_auto` the same process's second timed loop.", "",
             "| figure | library | repeats | median | min - max |", "|---|---|---|---|---|"]
    verdicts = []
    for key in ("value", "value_body_contacts_auto"):
        got = {}
        for name in ("parent", "child"):
            v = series(a.ab, name, key)
            got[name] = v
            if v:
                lines.append(f"| `{key}` | {name} | " + " ".join(f"{x:.2f}" for x in v) + f" | {statistics.median(v):.2f} | {min(v):.2f} - {max(v):.2f} |")
        if got["parent"] and got["child"]:
            m, lo, hi = statistics.median(got["child"]), min(got["parent"]), max(got["parent"])
            inside = lo <= m <= hi
            verdicts.append(f"`{key}`: the child's median {m:.2f} M lies " + ("INSIDE" if inside else ("ABOVE" if m > hi else "BELOW")) +
                            f" the parent's min - max of this session ({lo:.2f} - {hi:.2f} M); child / parent medians {m / statistics.median(got['parent']):.4f}.")
    lines += [""] + verdicts + ["", "## Registers, spills and scratch of the step kernels (`tools/kernel_resources.py`)", "",
                                "| kernel | parent: vgpr / agpr / spill / scratch B / code KB | child: vgpr / agpr / spill / scratch B / code KB |", "|---|---|---|"]
    rp, rc = resources(a.parent), resources(a.child)
    for k in rc:
        lines.append(f"| `{k}` | " + " / ".join(rp.get(k, ["-"])) + " | " + " / ".join(rc[k]) + " |")
    if a.launch and os.path.exists(a.launch):
        with open(a.launch) as fh:
            lines += ["", "## What a launch costs under a mask", ""] + fh.read().rstrip().split("\n")
    if a.note:
        lines += ["", "## Notes", "", a.note]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
