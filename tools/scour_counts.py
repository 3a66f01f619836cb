#!/usr/bin/env python3
"""What zamboni's leaf-block scours find, counted under host emulation (DESIGN.md §4.1 "The scour's
ballots"): the 512 T1 documents of tests/descend_cascade.py through the plain cascade, in a build of the
emulation with -DFMT_SCOUR_COUNT (every scour takes the serial pass and reports what its ballots
predicted beside what the pass found), and what each leaf-level packParent holds: children, leaves, children
that change, text units moved. Prints the tables. CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import micro_cascade  # noqa: E402

OUT = os.path.join(REPO, "tests", "_build", "libmt_emu_scour.so")
COLS = ("calls", "no change", "  caught by the ballots", "drops only", "  caught by the ballots", "merges", "mispredicted")


def main():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-DFMT_SCOUR_COUNT", "-o", OUT,
                    os.path.join(REPO, "tests", "emu", "mt_emu_tiers.cpp"), os.path.join(REPO, "tools", "scour_counts.cpp")],
                   check=True)
    micro_cascade.LIB_PATH = OUT  # (fresh, so lib() loads it as it is)
    from descend_cascade import DescendCascade
    from fluidframework_amd import workloads

    docs = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    batch = workloads.conflict_farm(docs, n_clients=8, ops_per_doc=2000, seed=1)
    L = micro_cascade.lib()
    L.scour_counts_reset()
    cas = DescendCascade(batch)
    esc = cas.rounds()
    assert int(esc[0]) == 0 and (cas.hdr["status"] == 0).all()
    g = np.zeros((2, 7), dtype=np.uint64)
    L.scour_counts_read(g.ctypes.data_as(ctypes.c_void_p))
    ops = float(sum(cas.ops_in))
    print(f"{docs} T1 documents, {int(ops)} ops replayed (ops per tier {cas.ops_in})")
    print(f"{'per op':28s} {'popped block':>14s} {'packParent sibling':>20s} {'all':>10s}")
    for i, name in enumerate(COLS):
        a, b = int(g[0, i]), int(g[1, i])
        print(f"{name:28s} {a / ops:14.4f} {b / ops:20.4f} {(a + b) / ops:10.4f}   ({a + b})")
    pk = np.zeros(13, dtype=np.uint64)
    L.pack_counts_read(pk.ctypes.data_as(ctypes.c_void_p))
    pk = [int(x) for x in pk]
    n = float(max(pk[0], 1))
    print()
    print(f"packParent at leaf level: {pk[0]} ({pk[0] / ops:.4f} per op)")
    print(f"{'per packParent':44s} {'mean':>10s}")
    for name, v in (("children", pk[1]), ("  holding leaves (scoured)", pk[2]), ("leaves in the span", pk[3]),
                    ("leaves left", pk[12]), ("children that change something", pk[4] + pk[5]),
                    ("  drop only", pk[4]), ("  merging", pk[5]), ("sibling text moves", pk[10])):
        print(f"{name:44s} {v / n:10.4f}   ({v})")
    print(f"{'packParents in which no child changes':44s} {pk[6] / n:10.4f}   ({pk[6]})")
    print(f"{'packParents in which one child changes':44s} {pk[7] / n:10.4f}   ({pk[7]})")
    print(f"{'packParents with a text move':44s} {pk[11] / n:10.4f}   ({pk[11]})")
    print(f"text units moved, the siblings' separate moves: {pk[8]} ({pk[8] / ops:.3f} per op)")
    print(f"text units one move per packParent would take:  {pk[9]} ({pk[9] / ops:.3f} per op)")


if __name__ == "__main__":
    main()
