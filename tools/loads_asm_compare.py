#!/usr/bin/env python3
"""Build-machine guard of the tip-loads kernels (no GPU needed), sibling of tools/bank_asm_compare.py and built on the
parser of tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/loads_asm_compare.py <asm dir of the parent commit> <asm dir of this tree>

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text (tools/tab_asm_compare.py, part 1, whose verdict
this repeats in one line).
Part 2 - each loads kernel (kr::RodTableLoads<T>) next to its table twin (kr::RodTable<T>): resources, scalar memory
loads inside loops, and EVERY loop of the two side by side (a loop whose census differs is marked; the two must have
the same number of loops for that).

Exit status 1 if part 1 finds a difference, if a loads kernel needs more scratch (.private_segment_fixed_size) than
its twin, if any loop has another number of fp64 vector instructions or more scalar memory loads than the twin's, if an
INNERMOST loop (the sweeps) has more scratch instructions, or if the loop structures differ.  An enclosing loop - the
time loop, the iteration of a solve - whose spill code the register allocator placed differently is marked `~~` and
reported, not failed: where the twin spills already, six more live values per step move a reload or two."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    print("part 2: loads kernels (kr::RodTableLoads<T>) next to their table twins in this build")
    cnt = lambda l, k: dict(l[1]).get(k, 0)
    n_loads = 0
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        if "kr::RodTableLoads<" not in d.split("(")[0]: continue
        n_loads += 1
        twin = bn.get(tac.normalise(d.replace("kr::RodTableLoads<", "kr::RodTable<")))
        print(f"\n{d}")
        if twin is None:
            print("  (no table twin in this build)"); bad += 1; continue
        a, b = branch[twin], branch[name]
        print(f"  twin: {a['unit']}: {dm[twin]}")
        for k in tac.KEYS: print(f"  {k:30s} twin {a['meta'][k]:>6s}   loads {b['meta'][k]:>6s}")
        print(f"  instructions                   twin {len(a['body']):6d}   loads {len(b['body']):6d}")
        if int(b["meta"][".private_segment_fixed_size"]) > int(a["meta"][".private_segment_fixed_size"]):
            print("  FAIL: the loads kernel needs more scratch than its twin"); bad += 1
        if len(a["loops"]) != len(b["loops"]):
            print(f"  FAIL: loop counts differ: twin {len(a['loops'])}, loads {len(b['loops'])}"); bad += 1
            continue
        more = moved = 0
        print(f"  all {len(a['loops'])} loops, in program order (twin / loads):")
        for la, lb in zip(a["loops"], b["loops"]):
            spill = cnt(lb, "scratch") > cnt(la, "scratch")
            worse = cnt(lb, "valu_f64") != cnt(la, "valu_f64") or cnt(lb, "smem") > cnt(la, "smem") or (spill and lb[2] == 0)
            more += worse
            moved += spill and not worse
            print(f"   {'  ==' if la == lb else '  !='} twin  " + tac.fmt_loop(la))
            if la != lb: print(f"     {'!!' if worse else '~~' if spill else '  '} loads " + tac.fmt_loop(lb))
        same = sum(1 for la, lb in zip(a["loops"], b["loops"]) if la == lb)
        print(f"  {same} of {len(a['loops'])} loops have an identical census; {more} loop(s) with another fp64 count, more scalar memory "
              f"loads or (innermost) more scratch instructions than the twin's; {moved} enclosing loop(s) with more scratch instructions")
        if more: print("  FAIL: a loop does more than its twin's"); bad += 1
    if n_loads == 0:
        print("  (no loads kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
