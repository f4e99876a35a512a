#!/usr/bin/env python3
"""Build-machine guard of the key-point kernels (no GPU needed), sibling of tools/bnd_asm_compare.py and built on the
parser of tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/kp_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text.  The solves of kr_ms_impl.hpp take the kind of
their solve arguments from the argument (MsSolveArgs<T> everywhere but in the key-point kernels): that must leave every
existing kernel's text alone.
Part 2 - each key-point kernel (kr::RodTableBndKp<T>) next to its boundary twin (kr::RodTableBnd<T>): resources and the
census of EVERY loop of the two.  The store block of a marked point adds branches, so the loops do not pair one to one:
each loop of the key-point kernel is held against the twin's loops of the same fp64 count.

Exit status 1 if part 1 finds a difference, if a key-point kernel with the MLP off has any scratch (with the MLP on
more scratch than the twin's is reported, not failed), or if a loop of a key-point kernel has an fp64 count that no loop of
its twin has, more scalar memory loads than every twin loop of that count or - innermost loops, the sweeps - more scratch
instructions."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    print("part 2: key-point kernels (kr::RodTableBndKp<T>) next to their boundary twins in this build")
    cnt = lambda l, k: dict(l[1]).get(k, 0)
    n_bnd = 0
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        if "kr::RodTableBndKp<" not in d.split("(")[0]: continue
        n_bnd += 1
        twin = bn.get(tac.normalise(d.replace("kr::RodTableBndKp<", "kr::RodTableBnd<")))
        print(f"\n{d}")
        if twin is None:
            print("  (no boundary twin in this build)"); bad += 1; continue
        a, b = branch[twin], branch[name]
        print(f"  twin: {a['unit']}: {dm[twin]}")
        for k in tac.KEYS: print(f"  {k:30s} twin {a['meta'][k]:>6s}    kp {b['meta'][k]:>6s}")
        print(f"  instructions                   twin {len(a['body']):6d}    kp {len(b['body']):6d}")
        if int(b["meta"][".private_segment_fixed_size"]) > int(a["meta"][".private_segment_fixed_size"]):
            print("  note: the key-point kernel needs more scratch than its twin (MLP on: every register that lives across a sweep is a spilled one)")
        # (ms_sim_kernel's fifth template argument is NN; mso_sim_kernel has no MLP form)
        nn = "ms_sim_kernel<" in d and d.split("ms_sim_kernel<")[1].split(",")[4].strip() == "true"
        if not nn and int(b["meta"][".private_segment_fixed_size"]) != 0:
            print("  FAIL: scratch in a key-point kernel with the MLP off"); bad += 1
        # The parser takes every backward branch for a loop, and the store block of a marked point - a branch round 14 or 7
        # stores - adds backward branches inside the trips: the two lists do not align one to one (a two-trip pass shows
        # up once more as the enclosing copy of itself).  So every loop of the key-point kernel is held against the
        # twin's loops of the SAME fp64 count: there must be one, and none of them may have fewer scalar memory loads
        # or (innermost loops) fewer scratch instructions than it has.
        la, lb = a["loops"], b["loops"]
        print(f"  loops of the twin ({len(la)}) and of the key-point kernel ({len(lb)}), in program order:")
        for l in la: print("      twin  " + tac.fmt_loop(l))
        more = 0
        for l in lb:
            same = [t for t in la if cnt(t, "valu_f64") == cnt(l, "valu_f64")]
            worse = (not same and cnt(l, "valu_f64") > 0) or (same and cnt(l, "smem") > max(cnt(t, "smem") for t in same)) or \
                    (not same and cnt(l, "smem") > 0) or (l[2] == 0 and cnt(l, "scratch") > max([cnt(t, "scratch") for t in same] or [0]))
            more += bool(worse)
            print(f"   {'!!' if worse else '  '} kp    " + tac.fmt_loop(l))
        print(f"  {more} loop(s) with an fp64 count no loop of the twin has, more scalar memory loads or (innermost) more scratch instructions")
        if more: print("  FAIL: a loop does more than its twin's"); bad += 1
    if n_bnd == 0:
        print("  (no key-point kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
