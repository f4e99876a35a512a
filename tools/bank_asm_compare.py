#!/usr/bin/env python3
"""Build-machine guard of the network-bank kernels (no GPU needed), sibling of tools/tab_asm_compare.py and built on
its parser: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/bank_asm_compare.py <asm dir of the parent commit> <asm dir of this tree>

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build (trailing defaulted `kr::RodConst<T>` / `kr::MlpDev<T>` template arguments dropped from the
demangled name): resources, per-loop census and instruction text.
Part 2 - each bank kernel (kr::MlpBank<T>) next to its one-network table twin: resources, scalar memory loads inside
loops, and EVERY loop of the two side by side (the two must have the same number of loops for that; a loop whose
census differs is marked).

Exit status 1 if part 1 finds a difference, if a bank kernel needs more scratch (.private_segment_fixed_size) than its
twin, or if it has a scalar memory load in a loop where the twin has none."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402


def normalise(name):
    name = re.sub(r"(\bms_sim_kernel<[^()]*?), kr::MlpDev<\w+>>\(", r"\1>(", name)
    return tac.normalise(name)


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, normalise)
    print("part 2: bank kernels (kr::MlpBank<T>) next to their one-network table twins in this build")
    smem = lambda k: sum(dict(l[1]).get("smem", 0) for l in k["loops"])
    n_bank = 0
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        if "kr::MlpBank<" not in d.split("(")[0]: continue
        n_bank += 1
        twin_key = normalise(re.sub(r", kr::MlpBank<\w+>>\((.*), kr::MlpBank<(\w+)>\)$", r">(\1, kr::MlpDev<\2>)", d))
        twin = bn.get(twin_key)
        print(f"\n{d}")
        if twin is None:
            print("  (no table twin in this build)"); bad += 1; continue
        a, b = branch[twin], branch[name]
        print(f"  twin: {a['unit']}: {dm[twin]}")
        for k in tac.KEYS: print(f"  {k:30s} twin {a['meta'][k]:>6s}   bank {b['meta'][k]:>6s}")
        print(f"  instructions                   twin {len(a['body']):6d}   bank {len(b['body']):6d}")
        print(f"  scalar memory loads in loops   twin {smem(a):6d}   bank {smem(b):6d}")
        if int(b["meta"][".private_segment_fixed_size"]) > int(a["meta"][".private_segment_fixed_size"]):
            print("  FAIL: the bank kernel needs more scratch than its twin"); bad += 1
        if len(a["loops"]) == len(b["loops"]):
            extra = 0
            print(f"  all {len(a['loops'])} loops, in program order (twin / bank):")
            for la, lb in zip(a["loops"], b["loops"]):
                sa, sb = dict(la[1]).get("smem", 0), dict(lb[1]).get("smem", 0)
                if sb > sa: extra += 1
                mark = "  ==" if la == lb else "  !="
                print(f"   {mark} twin " + tac.fmt_loop(la))
                if la != lb: print("       bank " + tac.fmt_loop(lb))
            same = sum(1 for la, lb in zip(a["loops"], b["loops"]) if la == lb)
            print(f"  {same} of {len(a['loops'])} loops have an identical census; {extra} loop(s) with more scalar memory loads than the twin's")
            if extra: print("  FAIL: a scalar memory load in a loop where the twin has none"); bad += 1
        else:
            print(f"  loop counts differ: twin {len(a['loops'])}, bank {len(b['loops'])}")
            if smem(b) > smem(a): print("  FAIL: more scalar memory loads inside loops than the twin"); bad += 1
            big = lambda k: [l for l in k["loops"] if l[0] >= 40 and l[2] == 0]
            print("  innermost loops of >= 40 instructions, twin:")
            for l in big(a): print("    " + tac.fmt_loop(l))
            print("  ... bank:")
            for l in big(b): print("    " + tac.fmt_loop(l))
    if n_bank == 0:
        print("  (no bank kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
