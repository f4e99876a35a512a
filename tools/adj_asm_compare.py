#!/usr/bin/env python3
"""Build-machine guard of the step-adjoint unit (no GPU needed), built on the parser of tools/tab_asm_compare.py: compares
gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/adj_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text.  point_map_dual moved from kr_vjp.hip into
kr_point_dual.hpp: the kernels of kr_vjp.hip are among them.
Part 2 - the kernels of kr_adj.hip: VGPRs, SGPRs, scratch, LDS and the instruction census of every loop (the two
per-point loops of step_vjp_kernel: pass 1 with seven cotangent vectors, pass 2 with one).

Exit status 1 if part 1 finds a difference, if kr_adj.s holds no kernel, or if one of its kernels has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    print("part 2: the kernels of kr_adj.s in this build")
    mine = [n for n in sorted(branch, key=lambda n: dm[n]) if branch[n]["unit"] == "kr_adj.s"]
    for name in mine:
        k = branch[name]
        print(f"\n{dm[name]}")
        for key in tac.KEYS: print(f"  {key:30s} {k['meta'][key]:>6s}")
        print(f"  instructions                   {len(k['body']):6d}")
        if int(k["meta"][".private_segment_fixed_size"]) != 0:
            print("  FAIL: scratch in a step-adjoint kernel"); bad += 1
        print(f"  loops ({len(k['loops'])}), in program order:")
        for l in k["loops"]: print("      " + tac.fmt_loop(l))
    if not mine:
        print("  (no kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
