#!/usr/bin/env python3
"""Build-machine guard of the unit of the parameter adjoint (no GPU needed), built on the parser of
tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/par_adj_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text.  The body of step_vjp_kernel moved from kr_adj.hip
into kr_adj_impl.hpp (step_vjp_body<T, false>) and point_map_dual became a template on the type of its constants: the
kernels of kr_adj.hip, kr_adj_nn.hip and kr_vjp.hip are among them.
Part 2 - the kernels of kr_adj_par.hip: VGPRs, SGPRs, scratch, LDS and the instruction census of every loop
(step_vjp_par_kernel: the two per-point loops - pass 1 as in step_vjp_kernel, pass 2 with the second evaluation of the
point map along the parameter directions).

Exit status 1 if part 1 finds a difference, if the unit holds no kernel, or if one of its kernels has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402

UNITS = ("kr_adj_par.s",)


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    for unit in UNITS:
        print(f"\npart 2: the kernels of {unit} in this build")
        mine = [n for n in sorted(branch, key=lambda n: dm[n]) if branch[n]["unit"] == unit]
        for name in mine:
            k = branch[name]
            print(f"\n{dm[name]}")
            for key in tac.KEYS: print(f"  {key:30s} {k['meta'][key]:>6s}")
            print(f"  instructions                   {len(k['body']):6d}")
            if int(k["meta"][".private_segment_fixed_size"]) != 0:
                print("  FAIL: scratch in a kernel of the parameter adjoint"); bad += 1
            print(f"  loops ({len(k['loops'])}), in program order:")
            for l in k["loops"]: print("      " + tac.fmt_loop(l))
        if not mine:
            print("  (no kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
