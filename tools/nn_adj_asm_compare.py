#!/usr/bin/env python3
"""Build-machine guard of the units of the adjoint with the MLP on (no GPU needed), built on the parser of
tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/nn_adj_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text.  The helpers of step_vjp_kernel moved from kr_adj.hip
into kr_adj_impl.hpp: the kernels of kr_adj.hip are among them.
Part 2 - the kernels of kr_nnjac.hip and kr_adj_nn.hip: VGPRs, SGPRs, scratch, LDS and the instruction census of every
loop (mlp_input_jacobian_kernel: the k-step loop of a 64-unit chunk; step_vjp_nn_kernel: the two per-point loops).

Exit status 1 if part 1 finds a difference, if one of the two units holds no kernel, or if one of their kernels has scratch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402

UNITS = ("kr_nnjac.s", "kr_adj_nn.s")


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
                print("  FAIL: scratch in a kernel of the adjoint with the MLP on"); bad += 1
            print(f"  loops ({len(k['loops'])}), in program order:")
            for l in k["loops"]: print("      " + tac.fmt_loop(l))
        if not mine:
            print("  (no kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
