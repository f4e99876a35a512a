#!/usr/bin/env python3
"""Build-machine guard of the unit of the bank step adjoint (no GPU needed), built on tools/tab_adj_asm_compare.py:
compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/bank_adj_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently (part 1 of tools/tab_asm_compare.py; the new kernels are listed as NEW).
Part 2 - the kernels of kr_adj_bank.s beside their twins: step_vjp_bank_kernel beside step_vjp_nn_kernel (kr_adj_nn.s), the
handle form of the same body, and beside step_vjp_tab_kernel (kr_adj_tab.s), whose row reads it shares; nn_rows_bank_kernel
beside nn_rows_kernel.  VGPRs, SGPRs, scratch, LDS, spill counts, and the instruction census of every loop line by line
(valu_f64 = the fp64 vector instructions, smem = scalar loads).

Exit status 1 if part 1 finds a difference in a parent kernel, if a bank kernel is missing, has more scratch than its twin,
or if the innermost loops of the step kernel have other fp64 counts than its twin's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402
import tab_adj_asm_compare as tadj  # noqa: E402

TWINS = (("step_vjp_bank_kernel", "step_vjp_nn_kernel", "kr_adj_nn.s"), ("step_vjp_bank_kernel", "step_vjp_tab_kernel", "kr_adj_tab.s"),
         ("nn_rows_bank_kernel", "nn_rows_kernel", "kr_adj_nn.s"))


def main():
    dirs = [a for a in sys.argv if "=" not in a]
    bad, branch, dm, bn = tac.part1(dirs, each=False)
    asm = dirs[2]
    sp = {}
    for unit in ("kr_adj_nn.s", "kr_adj_tab.s", "kr_adj_bank.s"): sp.update(tadj.spills(os.path.join(asm, unit)))
    print("part 2: the kernels of kr_adj_bank.s beside their twins in this build")
    by = lambda base, unit, el: next((n for n in branch if branch[n]["unit"] == unit and dm[n].startswith(f"void kr::{base}<{el}>(")), None)
    for bank, twin, unit in TWINS:
        for el in ("double", "float"):
            t, w = by(bank, "kr_adj_bank.s", el), by(twin, unit, el)
            print(f"\n{bank}<{el}> beside {twin}<{el}>")
            if t is None or w is None:
                print("  FAIL: kernel not found"); bad += 1; continue
            print(f"  twin   {tadj.figures(branch[w], sp.get(w, {}))}")
            print(f"  bank   {tadj.figures(branch[t], sp.get(t, {}))}")
            st, sw = int(branch[t]["meta"][".private_segment_fixed_size"]), int(branch[w]["meta"][".private_segment_fixed_size"])
            if st > sw:
                print("  FAIL: more scratch in the bank kernel than in its twin"); bad += 1
            tadj.side_by_side(branch[w], branch[t], "twin", "bank")
            if twin == "step_vjp_nn_kernel":
                # (the compiler nests the pass-2 variants in one more loop in some instantiations: the innermost loops are compared)
                f64 = lambda k: sorted(dict(c).get("valu_f64", 0) for n, c, inner in k["loops"] if not inner and dict(c).get("valu_f64", 0))
                a, b = f64(branch[w]), f64(branch[t])
                print(f"  fp64 instructions of the innermost loops: twin {a}, bank {b}")
                if a != b:
                    print("  FAIL: fp64 counts per loop differ"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
