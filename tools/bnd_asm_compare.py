#!/usr/bin/env python3
"""Build-machine guard of the boundary kernels (no GPU needed), sibling of tools/loads_asm_compare.py and built on the
parser of tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/bnd_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text (tools/tab_asm_compare.py, part 1, whose verdict
this repeats in one line).  The loads kernels are kernels of the parent build: the trait that names the cold slots a step
rewrites (rod_src_step_slots) must leave their text alone.
Part 2 - each boundary kernel (kr::RodTableBnd<T>) next to its loads twin (kr::RodTableLoads<T>): resources, scalar memory
loads inside loops, and EVERY loop of the two side by side (a loop whose census differs is marked; the two must have
the same number of loops for that).

Exit status 1 if part 1 finds a difference, if a boundary kernel with the MLP off has any scratch or one with the MLP on
more (.private_segment_fixed_size) than its twin, if any loop has another number of fp64 vector instructions or more scalar memory loads than the twin's, if an
INNERMOST loop (the sweeps) has more scratch instructions, or if the loop structures differ.  An enclosing loop - the
time loop, the iteration of a solve - whose spill code the register allocator placed differently is marked `~~` and
reported, not failed: where the twin spills already, another lane mask per step moves a reload or two."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402


def align(la, lb, cnt):
    """Pairs of loops (twin, bnd) in program order and the loops without a partner [(side, loop)]; (None, None) if the lists
    do not align on (fp64, LDS, vector memory) counts."""
    import difflib
    key = lambda l: (cnt(l, "valu_f64"), cnt(l, "lds"), cnt(l, "vmem"))
    pairs, extra = [], []
    for op, i0, i1, j0, j1 in difflib.SequenceMatcher(None, [key(l) for l in la], [key(l) for l in lb], autojunk=False).get_opcodes():
        if op == "equal": pairs += list(zip(la[i0:i1], lb[j0:j1]))
        elif op == "insert": extra += [("bnd", l) for l in lb[j0:j1]]
        elif op == "delete": extra += [("twin", l) for l in la[i0:i1]]
        else: return None, None  # a loop of the twin replaced by one that does something else
    return pairs, extra


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    print("part 2: boundary kernels (kr::RodTableBnd<T>) next to their loads twins in this build")
    cnt = lambda l, k: dict(l[1]).get(k, 0)
    n_bnd = 0
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        if "kr::RodTableBnd<" not in d.split("(")[0]: continue
        n_bnd += 1
        twin = bn.get(tac.normalise(d.replace("kr::RodTableBnd<", "kr::RodTableLoads<")))
        print(f"\n{d}")
        if twin is None:
            print("  (no loads twin in this build)"); bad += 1; continue
        a, b = branch[twin], branch[name]
        print(f"  twin: {a['unit']}: {dm[twin]}")
        for k in tac.KEYS: print(f"  {k:30s} twin {a['meta'][k]:>6s}   bnd {b['meta'][k]:>6s}")
        print(f"  instructions                   twin {len(a['body']):6d}   bnd {len(b['body']):6d}")
        if int(b["meta"][".private_segment_fixed_size"]) > int(a["meta"][".private_segment_fixed_size"]):
            print("  FAIL: the boundary kernel needs more scratch than its twin"); bad += 1
        # (ms_sim_kernel's fifth template argument is NN; mso_sim_kernel has no MLP form)
        nn = "ms_sim_kernel<" in d and d.split("ms_sim_kernel<")[1].split(",")[4].strip() == "true"
        if not nn and int(b["meta"][".private_segment_fixed_size"]) != 0:
            print("  FAIL: scratch in a boundary kernel with the MLP off"); bad += 1
        # The parser takes every backward branch for a loop, and the block placement of an if / else inside the time loop can
        # add or drop one (12 instructions, no memory access).  The two lists are therefore aligned on what a loop does -
        # its fp64, LDS and vector-memory counts - and a loop without a partner must do none of what is compared.
        pairs, extra = align(a["loops"], b["loops"], cnt)
        if pairs is None:
            print(f"  FAIL: loop structures differ: twin {len(a['loops'])}, bnd {len(b['loops'])}"); bad += 1
            continue
        more = moved = 0
        print(f"  all {len(b['loops'])} loops of the boundary kernel, in program order (twin / bnd):")
        for who, l in extra:
            heavy = cnt(l, "valu_f64") or cnt(l, "smem") or cnt(l, "scratch")
            print(f"   {'!!' if heavy else '  '} without a partner, {who}: " + tac.fmt_loop(l))
            if heavy and who == "bnd":
                print("  FAIL: a loop of the boundary kernel alone has fp64, scalar memory or scratch instructions"); bad += 1
        for la, lb in pairs:
            spill = cnt(lb, "scratch") > cnt(la, "scratch")
            worse = cnt(lb, "valu_f64") != cnt(la, "valu_f64") or cnt(lb, "smem") > cnt(la, "smem") or (spill and lb[2] == 0)
            more += worse
            moved += spill and not worse
            print(f"   {'  ==' if la == lb else '  !='} twin  " + tac.fmt_loop(la))
            if la != lb: print(f"     {'!!' if worse else '~~' if spill else '  '} bnd   " + tac.fmt_loop(lb))
        same = sum(1 for la, lb in pairs if la == lb)
        print(f"  {same} of {len(pairs)} paired loops have an identical census; {more} loop(s) with another fp64 count, more scalar memory "
              f"loads or (innermost) more scratch instructions than the twin's; {moved} enclosing loop(s) with more scratch instructions")
        if more: print("  FAIL: a loop does more than its twin's"); bad += 1
    if n_bnd == 0:
        print("  (no boundary kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
