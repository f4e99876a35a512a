#!/usr/bin/env python3
"""Build-machine guard of the unit of the table step adjoint (no GPU needed), built on the parser of
tools/tab_asm_compare.py: compares gfx950 assembly kept by the build (knode-cosserat_amd/lib/asm/*.s).

    python tools/tab_adj_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> [label=file.s ...] > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same name
in this build: resources, per-loop census and instruction text.
Part 2 - the step kernels of kr_adj_tab.s beside their handle twins (step_vjp_kernel of kr_adj.s, step_vjp_par_kernel of
kr_adj_par.s): VGPRs, SGPRs, scratch, LDS, SGPR / VGPR spill counts, and the instruction census of every loop, twin and table
form line by line (valu_f64 = the fp64 vector instructions, smem = scalar loads).
Part 3 - optional: the same figures of other builds of the unit (label=file.s), e.g. the row copied into SGPRs or staged in
LDS, for the decision where the row lives.

Exit status 1 if part 1 finds a difference, if a table kernel is missing, has scratch, or has more scratch than its twin."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402

TWINS = (("step_vjp_tab_kernel", "step_vjp_kernel"), ("step_vjp_tab_par_kernel", "step_vjp_par_kernel"))
SPILL = (".sgpr_spill_count", ".vgpr_spill_count")


def spills(path):
    """{mangled kernel name: {spill key: value}} from the metadata of one .s file"""
    out, name, cur = {}, None, {}
    for l in open(path):
        m = re.match(r"^    (\.\w+):\s*(\S+)", l)
        if not m: continue
        if m.group(1) == ".name": name = m.group(2)
        if m.group(1) in SPILL: cur[m.group(1)] = m.group(2)
        if name and len(cur) == len(SPILL):
            out[name], name, cur = cur, None, {}
    return out


def figures(k, sp):
    m = k["meta"]
    return (f"vgpr {m['.vgpr_count']} sgpr {m['.sgpr_count']} scratch {m['.private_segment_fixed_size']} lds {m['.group_segment_fixed_size']} "
            f"sgpr spills {sp.get('.sgpr_spill_count', '?')} vgpr spills {sp.get('.vgpr_spill_count', '?')} instructions {len(k['body'])}")


def side_by_side(a, b, la, lb):
    for i in range(max(len(a["loops"]), len(b["loops"]))):
        for lab, k in ((la, a), (lb, b)):
            print(f"    loop {i} {lab:6s} " + (tac.fmt_loop(k["loops"][i]) if i < len(k["loops"]) else "-"))


def main():
    dirs = [a for a in sys.argv if "=" not in a]
    extra = [a.split("=", 1) for a in sys.argv[1:] if "=" in a]
    bad, branch, dm, bn = tac.part1(dirs, each=False)
    asm = dirs[2]
    sp = {}
    for unit in ("kr_adj.s", "kr_adj_par.s", "kr_adj_tab.s"): sp.update(spills(os.path.join(asm, unit)))
    print("part 2: the step kernels of kr_adj_tab.s beside their handle twins in this build")
    by = lambda base, unit, el: next((n for n in branch if branch[n]["unit"] == unit and dm[n].startswith(f"void kr::{base}<{el}>(")), None)
    for tab, twin in TWINS:
        for el in ("double", "float"):
            t, w = by(tab, "kr_adj_tab.s", el), by(twin, "kr_adj_par.s" if "par" in twin else "kr_adj.s", el)
            print(f"\n{tab}<{el}> beside {twin}<{el}>")
            if t is None or w is None:
                print("  FAIL: kernel not found"); bad += 1; continue
            print(f"  twin   {figures(branch[w], sp.get(w, {}))}")
            print(f"  table  {figures(branch[t], sp.get(t, {}))}")
            st, sw = int(branch[t]["meta"][".private_segment_fixed_size"]), int(branch[w]["meta"][".private_segment_fixed_size"])
            if st > sw or st != 0:
                print("  FAIL: scratch in the table kernel"); bad += 1
            side_by_side(branch[w], branch[t], "twin", "table")
    for label, path in extra:
        print(f"\npart 3: {label} ({os.path.basename(path)})")
        ks, sv = tac.parse(path), spills(path)
        names = tac.demangle(sorted(ks))
        for n in sorted(ks, key=lambda n: names[n]):
            if "step_vjp_tab" not in names[n]: continue
            print(f"\n  {names[n].split('(')[0]}\n  {figures(ks[n], sv.get(n, {}))}")
            for i, l in enumerate(ks[n]["loops"]): print(f"    loop {i}        " + tac.fmt_loop(l))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
