#!/usr/bin/env python3
"""Build-machine guard of the bank key-point kernels (no GPU needed), sibling of tools/bank_asm_compare.py and
tools/kp_asm_compare.py and built on the parser of tools/tab_asm_compare.py: compares gfx950 assembly kept by the build
(knode-cosserat_amd/lib/asm/*.s).

    python tools/bank_kp_asm_compare.py <asm dir of the parent commit> <asm dir of this tree> > profiles/<name>.txt

Part 1 - nothing existing was generated differently: every kernel of the parent build against the kernel of the same
name in this build: resources, per-loop census and instruction text.
Part 2 - each new kernel (ms_sim_kernel<..., kr::RodTableBndKp<T>, kr::MlpBank<T>>) next to its two parents: the bank
kernel (kr::RodTable<T>, kr::MlpBank<T>) and the MLP-on key-point kernel (kr::RodTableBndKp<T>, the handle's kr::MlpDev<T>).
Resources (VGPRs, SGPRs, scratch, LDS) against both, and every loop against the key-point parent's loop at the same
place: the fp64, transcendental, matrix-core, LDS and memory instruction classes of the sweeps and MLP chains.  The store
block of a marked point adds branches, so against the bank kernel the loops do not pair one to one
(tools/kp_asm_compare.py); its loops are listed.

Exit status 1 if part 1 finds a difference, if a new kernel has more VGPRs or more scratch than BOTH parents, if it does
not have the key-point parent's loops one to one, or if a loop's fp64, transcendental, matrix-core, LDS or vector memory
instruction count differs from that parent's loop.  Scalar, integer vector and scratch instruction differences (the
bank's moved base pointers) are reported per loop with their figures, not tuned away."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tab_asm_compare as tac  # noqa: E402

HELD = ("valu_f64", "trans", "mfma", "lds", "vmem")  # what a sweep and an MLP chain are made of
REPORT = ("salu", "smem", "valu_other", "scratch")


def main():
    bad, branch, dm, bn = tac.part1(sys.argv, each=False)
    print("part 2: bank key-point kernels (kr::RodTableBndKp<T>, kr::MlpBank<T>) next to their bank and key-point parents in this build")
    cnt = lambda l, k: dict(l[1]).get(k, 0)
    priv = lambda k: int(k["meta"][".private_segment_fixed_size"])
    vgpr = lambda k: int(k["meta"][".vgpr_count"])
    found = 0
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        head = d.split("(")[0]
        if "kr::RodTableBndKp<" not in head or "kr::MlpBank<" not in head: continue
        found += 1
        bank = bn.get(tac.normalise(d.replace("kr::RodTableBndKp<", "kr::RodTable<")))
        kp = bn.get(tac.normalise(d.replace("kr::MlpBank<", "kr::MlpDev<")))
        print(f"\n{d}")
        if bank is None or kp is None:
            print(f"  (no {'bank' if bank is None else 'key-point'} parent in this build)"); bad += 1; continue
        a, k, b = branch[bank], branch[kp], branch[name]
        print(f"  bank parent:      {a['unit']}: {dm[bank]}")
        print(f"  key-point parent: {k['unit']}: {dm[kp]}")
        for key in tac.KEYS: print(f"  {key:30s} bank {a['meta'][key]:>6s}    kp {k['meta'][key]:>6s}    bank-kp {b['meta'][key]:>6s}")
        print(f"  instructions                   bank {len(a['body']):6d}    kp {len(k['body']):6d}    bank-kp {len(b['body']):6d}")
        if vgpr(b) > max(vgpr(a), vgpr(k)):
            print("  FAIL: more VGPRs than both parents"); bad += 1
        if priv(b) != priv(k):
            print(f"  note: scratch {priv(b)} bytes against the key-point parent's {priv(k)} and the bank parent's {priv(a)}: the bank's index and "
                  "stride and the key-point mask are live across the sweeps together here, in neither parent")
        if priv(b) > max(priv(a), priv(k)):
            print("  FAIL: more scratch than both parents"); bad += 1
        la, lk, lb = a["loops"], k["loops"], b["loops"]
        print(f"  loops: bank parent {len(la)}, key-point parent {len(lk)}, new kernel {len(lb)}")
        if len(lk) != len(lb):
            print("  FAIL: not the loop structure of the key-point parent"); bad += 1; continue
        # The new kernel has the key-point parent's loops, one to one in program order (the store block of a marked point
        # is in both); against the bank parent they do not pair (tools/kp_asm_compare.py).  Held per loop: the classes an
        # MLP chain and a sweep are made of.  Reported per loop: address arithmetic (the network's base pointers are
        # moved by index * stride: scalar and integer vector instructions) and scratch.
        more = 0
        tot = {c: 0 for c in REPORT}
        for x, y in zip(lk, lb):
            worse = [c for c in HELD if cnt(y, c) != cnt(x, c)]
            delta = {c: cnt(y, c) - cnt(x, c) for c in REPORT if cnt(y, c) != cnt(x, c)}
            for c, v in delta.items(): tot[c] += v if x[2] == 0 else 0
            more += bool(worse)
            print(f"   {'!!' if worse else '  '} kp       " + tac.fmt_loop(x))
            print(f"   {'!!' if worse else '  '} bank-kp  " + tac.fmt_loop(y) + (f"   [{' '.join(f'{c}{v:+d}' for c, v in sorted(delta.items()))}]" if delta else ""))
        print(f"  {more} of {len(lb)} loops differ from the key-point parent's in {' / '.join(HELD)} instruction counts")
        print("  innermost loops, summed difference to the key-point parent: " + " ".join(f"{c}{v:+d}" for c, v in tot.items()))
        if more: print("  FAIL: a loop's sweep or MLP chain is not its parent's"); bad += 1
    if found == 0:
        print("  (no bank key-point kernel found)"); bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
