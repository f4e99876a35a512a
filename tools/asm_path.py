#!/usr/bin/env python3
"""Build-machine tool (no GPU needed): basic blocks of one kernel in a gfx950 .s file kept by the build
(knode-cosserat_amd/lib/asm/<unit>.s), with an instruction census by class per block and the branch targets, and the
sums over a path given as a list of block labels.

    python tools/asm_path.py <unit.s> <kernel-name substring> [--path L1,L2,...] [--loop L] [--blocks] [--min N]

The substring is looked for in the mangled and in the demangled name (c++filt, when there is one); it must select one
kernel.  A block is named by its label (`.LBB3_17`), a block without one by `bb.<n>` from the compiler's own comment,
the entry block `entry`.  A path entry `L*k` counts the block k times (a loop body).  --blocks prints every block
(default: only those on the path, or all when no path is given); --min N leaves out blocks of fewer instructions.
--loop L sums, statically, over every block of the outermost loop that contains block L (all blocks that reach L and
are reached from it: for a persistent kernel the time-step loop with its cold paths).

Classes: fp64, vec (other vector), lane (v_readlane / v_writelane / v_readfirstlane), agpr (v_accvgpr_*), dpp,
lds_rd, lds_wr, gld (global / flat / buffer / scratch load), gst (their stores and atomics), sld (scalar load), salu,
wait, nop, branch.  `spill_rd` is counted beside them (it is part of `lane`): v_readlane_b32 from a VGPR that the
kernel also fills with v_writelane_b32 - the registers SGPRs are spilled to.

Also printed: .sgpr_spill_count, .vgpr_spill_count (kernel metadata), NumVgprs, NumAgprs, ScratchSize."""
import argparse
import collections
import re
import shutil
import subprocess
import sys

CLASSES = ["fp64", "vec", "lane", "agpr", "dpp", "lds_rd", "lds_wr", "gld", "gst", "sld", "salu", "wait", "nop", "branch"]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BBCOM = re.compile(r"^;\s*%bb\.(\d+):")
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)")
VMEM = ("global_", "flat_", "buffer_", "scratch_")


def classify(ins):
    """class of one instruction line (mnemonic and operands)"""
    op = ins.split()[0]
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): return "lane"
    if op.startswith("v_accvgpr"): return "agpr"
    if op.startswith("v_"):
        if "_dpp" in op or " quad_perm:" in ins or " row_" in ins or " wave_" in ins: return "dpp"
        if "f64" in op: return "fp64"
        return "vec"
    if op.startswith("ds_"):
        return "lds_wr" if op.startswith(("ds_write", "ds_store")) else "lds_rd"
    if op.startswith(VMEM):
        return "gld" if "_load" in op else "gst"
    if op.startswith(("s_load", "s_buffer_load", "s_scratch_load")): return "sld"
    if op.startswith("s_waitcnt") or op.startswith("s_wait_"): return "wait"
    if op.startswith("s_nop"): return "nop"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm", "s_call", "s_swappc")): return "branch"
    if op.startswith("s_"): return "salu"
    return "vec"


def demangle(names):
    if not names or not shutil.which("c++filt"): return {n: n for n in names}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: (d or n) for n, d in zip(names, out)}


def kernels(lines):
    """mangled name -> (first line, line of the closing .Lfunc_end) of every global function in the file"""
    found, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", l)
        if m and not l.startswith(".") and cur is None:
            cur = (m.group(1), i)
        elif cur and l.startswith(".Lfunc_end"):
            found[cur[0]] = (cur[1], i)
            cur = None
    return found


def pick(lines, key):
    ks = kernels(lines)
    dm = demangle(sorted(ks))
    hit = [n for n in sorted(ks) if key in n or key in dm[n]]
    if len(hit) != 1:
        raise SystemExit(f"'{key}' selects {len(hit)} kernels:\n" + "\n".join(f"  {dm[n]}" for n in (hit or sorted(ks))))
    return hit[0], dm[hit[0]], ks[hit[0]]


def split_blocks(lines, a, b):
    """[(name, [instruction, ...])] in program order"""
    blocks = [("entry", [])]
    for l in lines[a + 1:b]:
        s = l.strip()
        m = LABEL.match(s)
        if m:
            if blocks[-1][1] or not blocks[-1][0].startswith("bb."): blocks.append((m.group(1), []))
            else: blocks[-1] = (m.group(1), [])  # a label right behind the compiler's %bb comment: the same block
            continue
        m = BBCOM.match(s)
        if m:
            if m.group(1) != "0" or blocks[-1][1]: blocks.append((f"bb.{m.group(1)}", []))
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"): continue
        blocks[-1][1].append(s.split(";")[0].strip())
    return blocks


def spill_regs(blocks):
    regs = set()
    for _, ins in blocks:
        for i in ins:
            m = re.match(r"^v_writelane_b32\s+(v\d+),", i)
            if m: regs.add(m.group(1))
    return regs


def census(ins, spills):
    c = collections.Counter()
    for i in ins:
        c[classify(i)] += 1
        m = re.match(r"^v_readlane_b32\s+\S+\s+(v\d+),", i)
        if m and m.group(1) in spills: c["spill_rd"] += 1
    return c


def targets(blocks, k):
    ins = blocks[k][1]
    t = [m.group(2) for m in (BRANCH.match(i) for i in ins) if m]
    last = ins[-1].split()[0] if ins else ""
    if not last.startswith(("s_branch", "s_endpgm", "s_setpc")) and k + 1 < len(blocks): t.append(blocks[k + 1][0] + " (falls through)")
    return t


def loop_of(blocks, label):
    """names of the blocks that reach `label` and are reached from it (its outermost loop), `label` included"""
    succ = {n: [t.split(" ")[0] for t in targets(blocks, k)] for k, (n, _) in enumerate(blocks)}
    pred = {n: [] for n in succ}
    for n, ts in succ.items():
        for t in ts: pred.setdefault(t, []).append(n)

    def reach(edges):
        seen, todo = set(), [label]
        while todo:
            for t in edges.get(todo.pop(), []):
                if t not in seen: seen.add(t); todo.append(t)
        return seen
    return (reach(succ) & reach(pred)) | {label}


def meta(lines, name, b):
    out = {}
    in_k, cur = False, {}
    for l in lines:  # the amdhsa.kernels list: one mapping per kernel, `.name:` somewhere inside it
        s = l.strip()
        if s.startswith("- .") or s == "...":
            if cur.get(".name") == name: out.update(cur)
            cur = {}
            s = s[2:] if s.startswith("- ") else s
        m = re.match(r"^(\.\w+):\s*(\S+)\s*$", s)
        if m: cur[m.group(1)] = m.group(2)
    if cur.get(".name") == name: out.update(cur)
    res = {k: out.get(k, "?") for k in (".sgpr_spill_count", ".vgpr_spill_count")}
    for l in lines[b:b + 80]:  # the resource comment block behind the function
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize):\s*(\S+)", l.strip())
        if m and m.group(1) not in res: res[m.group(1)] = m.group(2)
    for k in ("NumVgprs", "NumAgprs", "ScratchSize"): res.setdefault(k, "?")
    return res


def fmt(c):
    n = sum(c[k] for k in CLASSES)
    return f"{n:5d}  " + " ".join(f"{k}={c[k]}" for k in CLASSES if c[k]) + (f"  [spill_rd={c['spill_rd']}]" if c["spill_rd"] else "")


def report(lines, key, path=None, all_blocks=False, minlen=0, out=sys.stdout, loop=None):
    name, dname, (a, b) = pick(lines, key)
    blocks = split_blocks(lines, a, b)
    spills = spill_regs(blocks)
    index = {n: k for k, (n, _) in enumerate(blocks)}
    cs = [census(ins, spills) for _, ins in blocks]
    p = out.write
    p(f"kernel: {dname}\n")
    m = meta(lines, name, b)
    p("resources: " + "  ".join(f"{k} {v}" for k, v in m.items()) + "\n")
    p(f"registers SGPRs are spilled to (v_writelane_b32 destinations): {' '.join(sorted(spills, key=lambda r: int(r[1:]))) or 'none'}\n")
    tot = collections.Counter()
    for c in cs: tot.update(c)
    p(f"blocks: {len(blocks)}   static instructions: {fmt(tot)}\n")
    steps = []
    for e in path or []:
        lab, _, rep = e.partition("*")
        if lab not in index: raise SystemExit(f"no block '{lab}' in this kernel")
        steps.append((lab, int(rep) if rep else 1))
    on_path = {lab for lab, _ in steps}
    p("\nblock          instr  census -> branch targets\n")
    for k, (n, ins) in enumerate(blocks):
        if not (all_blocks or not steps or n in on_path): continue
        if len(ins) < minlen and n not in on_path: continue
        p(f"{n:12s} {fmt(cs[k])} -> {', '.join(targets(blocks, k)) or 'end'}\n")
    sums = collections.Counter()
    if steps:
        p("\npath: " + ",".join(lab + (f"*{r}" if r != 1 else "") for lab, r in steps) + "\n")
        for lab, r in steps:
            for k2, v in cs[index[lab]].items(): sums[k2] += v * r
        p(f"path sum:    {fmt(sums)}\n")
        for k2 in CLASSES + ["spill_rd"]: p(f"  {k2:9s}{sums[k2]:6d}\n")
    lsum = collections.Counter()
    if loop:
        if loop not in index: raise SystemExit(f"no block '{loop}' in this kernel")
        members = loop_of(blocks, loop)
        for n in members: lsum.update(cs[index[n]])
        p(f"\nouter loop of {loop}: {len(members)} blocks, static sum: {fmt(lsum)}\n")
        for k2 in CLASSES + ["spill_rd"]: p(f"  {k2:9s}{lsum[k2]:6d}\n")
    return {"blocks": blocks, "census": cs, "meta": m, "path": sums, "spills": spills, "loop": lsum}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--path", default="")
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--loop", default=None)
    ap.add_argument("--min", type=int, default=0)
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    report(lines, a.kernel, [x for x in a.path.split(",") if x], a.blocks, a.min, loop=a.loop)


if __name__ == "__main__":
    main()
