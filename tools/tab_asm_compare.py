#!/usr/bin/env python3
"""Build-machine guard of the parameter-table kernels (no GPU needed): compares gfx950 assembly kept by the build
(knode-cosserat_amd/lib/asm/*.s).

    python tools/tab_asm_compare.py <asm dir of the parent commit> <asm dir of this tree>

Part 1 - nothing existing was generated differently: for EVERY kernel of the parent build, the kernel of the same
name in this build (a trailing defaulted `kr::RodConst<T>` template argument is dropped from the demangled name) must
have the same .vgpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size, the same per-loop
instruction census and - stronger - the same instruction text once labels and symbol names are normalised.
Part 2 - the table kernels next to their plain twins: resources and the census of every loop, with scalar memory
instructions (s_load_*, s_buffer_load_*) counted in a class of their own.

Exit status 1 if part 1 finds a difference."""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys

KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"


def demangle(names):
    out = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    out = out.replace("> >", ">>").replace("> >", ">>")  # (GNU c++filt separates closing brackets)
    return dict(zip(names, out.split("\n")))


def normalise(name):
    # ms_sim_kernel<..., kr::RodConst<double>>(  ->  ms_sim_kernel<...>(   (the defaulted parameter-source argument)
    return re.sub(r"(\b(?:mso_sim_kernel|ms_sim_kernel)<[^()]*?), kr::RodConst<\w+>>\(", r"\1>(", name)


def cls(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"):
        if "f64" in op: return "valu_f64"
        if op.startswith(("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")): return "trans"
        return "valu_other"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "flat_", "buffer_")): return "vmem"
    if op.startswith("scratch_"): return "scratch"
    if op.startswith(("s_load", "s_buffer_load")): return "smem"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")): return "branch"
    if op.startswith("s_"): return "salu"
    return "other"


VECTOR = ("mfma", "valu_f64", "trans", "valu_other", "lds", "vmem", "scratch")


def parse(path):
    """{mangled kernel name: dict(meta, loops, body)} of one .s file"""
    lines = open(path).read().split("\n")
    kernels = {}
    # metadata: entries of amdhsa.kernels, keys at indent 4
    meta, cur = {}, None
    in_md = False
    for l in lines:
        if l.startswith("amdhsa.kernels:"): in_md = True; continue
        if not in_md: continue
        if l.startswith("amdhsa.") or l.startswith("..."): in_md = False; cur = None; continue
        m = re.match(r"^  - (\.\w+):\s*(.*)$", l)
        if m:
            cur = {}
            meta[id(cur)] = cur
            cur[m.group(1)] = m.group(2).strip()
            continue
        m = re.match(r"^    (\.\w+):\s*(.*)$", l)
        if m and cur is not None: cur[m.group(1)] = m.group(2).strip()
    by_name = {d[".symbol"][:-3] if d.get(".symbol", "").endswith(".kd") else d.get(".name"): d for d in meta.values()}
    for name, d in by_name.items():
        try:
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        except StopIteration:
            continue
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm") or lines[i].startswith(".Lfunc_end"))
        while not lines[end].startswith(".Lfunc_end") and end + 1 < len(lines): end += 1  # (a kernel may have several s_endpgm)
        labels, loops, body = {}, [], []
        for i in range(start, end):
            m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
            if m: labels[m.group(1)] = i
        for i in range(start, end):
            m = re.match(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", lines[i])
            if m and m.group(2) in labels and labels[m.group(2)] < i: loops.append((labels[m.group(2)], i))
        census = []
        for a, b in sorted(loops):
            c = collections.Counter()
            for l in lines[a:b + 1]:
                s = l.split(";")[0].strip()
                if not s or s.startswith(".") or s.endswith(":"): continue
                c[cls(s.split()[0])] += 1
            census.append((sum(c.values()), tuple(sorted(c.items())), len([x for x in loops if x[0] > a and x[1] < b])))
        for l in lines[start + 1:end]:
            s = l.split(";")[0].strip()
            if not s or (s.startswith(".") and not s.startswith(".LBB")): continue
            s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s).replace(name, "<kernel>")
            body.append(s)
        kernels[name] = dict(meta={k: d.get(k) for k in KEYS}, loops=census, body=body)
    return kernels


def load_dir(d):
    out = {}
    for p in sorted(glob.glob(os.path.join(d, "*.s"))):
        for name, k in parse(p).items():
            k["unit"] = os.path.basename(p)
            out[name] = k
    return out


def fmt_loop(lp):
    n, c, inner = lp
    d = dict(c)
    vec = sum(d.get(k, 0) for k in VECTOR)
    return f"instr {n:5d} vector {vec:5d} inner {inner}  " + " ".join(f"{k}={v}" for k, v in c)


def part1(argv, norm=None, each=True, new_ok=True):
    """Part 1 of every *_asm_compare tool, and all of asm_unchanged.py: every kernel of the parent build (argv[1]) against the
    kernel of the same name, normalised by `norm`, in this build (argv[2]).  Prints a line per kernel (`each`) or per
    difference, then the verdict; a kernel the parent does not have counts only where `new_ok` is False.
    Returns (differences, kernels of this build, their demangled names, {normalised name: mangled name})."""
    norm = norm or normalise
    parent, branch = load_dir(argv[1]), load_dir(argv[2])
    dm = demangle(sorted(set(parent) | set(branch)))
    bn = {norm(dm[name]): name for name in branch}
    if each: print(f"part 1: {len(parent)} kernels of the parent build against this build ({len(branch)} kernels)")
    bad = 0
    for name in sorted(parent, key=lambda n: (parent[n]["unit"], dm[n])):
        key = norm(dm[name])
        if key not in bn:
            print(f"MISSING  {parent[name]['unit']}: {dm[name]}"); bad += 1; continue
        a, b = parent[name], branch[bn[key]]
        diffs = [f"{k} {a['meta'][k]} -> {b['meta'][k]}" for k in KEYS if a["meta"][k] != b["meta"][k]]
        if a["loops"] != b["loops"]: diffs.append(f"loop census differs ({len(a['loops'])} / {len(b['loops'])} loops)")
        if a["body"] != b["body"] and not diffs: diffs.append("instruction text differs (same resources and census)")
        renamed = " [name normalised]" if bn[key] != name else ""
        if diffs:
            bad += 1
            print(f"DIFFERS  {a['unit']}: {dm[name]}{renamed}: " + "; ".join(diffs))
        elif each:
            m = a["meta"]
            print(f"same     {a['unit']}: {dm[name]}{renamed}: vgpr {m['.vgpr_count']} sgpr {m['.sgpr_count']} private {m['.private_segment_fixed_size']} "
                  f"lds {m['.group_segment_fixed_size']} loops {len(a['loops'])} instructions {len(a['body'])} (text identical)")
    if not new_ok:
        have = {norm(dm[name]) for name in parent}
        for key in sorted(set(bn) - have):
            print(f"NEW      {branch[bn[key]]['unit']}: {dm[bn[key]]}"); bad += 1
    if each: print(f"part 1: {bad} of {len(parent)} kernels differ")
    else:
        print(f"part 1: {bad} of {len(parent)} kernels of the parent build differ in this build ({len(branch)} kernels): resources, "
              "loop census, instruction text")
    print()
    return bad, branch, dm, bn


def main():
    bad, branch, dm, bn = part1(sys.argv)
    print("part 2: table kernels (kr::RodTable<T>) next to their plain twins in this build")
    for name in sorted(branch, key=lambda n: dm[n]):
        d = dm[name]
        if "kr::RodTable<" not in d.split("(")[0]: continue
        twin_key = re.sub(r", kr::RodTable<\w+>>\(kr::RodTable<(\w+)>", r">(kr::RodConst<\1>", d)
        twin = bn.get(twin_key)
        print(f"\n{d}")
        if twin is None:
            print("  (no plain twin in this build)"); continue
        a, b = branch[twin], branch[name]
        for k in KEYS: print(f"  {k:30s} plain {a['meta'][k]:>6s}   table {b['meta'][k]:>6s}")
        print(f"  instructions                   plain {len(a['body']):6d}   table {len(b['body']):6d}")
        print(f"  scalar memory loads in loops   plain {sum(dict(l[1]).get('smem', 0) for l in a['loops']):6d}   table {sum(dict(l[1]).get('smem', 0) for l in b['loops']):6d}")
        big = lambda k: [l for l in k["loops"] if l[0] >= 40 and l[2] == 0]
        print("  innermost loops of >= 40 instructions, plain:")
        for l in big(a): print("    " + fmt_loop(l))
        print("  ... table:")
        for l in big(b): print("    " + fmt_loop(l))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
