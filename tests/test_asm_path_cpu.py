"""CPU test of tools/asm_path.py: a synthetic gfx950 listing of one kernel with three basic blocks (entry, a loop body,
an exit) and every instruction class once; the per-block census, the branch targets, the path sums with a repeat count,
the spill-register reads and the resource figures must come out as written here."""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """\t.text
\t.globl\t_Z9toy_sweepPd
\t.type\t_Z9toy_sweepPd,@function
_Z9toy_sweepPd:                         ; @_Z9toy_sweepPd
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_writelane_b32 v40, s6, 0
\tv_accvgpr_write_b32 a0, v1
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dwordx2 v[2:3], v0, s[0:1]
\ts_mov_b32 s8, 0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_fma_f64 v[2:3], v[2:3], v[4:5], v[6:7]
\tv_add_f64 v[2:3], v[2:3], v[2:3]
\tv_mov_b32_dpp v8, v2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
\tds_read_b64 v[4:5], v9
\tds_write_b64 v9, v[2:3]
\tv_readlane_b32 s9, v40, 0
\tv_readlane_b32 s10, v2, 3
\ts_nop 1
\ts_add_i32 s8, s8, 1
\ts_cmp_lt_i32 s8, 4
\ts_cbranch_scc1 .LBB0_1
.LBB0_2:
\tv_accvgpr_read_b32 v1, a0
\tv_cndmask_b32_e32 v1, v1, v2, vcc
\tglobal_store_dwordx2 v0, v[2:3], s[0:1]
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z9toy_sweepPd, .Lfunc_end0-_Z9toy_sweepPd
                                        ; -- End function
; Kernel info:
; NumSgprs: 16
; NumVgprs: 41
; NumAgprs: 1
; ScratchSize: 0
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     1
    .name:           _Z9toy_sweepPd
    .sgpr_count:     16
    .sgpr_spill_count: 1
    .vgpr_count:     42
    .vgpr_spill_count: 0
...
\t.end_amdgpu_metadata
"""


def _tool():
    spec = importlib.util.spec_from_file_location("asm_path", os.path.join(ROOT, "tools", "asm_path.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_three_blocks():
    ap = _tool()
    out = io.StringIO()
    r = ap.report(ASM.split("\n"), "toy_sweep", ["entry", ".LBB0_1*4", ".LBB0_2"], out=out)
    names = [n for n, _ in r["blocks"]]
    assert names == ["entry", ".LBB0_1", ".LBB0_2"]
    c = dict(zip(names, r["census"]))
    assert {k: v for k, v in c["entry"].items() if v} == dict(sld=1, lane=1, agpr=1, wait=1, gld=1, salu=1)
    assert {k: v for k, v in c[".LBB0_1"].items() if v} == dict(fp64=2, dpp=1, lds_rd=1, lds_wr=1, lane=2, spill_rd=1, nop=1,
                                                               salu=2, branch=1)
    assert {k: v for k, v in c[".LBB0_2"].items() if v} == dict(agpr=1, vec=1, gst=1, branch=1)
    assert r["spills"] == {"v40"}
    assert ap.targets(r["blocks"], 0) == [".LBB0_1 (falls through)"]
    assert ap.targets(r["blocks"], 1) == [".LBB0_1", ".LBB0_2 (falls through)"]
    assert ap.targets(r["blocks"], 2) == []
    p = r["path"]
    assert p["fp64"] == 8 and p["spill_rd"] == 4 and p["lane"] == 9 and p["agpr"] == 2 and p["branch"] == 5
    assert sum(p[k] for k in ap.CLASSES) == 6 + 4 * 11 + 4
    assert r["meta"] == {".sgpr_spill_count": "1", ".vgpr_spill_count": "0", "NumVgprs": "41", "NumAgprs": "1", "ScratchSize": "0"}
    assert ap.loop_of(r["blocks"], ".LBB0_1") == {".LBB0_1"}
    r2 = ap.report(ASM.split("\n"), "toy_sweep", loop=".LBB0_1", out=io.StringIO())
    assert r2["loop"]["fp64"] == 2 and r2["loop"]["spill_rd"] == 1
    text = out.getvalue()
    assert "path: entry,.LBB0_1*4,.LBB0_2" in text and ".sgpr_spill_count 1" in text
