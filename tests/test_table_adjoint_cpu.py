"""CPU tier of the table adjoint (kr_step_vjp_table_batch, kr_simulate_vjp_table_batch, krod_grad's table forms): the C ABI
surface, the argument checks that need no device or library, and the composition the calls are defined as - restated in NumPy
with per-rod parameters and per-step boundary values (table_adjoint_cases.numpy_rollout_adjoint) - held to the fixture the GPU
tests compare with; two mutants of it show that the fixture tells the rods and the steps apart.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import param_adjoint_cases as pc
import step_adjoint_cases as sc
import table_adjoint_cases as tc
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = ("kr_step_vjp_table_batch", "kr_simulate_vjp_table_batch")


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_table_symbols_declared_exported_and_bound(lib):
    """The header declares both calls, cites the reference lines they differentiate and says what they do not serve; the
    library exports them and krod_native binds them with the header's argument count; a null handle or table is refused
    without a device and no output byte is written."""
    import krod_native as kn
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert proto, f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == proto.group(1).count(",") + 1, name
        assert "const kr_param_table* t" in proto.group(1) and "g_par" in proto.group(1) and "use_nn" not in proto.group(1)
        assert "int64_t B" not in proto.group(1)  # (B is the table's)
    assert "bnd_per_step" in re.search(r"\bint\s+kr_simulate_vjp_table_batch\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    doc = text[text.index("the adjoint of a heterogeneous batch"):]
    assert "knode.py:70-100" in doc and "cosserat_ode.py:188-213" in doc
    for word in ("MLP-on", "RK4", "del_t", "bank", "bnd_per_step == 1", "loads[b][t]", "bnd[b][t]"):
        assert word in doc, word
    # the existing adjoint calls point here
    par_doc = text[text.index("gradient of the rod's material parameters"):text.index("the adjoint of a heterogeneous batch")]
    assert "kr_step_vjp_table_batch" in par_doc and "kr_simulate_vjp_table_batch" in par_doc
    out = (ctypes.c_double * 43)(*([7.0] * 43))
    buf = (ctypes.c_double * 64)()
    assert lib.kr_step_vjp_table_batch(None, None, kn.KR_EULER, buf, buf, buf, buf, buf, out, out, out, out, out, None, None, kn.KR_F64,
                                       None) == kn.KR_E_ARG and b"handle" in lib.kr_last_error()
    assert lib.kr_simulate_vjp_table_batch(None, None, 1, kn.KR_EULER, buf, buf, None, out, None, out, out, 1, out, None, None, kn.KR_F64,
                                           None) == kn.KR_E_ARG and b"handle" in lib.kr_last_error()
    assert list(out) == [7.0] * 43


class _Robot:
    """stands in for a CosseratRod in the checks that come before any library or device work"""
    _use_nn = False

    def _native(self):
        raise AssertionError("the argument checks come before the device is touched")

    def _params(self):
        raise AssertionError("the argument checks come before the library's rows are made")

    def compute_intermediate_terms(self):
        raise AssertionError("the argument checks come before the robot is written")


def test_simulate_tips_batch_checks_its_arguments():
    """robots with the MLP on, wrong shapes, unknown names, len(robots) != B: KrError before anything runs"""
    import torch
    import krod_grad as kg
    import krod_native as kn
    r, B, T = _Robot(), 2, 3
    robots = [_Robot(), _Robot()]
    ctl = torch.zeros((B, T, 4))
    with pytest.raises(kn.KrError, match="robots holds 3 rods, ctl 2"):
        kg.simulate_tips_batch(r, robots + [_Robot()], ctl)
    with pytest.raises(kn.KrError, match="unknown parameter 'del_t'"):
        kg.simulate_tips_batch(r, robots, ctl, theta={"del_t": torch.zeros(B)})
    with pytest.raises(kn.KrError, match=r"theta\['Bbt'\] must have shape \(2, 3, 3\)"):
        kg.simulate_tips_batch(r, robots, ctl, theta={"Bbt": torch.zeros((3, 3))})
    with pytest.raises(kn.KrError, match=r"theta\['E'\] must have shape \(2,\)"):
        kg.simulate_tips_batch(r, robots, ctl, theta={"E": torch.tensor(1e9)})
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_batch(r, robots, ctl, theta={"E": np.zeros(B)})
    with pytest.raises(kn.KrError, match=r"base_motion must be \[B, T, 13\] = \[2, 3, 13\]"):
        kg.simulate_tips_batch(r, robots, ctl, base_motion=torch.zeros((B, T, 19)))
    with pytest.raises(kn.KrError, match=r"tip_loads must be \[B, T, 6\] = \[2, 3, 6\]"):
        kg.simulate_tips_batch(r, robots, ctl, tip_loads=np.zeros((T, 6)))
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_batch(r, robots, np.zeros((B, T, 4)))
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.simulate_tips_batch(r, robots, torch.zeros((B, T, 5)))
    with pytest.raises(kn.KrError, match="unsupported dtype"):
        kg.simulate_tips_batch(r, robots, ctl, dtype="f16")
    nn = _Robot()
    nn._use_nn = True
    with pytest.raises(kn.KrError, match="rod 1: .* MLP on is not served"):
        kg.simulate_tips_batch(r, [_Robot(), nn], ctl)
    with pytest.raises(kn.KrError, match="MLP on is not served"):
        kg.simulate_tips_batch(nn, robots, ctl)
    g_tips, states = np.zeros((B, T, 3)), np.zeros((T + 1, B, 5, kn.KR_SLOTS))
    with pytest.raises(kn.KrError, match="robots holds 1 rods, ctl 2"):
        kg.rollout_grad(r, np.zeros((B, T, 4)), states, g_tips=g_tips, robots=[_Robot()])
    with pytest.raises(kn.KrError, match="rod 0: .* MLP on is not served"):
        kg.rollout_grad(r, np.zeros((B, T, 4)), states, g_tips=g_tips, robots=[nn, _Robot()])
    with pytest.raises(kn.KrError, match="per_step_boundary needs robots"):
        kg.rollout_grad(r, np.zeros((B, T, 4)), states, g_tips=g_tips, per_step_boundary=True)


def test_fixture_covers_the_cases_and_resolves_every_block():
    """table_adjoint.npz holds the three rods at N = 9 in the three cases, is what table_adjoint_cases derives (inputs and
    states re-derived here from the oracle), every block's tolerance is at most 1e-2 of the block, and the file is no larger
    than rk4_sweeps.npz."""
    g = load_golden("table_adjoint")
    gold = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(gold, "table_adjoint.npz")) <= os.path.getsize(os.path.join(gold, "rk4_sweeps.npz"))
    worst = 0.0
    for b in range(3):
        for case, (T, with_prev) in tc.CASES.items():
            k, rc = tc.key(b, case), tc.rod_case(b, case)
            assert g[k + "states"].shape == (T + 1, tc.N_FIX, 28) and g[k + "bnd"].shape == (T, 19) and (k + "prev_init" in g) == with_prev
            for name in ("ctl", "bnd", "state0", "gbar", "states"):
                assert np.max(np.abs(g[k + name] - rc[name])) < 1e-13, (k, name)
            assert np.ptp(g[k + "bnd"][:, 0:3], axis=0).max() > 0 if T > 1 else True  # (the base does move)
            n = 23 * T + len(tc.entries()) * (2 if with_prev else 1)
            assert g[k + "x_fd_h"].shape == g[k + "x_fd_2h"].shape == (2, n) and g[k + "par_fd_h"].shape == (2, pc.KR_PAR)
            for c in range(2):
                for name, idx in tc.x_blocks(T, with_prev):
                    a, bb = g[k + "x_fd_h"][c][idx], g[k + "x_fd_2h"][c][idx]
                    if not np.any(a) and not np.any(bb):
                        assert c == 1 and T == 3 and ("[1]" in name or "[2]" in name), (k, c, name)  # steps behind the one state touched
                        continue
                    tol, size = sc.block_tol(a, bb, tc._floor_of(name, g[k + "x_floor"][c])), float(np.max(np.abs(a)))
                    assert tol <= tc.MAX_REL_TOL * size, (k, c, name, tol, size)
                    worst = max(worst, tol / size)
                for bi, (name, err, tol, size, zero) in enumerate(pc.block_report(g[k + "par_fd_h"][c], g[k + "par_fd_h"][c], g[k + "par_fd_2h"][c],
                                                                                  g[k + "par_floor"][c])):
                    assert float(g[k + "par_rung"][c, bi]) in pc.ladder_of(name) and not zero, (k, name)
                    assert tol <= tc.MAX_REL_TOL * size, (k, c, name, tol, size)
                    worst = max(worst, tol / size)
    print(f"largest tolerance / block size: {worst:.1e}")


_adj = {}


def adjoint(b, case, c, row=None):
    """numpy_rollout_adjoint of rod b with the row of rod `row` (default its own), computed once"""
    row = b if row is None else row
    if (b, case, c, row) not in _adj:
        rc = tc.rod_case(b, case)
        _adj[(b, case, c, row)] = tc.numpy_rollout_adjoint(sc.params(tc.SETS[row], tc.N_FIX), rc, c)
    return _adj[(b, case, c, row)]


def _inner_tol(a, b, rnd):
    """what the NumPy adjoint's own differences of the point map leave (test_param_adjoint_cpu): ten times the disagreement of two
    inner steps plus the rounding of the quotients"""
    return 10.0 * float(np.max(np.abs(a - b))) + float(np.max(rnd))


@pytest.mark.parametrize("b", range(3))
def test_numpy_rollout_adjoint_reproduces_the_fixture(b):
    """Every block of the fixture - g_ctl, the per-step g_bnd, the entries of g_states[0] / g_prev_init under the block rule;
    the ten parameter blocks under it plus the resolution of the restatement's own inner differences - for rod b in every case
    and both cotangents."""
    g = load_golden("table_adjoint")
    for case, (T, with_prev) in tc.CASES.items():
        k = tc.key(b, case)
        for c in range(2):
            res = adjoint(b, case, c)
            tc.assert_x_blocks(res["gx"], g[k + "x_fd_h"][c], g[k + "x_fd_2h"][c], g[k + "x_floor"][c], T, with_prev, f"{k} cot {c}")
            got, got2 = res["g_par"]
            for bi, (name, off, n, _) in enumerate(pc.PAR_BLOCKS):
                a, bb = g[k + "par_fd_h"][c, off:off + n], g[k + "par_fd_2h"][c, off:off + n]
                err = float(np.max(np.abs(got[off:off + n] - a)))
                tol = sc.block_tol(a, bb, float(g[k + "par_floor"][c, bi])) + _inner_tol(got[off:off + n], got2[off:off + n], res["round"][off:off + n])
                print(f"{k} cot {c} {name:12s} err {err:.2e} tol {tol:.2e} size {np.max(np.abs(a)):.2e}")
                assert err <= tol, (k, c, name, err, tol)


@pytest.mark.parametrize("b", range(3))
def test_mutants_miss_by_ten_bounds(b):
    """Two wrong adjoints are each seen by at least one block of rod b at ten times its bound or more: rod b computed with row
    (b + 1) mod 3, and the per-step boundary gradient shifted by one step - and the same summed over the steps.  (A mutant that
    stayed under ten bounds would mean inputs too alike; the inputs would change, not the bound.)"""
    g = load_golden("table_adjoint")
    case, T = "T3", 3
    k = tc.key(b, case)
    args = lambda c: (g[k + "x_fd_h"][c], g[k + "x_fd_2h"][c], g[k + "x_floor"][c], T, False)
    wrong_row = max(tc.x_misses(adjoint(b, case, 0, row=(b + 1) % 3)["gx"], *args(0)), key=lambda m: m[1])
    good = adjoint(b, case, 0)
    shifted = max(tc.x_misses(tc.with_bnd_grad(good["gx"], np.roll(good["g_bnd"], 1, axis=0), T), *args(0)), key=lambda m: m[1])
    summed = max(tc.x_misses(tc.with_bnd_grad(good["gx"], np.tile(good["g_bnd"].sum(axis=0), (T, 1)), T), *args(0)), key=lambda m: m[1])
    clean = max(tc.x_misses(good["gx"], *args(0)), key=lambda m: m[1])
    print(f"{k}: wrong row {wrong_row}, shifted {shifted}, summed {summed}; the adjoint itself {clean}")
    assert clean[1] <= 1.0
    assert wrong_row[1] >= 10.0 and shifted[1] >= 10.0 and summed[1] >= 10.0
