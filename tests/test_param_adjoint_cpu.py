"""CPU tier of the parameter adjoint (kr_step_vjp_par_batch, kr_simulate_vjp_par_batch, krod_grad's physical gradients):
the C ABI surface, the argument checks that need no device, and the recursion the kernel implements - restated in NumPy
(param_adjoint_cases.numpy_param_adjoint) - held to the fixture the GPU tests compare with.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import param_adjoint_cases as pc
import step_adjoint_cases as sc
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = ("kr_step_vjp_par_batch", "kr_simulate_vjp_par_batch")


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_par_symbols_declared_exported_and_bound(lib):
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
        assert "g_par" in proto.group(1) and "use_nn" not in proto.group(1)
    assert re.search(r"#define\s+KR_PAR\s+43\b", src) and kn.KR_PAR == pc.KR_PAR == 43
    # the Python list of blocks is the order and layout of struct kr_params, and the tests' own
    assert [(n, o, s) for n, s, o in kn.PAR_BLOCKS] == [(n, o, s) for n, o, _, s in pc.PAR_BLOCKS]
    fields = [f[0] for f in kn.KrParams._fields_ if f[0] in pc.BLOCK_NAMES]
    assert fields == ["L", "E", "r", "rho", "vstar", "g", "Bse", "Bbt", "C", "tendon_dirs"]  # (L leads the struct; g_par keeps E r rho L)
    v = np.arange(2 * 43, dtype=np.float64).reshape(2, 43)
    parts = kn.split_par(v)
    assert parts["L"].shape == (2,) and parts["Bbt"].shape == (2, 3, 3) and parts["tendon_dirs"].shape == (2, 4, 3)
    assert parts["Bbt"][1, 2, 1] == 43 + 19 + 7 and parts["C"][0, 2] == 30
    # what the calls do not serve is said where they are declared
    doc = text[text.index("gradient of the rod's material parameters"):]
    for word in ("MLP-on", "RK4", "del_t", "table"):
        assert word in doc, word
    # a null handle needs no device: KR_E_ARG with a message, and no output byte is written
    out = (ctypes.c_double * 43)(*([7.0] * 43))
    buf = (ctypes.c_double * 64)()
    assert lib.kr_step_vjp_par_batch(None, 1, kn.KR_EULER, buf, buf, buf, buf, buf, out, out, out, out, out, None, None, kn.KR_F64,
                                     None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert lib.kr_simulate_vjp_par_batch(None, 1, 1, kn.KR_EULER, buf, buf, None, out, None, out, out, out, None, None, kn.KR_F64,
                                         None) == kn.KR_E_ARG
    assert list(out) == [7.0] * 43


class _Robot:
    """stands in for a CosseratRod in the checks that come before any device work"""
    _use_nn = False

    def _native(self):
        raise AssertionError("the argument checks come before the device is touched")

    def compute_intermediate_terms(self):
        raise AssertionError("the argument checks come before the robot is written")


def test_simulate_tips_physical_checks_its_arguments():
    import torch
    import krod_grad as kg
    import krod_native as kn
    r = _Robot()
    ctl = torch.zeros((2, 3, 4))
    ok = {"E": torch.tensor(1e9)}
    with pytest.raises(kn.KrError, match="unknown parameter 'del_t'"):
        kg.simulate_tips_physical(r, ctl, {"del_t": torch.tensor(0.05)})
    with pytest.raises(kn.KrError, match=r"theta\['Bbt'\] must have shape \(3, 3\)"):
        kg.simulate_tips_physical(r, ctl, {"E": torch.tensor(1e9), "Bbt": torch.zeros(3)})
    with pytest.raises(kn.KrError, match="must have shape"):
        kg.simulate_tips_physical(r, ctl, {"tendon_dirs": torch.zeros((3, 4))})
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_physical(r, ctl, {"E": 1e9})
    with pytest.raises(kn.KrError, match="non-empty dict"):
        kg.simulate_tips_physical(r, ctl, {})
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_physical(r, np.zeros((2, 3, 4)), ok)
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.simulate_tips_physical(r, torch.zeros((2, 3, 5)), ok)
    with pytest.raises(kn.KrError, match="unsupported dtype"):
        kg.simulate_tips_physical(r, ctl, ok, dtype="f16")
    nn = _Robot()
    nn._use_nn = True
    with pytest.raises(kn.KrError, match="MLP on is not served"):
        kg.simulate_tips_physical(nn, ctl, ok)
    with pytest.raises(kn.KrError, match="MLP on is not served"):
        kg.rollout_grad(nn, np.zeros((2, 3, 4)), np.zeros((4, 2, 5, kn.KR_SLOTS)), g_tips=np.zeros((2, 3, 3)), physical=True)
    assert set(kg.PHYSICAL_SHAPES) == set(pc.BLOCK_NAMES)


def test_fixture_covers_the_cases_and_resolves_every_block():
    """param_adjoint.npz holds every case at the kept rung and at twice it; every block's tolerance is at most 1e-2 of the
    block's largest entry; the rungs are the ladder's; the slack tendon's row is exactly zero in both estimates."""
    g = load_golden("param_adjoint")
    keys = [pc.step_key(ps, N, rod, state) for ps, N, rods, state in pc.STEP_CASES for rod in range(rods)]
    keys += ["zeroT_" + pc.step_key(*pc.ZERO_T_CASE)] + [pc.roll_key(*c) for c in pc.ROLLOUT_CASES + [pc.CPU_ROLLOUT_CASE]]
    worst = {}
    for k in keys:
        assert g[k + "fd_h"].shape == g[k + "fd_2h"].shape == (2, pc.KR_PAR), k
        assert g[k + "rung"].shape == g[k + "floor"].shape == (2, len(pc.PAR_BLOCKS)), k
        assert np.all(np.isfinite(g[k + "fd_h"])) and np.all(np.isfinite(g[k + "fd_2h"]))
        for c in range(2):
            for bi, (name, err, tol, size, zero) in enumerate(pc.block_report(g[k + "fd_h"][c], g[k + "fd_h"][c], g[k + "fd_2h"][c], g[k + "floor"][c])):
                assert float(g[k + "rung"][c, bi]) in pc.ladder_of(name), (k, name)
                if zero:  # (one interval: a block that only the SECOND point's map would feel - the drag from a base at rest, Bbt)
                    assert name in ("C", "Bbt") and "_N2_" in k, (k, name)
                    continue
                assert tol <= pc.MAX_REL_TOL * size, (k, c, name, tol, size)
                worst[name] = max(worst.get(name, 0.0), tol / size)
    print("largest tolerance / block size per block:", {n: f"{v:.1e}" for n, v in worst.items()})
    z = "zeroT_" + pc.step_key(*pc.ZERO_T_CASE)
    assert g[z + "tens"][2] == 0.0 and not np.any(g[z + "fd_h"][:, 37:40]) and not np.any(g[z + "fd_2h"][:, 37:40])


def _inner_tol(a, b, rnd):
    """what numpy_param_adjoint's own differences of the point map leave: ten times the disagreement of two inner steps, plus
    the rounding of the quotients themselves (a map linear in a parameter gives two estimates that agree, both rounded)"""
    return 10.0 * float(np.max(np.abs(a - b))) + float(np.max(rnd))


SMALL = [("plain", 2, 0, "sine30"), ("bc", 2, 1, "sine30"), ("plain", 3, 2, "sine30"), ("bc", 3, 0, "sine30"), ("fullB", 10, 0, "sine30"),
         ("plain", 10, 1, "straight")]


@pytest.mark.parametrize("ps,N,rod,state", SMALL)
def test_numpy_param_adjoint_against_the_fixture(ps, N, rod, state):
    """The recursion of the header in NumPy, its parameter tangents of the point map by differences of cosserat_oracle.ode
    through RodParams.derived(): every block equals the finite difference of the oracle's step within the fixture's tolerance
    plus the resolution of the inner differences (formed at two inner steps)."""
    fx, fp = load_golden("step_adjoint"), load_golden("param_adjoint")
    k = pc.step_key(ps, N, rod, state)
    P = sc.params(ps, N)
    x = sc.x_of(fx[k + "cur"], fx[k + "prev"], fx[k + "tens"], sc.bnd_of(P))
    for c in range(pc.N_COT):
        gbar = fx[k + "gbar"][c]
        (got, got2), _ = pc.numpy_param_adjoint(P, x, fx[k + "next"], gbar, h_scales=(1.0, 2.0))
        for bi, (name, off, n, _) in enumerate(pc.PAR_BLOCKS):
            a, b = fp[k + "fd_h"][c, off:off + n], fp[k + "fd_2h"][c, off:off + n]
            err = float(np.max(np.abs(got[off:off + n] - a)))
            tol = sc.block_tol(a, b, float(fp[k + "floor"][c, bi])) + _inner_tol(got[off:off + n], got2[off:off + n], pc.numpy_param_adjoint.round[off:off + n])
            print(f"{k} cot {c} {name:12s} err {err:.2e} tol {tol:.2e} size {np.max(np.abs(a)):.2e}")
            assert err <= tol, (k, c, name, err, tol)


def test_numpy_rollout_composition_needs_no_initial_state_term():
    """T = 3, N = 6: g_par summed over the step adjoints of the composition equals the finite difference of the oracle's
    rollout whose straight initial state is REBUILT from the perturbed parameters (its p scales with L) - L among the blocks:
    no step reads p of an earlier state, so the initial state adds no parameter term."""
    fp = load_golden("param_adjoint")
    ps, N, T = pc.CPU_ROLLOUT_CASE
    P, ctl, gbar = pc.roll_inputs(ps, N, T)
    states = pc.rollout_of(P, ctl)
    k = pc.roll_key(ps, N, T)
    for c in range(2):
        got, got2 = pc.numpy_rollout_param_adjoint(P, ctl, states, gbar[c], h_scales=(1.0, 2.0))
        for bi, (name, off, n, _) in enumerate(pc.PAR_BLOCKS):
            a, b = fp[k + "fd_h"][c, off:off + n], fp[k + "fd_2h"][c, off:off + n]
            err = float(np.max(np.abs(got[off:off + n] - a)))
            tol = sc.block_tol(a, b, float(fp[k + "floor"][c, bi])) + _inner_tol(got[off:off + n], got2[off:off + n], pc.numpy_rollout_param_adjoint.round[off:off + n])
            print(f"{k} cot {c} {name:12s} err {err:.2e} tol {tol:.2e} size {np.max(np.abs(a)):.2e}")
            assert err <= tol, (k, c, name, err, tol)
    # and the term that is NOT there would have been seen: p of the straight state moves with L
    dL = 1e-3
    s0p = sc.straight_state(pc.with_theta(P, pc.theta_of(P) + dL * np.eye(pc.KR_PAR)[3]))
    assert np.max(np.abs(s0p - sc.straight_state(P))) == pytest.approx(dL, rel=1e-9)
