"""CPU tier of the step adjoint (kr_step_vjp_batch, kr_simulate_vjp_batch, krod_grad): the C ABI surface, the argument
checks that need no device, and the finite-difference machinery the GPU tests' expected values come from
(tests/step_adjoint_cases.py) held against itself.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import step_adjoint_cases as sc
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = ("kr_step_vjp_batch", "kr_simulate_vjp_batch")


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_adjoint_symbols_declared_exported_and_bound(lib):
    import krod_native as kn
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert proto, f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int
        assert len(getattr(lib, name).argtypes) == proto.group(1).count(",") + 1, name
    # every entry point cites the reference lines it differentiates
    doc = text[text.index("adjoint of a solved step"):]
    assert doc.count("knode.py:70-100") >= 2 and doc.count("cosserat_ode.py:188-213") >= 2
    assert hasattr(kn.Handle, "step_vjp") and hasattr(kn.Handle, "simulate_vjp")
    # a null handle needs no device: KR_E_ARG with a message, and no output byte is written
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    buf = (ctypes.c_double * 64)()
    assert lib.kr_step_vjp_batch(None, 1, kn.KR_EULER, buf, buf, buf, buf, buf, out, out, out, out, None, None, 0, kn.KR_F64,
                                 None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert lib.kr_simulate_vjp_batch(None, 1, 1, kn.KR_EULER, buf, buf, None, out, None, out, out, None, None, 0, kn.KR_F64,
                                     None) == kn.KR_E_ARG
    assert list(out) == [7.0] * 4


class _Robot:
    """stands in for a CosseratRod in the checks that come before any device work"""
    _use_nn = False

    def _native(self):
        raise AssertionError("the argument checks come before the device is touched")


def test_krod_grad_imports_and_checks_its_arguments():
    import torch
    import krod_grad as kg
    import krod_native as kn
    r = _Robot()
    ctl = np.zeros((2, 3, 4))
    states = np.zeros((4, 2, 5, kn.KR_SLOTS))
    with pytest.raises(kn.KrError, match="g_states and / or g_tips"):
        kg.rollout_grad(r, ctl, states)
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.rollout_grad(r, np.zeros((2, 3, 5)), states, g_tips=np.zeros((2, 3, 3)))
    with pytest.raises(kn.KrError, match="not a ring"):  # three slots where T + 1 = 4 are needed
        kg.rollout_grad(r, ctl, states[:3], g_tips=np.zeros((2, 3, 3)))
    with pytest.raises(kn.KrError, match="g_tips must be"):
        kg.rollout_grad(r, ctl, states, g_tips=np.zeros((2, 2, 3)))
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips(r, ctl)
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.simulate_tips(r, torch.zeros((2, 0, 4)))
    with pytest.raises(kn.KrError, match="unsupported dtype"):
        kg.simulate_tips(r, torch.zeros((2, 3, 4)), dtype="f16")
    nn = _Robot()
    nn._use_nn = True
    for call in (lambda: kg.rollout_grad(nn, ctl, states, g_tips=np.zeros((2, 3, 3))), lambda: kg.simulate_tips(nn, torch.zeros((2, 3, 4)))):
        with pytest.raises(kn.KrError, match="MLP on is not served"):
            call()


def test_rollout_fd_from_step_blocks_equals_fd_of_the_rollout():
    """N = 10, T = 3: the rollout gradient assembled by the chain rule from PER-STEP finite-difference blocks equals the
    finite difference of the whole rollout.  Each side is formed at H and 2 H; the tolerance of a block is ten times the
    disagreement of the whole-rollout estimates plus that of the assembled ones (both carry their own error), plus the
    resolution of the quotient (step_adjoint_cases.fd_floor)."""
    N, T = 10, 3
    P = sc.params("bc", N)
    ctl = sc.orc.batch_sine_controls(1, T, P.del_t, 11)[0]
    bnd = sc.bnd_of(P)
    s0 = sc.straight_state(P)
    states = sc.oracle_rollout(P, ctl, s0)
    gbar = sc.rollout_cotangents(T, N, 5)[0]

    def whole(h):
        x = np.concatenate([ctl.ravel(), bnd])
        fn = lambda xx: float(np.sum(gbar * sc.oracle_rollout(P, xx[:4 * T].reshape(T, 4), s0, bnd=xx[4 * T:])))
        return sc.fd_columns(fn, x, range(len(x)), h)

    def assembled(h):
        # step Jacobians d next[N, 25 slots] / d x by finite differences of the step, composed backwards in time
        g = gbar.copy()
        g_ctl, g_bnd = np.zeros((T, 4)), np.zeros(19)
        for t in range(T - 1, -1, -1):
            prev = states[t - 1] if t > 0 else states[0]
            x = sc.x_of(states[t], prev, ctl[t], bnd)
            G = sc.oracle_step(P, x, np.zeros(6))[1]
            J = sc.fd_columns(lambda xx: sc.oracle_step(P, xx, G)[0].ravel(), x, range(len(x)), h)  # [inputs, N * 28]
            gx = sc.split_grad(J @ g[t + 1].ravel(), N)
            g[t, :, :12] += gx["cur"]
            g[max(t - 1, 0), :, :12] += gx["prev"]
            g_ctl[t], g_bnd = gx["tens"], g_bnd + gx["bnd"]
        return np.concatenate([g_ctl.ravel(), g_bnd])
    w1, w2, a1, a2 = whole(sc.H), whole(2 * sc.H), assembled(sc.H), assembled(2 * sc.H)
    floor = sc.fd_floor(gbar, states)
    for name, sl in [("g_ctl", slice(0, 4 * T))] + [("g_bnd." + n, slice(4 * T + s.start, 4 * T + s.stop)) for n, a, s in
                                                     ((b[0][6:], b[1], b[2]) for b in sc.BLOCKS if b[1] == "bnd")]:
        err = np.max(np.abs(w1[sl] - a1[sl]))
        tol = sc.block_tol(w1[sl], w2[sl], floor) + sc.block_tol(a1[sl], a2[sl], floor)
        print(f"{name:14s} err {err:.2e} tol {tol:.2e} size {np.max(np.abs(w1[sl])):.2e}")
        assert err <= tol, (name, err, tol)


def test_numpy_adjoint_against_the_derivative_oracle_and_the_fd():
    """The NumPy restatement of the adjoint recursion (step_adjoint_cases.numpy_step_adjoint), N = 4: its point Jacobians
    are held to oracle/ode_derivative.py (50 digits), and with those Jacobians every output block equals the finite
    difference of the oracle's step within the tolerance rule; resid is at rounding level (cond(M) ~ 2)."""
    import ode_derivative as od
    N = 4
    for ps in ("bc", "fullB"):
        P = sc.params(ps, N)
        prev, cur, tens = sc.step_inputs(ps, N, 1, "sine30")
        x = sc.x_of(cur, prev, tens, sc.bnd_of(P))
        nxt, G = sc.oracle_step(P, x, np.zeros(6))
        D = P.derived()
        y, _ = sc.unpack(nxt)
        hist = D.c1 * cur + D.c2 * prev
        yh = np.zeros(19)
        yh[13:19] = hist[1, 0:6]
        tf = sc.orc.tendon_force(D, tens)
        Jfd, Jmp = sc.point_jacobian(D, y[:, 1], yh, hist[1, 6:12], tf), sc.jacobian_exact(D, y[:, 1], yh, hist[1, 6:12], tf)
        # central differences at 1e-6 in fp64 of a map whose intermediates reach |Kse vstar| (8.7e4): each evaluation is
        # rounded at 2^-53 of that, a few operations deep, and the quotient divides by 2e-6
        bound = 8 * 2.0 ** -53 * np.max(np.abs(D.Kse_vstar)) / 1e-6
        print(f"{ps}: point Jacobian, finite differences against 50 digits: {np.max(np.abs(Jfd - Jmp)):.2e} (bound {bound:.2e})")
        assert np.max(np.abs(Jfd - Jmp)) <= bound
        assert Jmp.shape == (od.N_OUT, 34)
        gb = sc.cotangents(N, 100 + N)
        for c in range(3):
            fn = lambda xx: gb[c].ravel() @ sc.oracle_step(P, xx, G)[0].ravel()
            a, b = sc.fd_columns(fn, x, range(len(x)), sc.H), sc.fd_columns(fn, x, range(len(x)), 2 * sc.H)
            got, resid = sc.numpy_step_adjoint(P, x, nxt, gb[c], jac=sc.jacobian_exact)
            assert resid <= 1e-10
            for name, err, tol, size in sc.block_report(got, a, b, N, sc.fd_floor(gb[c], nxt)):
                print(f"{ps} cot {c} {name:14s} err {err:.2e} tol {tol:.2e} size {size:.2e}")
                assert err <= tol, (ps, c, name, err, tol)


def test_fixture_covers_the_cases_and_agrees_with_itself():
    """step_adjoint.npz holds every case of step_adjoint_cases at both step sizes, and its stored next state is the
    oracle's step of its stored inputs (re-solved here for the smallest case)."""
    g = load_golden("step_adjoint")
    assert float(g["H"]) == sc.H
    for ps, N, rods, state in sc.STEP_CASES:
        for rod in range(rods):
            k = sc.case_key(ps, N, state) + f"_r{rod}_"
            assert g[k + "fd_h"].shape == g[k + "fd_2h"].shape == (3, 24 * N + 23), k
            assert np.array_equal(g[k + "gbar"], sc.cotangents(N, 100 + N))
            assert np.all(np.isfinite(g[k + "fd_h"])) and np.all(np.isfinite(g[k + "fd_2h"]))
    for ps, N, T in sc.ROLLOUT_CASES:
        k = f"roll_{ps}_N{N}_T{T}_"
        assert g[k + "fd_h"].shape == g[k + "fd_2h"].shape == (2, 4 * T + 19 + len(sc.rollout_state0_entries(N))), k
    ps, N, state = "bc", 2, "sine30"
    k = sc.case_key(ps, N, state) + "_r0_"
    P = sc.params(ps, N)
    nxt, _ = sc.oracle_step(P, sc.x_of(g[k + "cur"], g[k + "prev"], g[k + "tens"], sc.bnd_of(P)), np.zeros(6))
    assert np.max(np.abs(nxt - g[k + "next"])) < 1e-12
