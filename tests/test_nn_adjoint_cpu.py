"""CPU tier of the step adjoint with the residual MLP on (kr_step_vjp_nn_batch, kr_simulate_vjp_nn_batch, krod_grad's
rollout_grad_nn / simulate_tips_nn): the C ABI surface, the argument checks that need no device, and the mathematics -
the NumPy restatement of the recursion with J = Jp + Jn X and the weight-gradient rows, held against central differences
of the oracle's own step with the network in the sweep, re-derived here.  No kernel is launched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import nn_adjoint_cases as nc
import step_adjoint_cases as sc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = ("kr_step_vjp_nn_batch", "kr_simulate_vjp_nn_batch", "kr_mlp_input_jacobian_batch")


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_symbols_declared_exported_and_bound(lib):
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
    doc = text[text.index("the adjoint with the residual MLP on"):]
    assert doc.count("knode.py:70-100") >= 2 and doc.count("cosserat_ode.py:188-213") >= 2 and doc.count("cosserat_ode.py:178-184") >= 2
    for m in ("step_vjp_nn", "simulate_vjp_nn", "mlp_input_jacobian", "set_mlp_device"):
        assert hasattr(kn.Handle, m), m
    # a null handle needs no device: KR_E_ARG with a message, and no output byte is written
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    buf = (ctypes.c_double * 64)()
    assert lib.kr_step_vjp_nn_batch(None, 1, kn.KR_EULER, buf, buf, buf, buf, buf, out, out, out, out, None, None, out, out,
                                    kn.KR_F64, None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert lib.kr_simulate_vjp_nn_batch(None, 1, 1, kn.KR_EULER, buf, buf, None, out, None, out, out, None, None, out, out,
                                        kn.KR_F64, None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert list(out) == [7.0] * 4


class _Robot:
    """stands in for a CosseratRod in the checks that come before any device work"""
    _use_nn = True

    def _native(self):
        raise AssertionError("the argument checks come before the device is touched")


def test_krod_grad_checks_its_arguments_before_the_device():
    import torch
    import krod_grad as kg
    import krod_native as kn
    r = _Robot()
    ctl = np.zeros((2, 3, 4))
    states = np.zeros((4, 2, 5, kn.KR_SLOTS))
    with pytest.raises(kn.KrError, match="g_states and / or g_tips"):
        kg.rollout_grad_nn(r, ctl, states)
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.rollout_grad_nn(r, np.zeros((2, 3, 5)), states, g_tips=np.zeros((2, 3, 3)))
    with pytest.raises(kn.KrError, match="not a ring"):
        kg.rollout_grad_nn(r, ctl, states[:3], g_tips=np.zeros((2, 3, 3)))
    with pytest.raises(kn.KrError, match=r"g_tips must be"):
        kg.rollout_grad_nn(r, ctl, states, g_tips=np.zeros((2, 2, 3)))
    with pytest.raises(kn.KrError, match="nn.Linear order"):
        kg.rollout_grad_nn(r, ctl, states, g_tips=np.zeros((2, 3, 3)), params=[torch.zeros(3, 28)])
    with pytest.raises(kn.KrError, match="takes 5 inputs"):
        kg.simulate_tips_nn(r, torch.zeros(2, 3, 4), [torch.zeros(4, 28), torch.zeros(4), torch.zeros(25, 5), torch.zeros(25)])
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_nn(r, ctl, [torch.zeros(4, 28), torch.zeros(4), torch.zeros(25, 4), torch.zeros(25)])
    off = _Robot()
    off._use_nn = False
    with pytest.raises(kn.KrError, match="no MLP on"):
        kg.rollout_grad_nn(off, ctl, states, g_tips=np.zeros((2, 3, 3)))
    with pytest.raises(kn.KrError, match="no MLP on"):
        kg.simulate_tips_nn(off, torch.zeros(2, 3, 4), [])
    with pytest.raises(kn.KrError, match="MLP on is not served"):  # (the physics-only functions keep refusing, and say where to go)
        kg.rollout_grad(r, ctl, states, g_tips=np.zeros((2, 3, 3)))


_cases = {}


def small_case(ps, N, net):
    """one rod, state sine30 of the model with its network, the three cotangents; finite differences in x and along the
    weight directions at H and 2 H - derived once per module"""
    if (ps, N, net) not in _cases:
        P, mlp = sc.params(ps, N), nc.network(net)
        prev, cur, tens = nc.step_inputs_nn(ps, N, 0, "sine30", mlp)
        x = sc.x_of(cur, prev, tens, sc.bnd_of(P))
        nxt, G = nc.oracle_step_nn(P, mlp, x, np.zeros(6))
        gbar = sc.cotangents(N, 100 + N)
        gb = gbar.reshape(3, -1)
        fx = lambda xx: gb @ nc.oracle_step_nn(P, mlp, xx, G)[0].ravel()
        fw = lambda m: gb @ nc.oracle_step_nn(P, m, x, G)[0].ravel()
        dirs = nc.weight_directions(mlp)
        _cases[(ps, N, net)] = dict(
            P=P, mlp=mlp, x=x, nxt=nxt, gbar=gbar, dirs=dirs,
            fd=[sc.fd_columns(fx, x, range(x.size), h).T for h in (sc.H, 2 * sc.H)],
            wfd=[nc.weight_fd(fw, mlp, dirs, h) for h in (sc.H, 2 * sc.H)])
    return _cases[(ps, N, net)]


SMALL = [("plain", 3, "tanh17"), ("bc", 4, "elu64x64")]


@pytest.mark.parametrize("ps,N,net", SMALL)
def test_numpy_restatement_against_finite_differences(ps, N, net):
    """J = Jp + Jn X in the recursion, Jp from the 50-digit derivative oracle (with the central-difference point_jacobian the
    same check misses by up to 12 x: that helper's error, not the formula's): every block by the project's rule, ten times
    the H / 2 H disagreement plus fd_floor.  The weight gradient is the MLP backward pass over the rows (x_j, c_j)."""
    c = small_case(ps, N, net)
    worst = 0.0
    for k in range(3):
        gx, resid, X, Cc = nc.numpy_step_adjoint_nn(c["P"], c["mlp"], c["x"], c["nxt"], c["gbar"][k])
        assert resid <= 1e-10
        floor = sc.fd_floor(c["gbar"][k], c["nxt"])
        for name, err, tol, size in sc.block_report(gx, c["fd"][0][k], c["fd"][1][k], N, floor):
            print(f"{ps} N={N} {net} cotangent {k} {name:14s} err {err:.3e} tol {tol:.3e} size {size:.3e}")
            worst = max(worst, err / tol)
            assert err <= tol, (name, err, tol)
        gw = c["dirs"] @ nc.mlp_backward_rows(c["mlp"], X, Cc)
        a, b = c["wfd"][0][:, k], c["wfd"][1][:, k]
        for lo in range(0, len(gw), 6):  # (a block per layer: two directions and four corners)
            err, tol = np.max(np.abs(gw[lo:lo + 6] - a[lo:lo + 6])), sc.block_tol(a[lo:lo + 6], b[lo:lo + 6], floor)
            print(f"{ps} N={N} {net} cotangent {k} weights layer {lo // 6} err {err:.3e} tol {tol:.3e} size {np.max(np.abs(a[lo:lo + 6])):.3e}")
            worst = max(worst, err / tol)
            assert err <= tol, (lo, err, tol)
    print(f"largest error / tolerance {worst:.3f}")


@pytest.mark.parametrize("ps,N,net", SMALL)
def test_physics_only_adjoint_fails_the_same_comparison(ps, N, net):
    """The fixture can see the network: the recursion with Jp alone, on the same inputs, misses the same tolerances."""
    c = small_case(ps, N, net)
    gx, _ = sc.numpy_step_adjoint(c["P"], c["x"], c["nxt"], c["gbar"][0], jac=sc.jacobian_exact)
    floor = sc.fd_floor(c["gbar"][0], c["nxt"])
    rows = sc.block_report(gx, c["fd"][0][0], c["fd"][1][0], N, floor)
    ratio = max(err / tol for _, err, tol, _ in rows)
    print(f"{ps} N={N} {net}: physics-only adjoint misses by a factor {ratio:.3e}")
    assert ratio > 1e3
