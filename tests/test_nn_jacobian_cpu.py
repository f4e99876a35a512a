"""CPU tier of the MLP's input Jacobian (kr_mlp_input_jacobian_batch): the C ABI surface, and the NumPy closed form the GPU
test compares with (tests/nn_adjoint_cases.py) held against central differences of the oracle's own network evaluation.
No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import nn_adjoint_cases as nc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
NAME = "kr_mlp_input_jacobian_batch"


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_symbol_declared_exported_and_bound(lib):
    import krod_native as kn
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert proto, f"{NAME} is not declared in include/knode_rod.h"
    assert hasattr(ctypes.CDLL(kn.LIB_PATH), NAME), f"{NAME} is not exported by the library"
    assert NAME in kn.EXPORTED_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == proto.group(1).count(",") + 1
    # the entry point cites the reference lines it differentiates
    doc = text[text.index("The input Jacobian of the residual MLP"):text.index("int " + NAME)]
    assert "cosserat_ode.py:90-112" in doc and "cosserat_ode.py:178-184" in doc and "knode.py:70-100" in doc
    assert hasattr(kn.Handle, "mlp_input_jacobian")
    # a null handle needs no device: KR_E_ARG with a message, and no output byte is written
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    buf = (ctypes.c_double * 28)()
    assert fn(None, 1, buf, out, kn.KR_F64, None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert list(out) == [7.0] * 4


@pytest.mark.parametrize("name", list(nc.NETWORKS))
def test_closed_form_against_central_differences(name):
    """dNN/dx of nn_adjoint_cases.input_jacobian against (NN(x + h e_i) - NN(x - h e_i)) / 2h of cosserat_oracle.mlp_eval at
    h and 2 h: the tolerance is ten times the two estimates' disagreement plus the quotient's own resolution.  relu is
    piecewise linear: its two estimates agree to rounding unless a kink lies within 2 h of x, which the inputs avoid."""
    import cosserat_oracle as orc
    mlp = nc.network(name)
    x = np.random.default_rng(3).normal(size=28)
    J, B = nc.input_jacobian(mlp, x)
    assert J.shape == (25, 28) and np.all(B >= np.abs(J) * (1 - 1e-12))

    def fd(h):
        cols = []
        for i in range(28):
            e = np.zeros(28)
            e[i] = h
            cols.append((orc.mlp_eval(mlp, x + e) - orc.mlp_eval(mlp, x - e)) / (2 * h))
        return np.array(cols).T
    h = 1e-5
    a, b = fd(h), fd(2 * h)
    floor = 2.0 ** -52 * np.max(np.abs(orc.mlp_eval(mlp, x))) * 64 / (2 * h)
    tol = 10.0 * np.max(np.abs(a - b)) + floor
    err = np.max(np.abs(J - a))
    print(f"{name}: err {err:.3e} tol {tol:.3e} size {np.max(np.abs(J)):.3e}")
    assert err <= tol


def test_activation_derivative_forms():
    import cosserat_oracle as orc
    a = np.linspace(-30, 30, 241)
    assert np.allclose(nc.act_derivative(orc.ACT_TANH, a[60:181]), 1 - np.tanh(a[60:181]) ** 2, rtol=0, atol=4e-16)
    assert np.allclose(nc.act_derivative(orc.ACT_SOFTPLUS, a), 1 / (1 + np.exp(-a)), rtol=1e-15, atol=0)
    assert nc.act_derivative(orc.ACT_TANH, np.array([25.0]))[0] > 0  # (1 - tanh^2 is exactly 0 there)
    assert np.array_equal(nc.act_derivative(orc.ACT_RELU, np.array([-1.0, 0.0, 2.0])), [0.0, 0.0, 1.0])
    assert np.array_equal(nc.act_derivative(orc.ACT_ELU, np.array([0.0, 3.0])), [1.0, 1.0])


def test_integer_networks_are_asymmetric_and_exact():
    for hidden in ((17,), (33, 20), (130,)):
        mlp = nc.integer_mlp(hidden, 5)
        prod = mlp.weights[0].astype(np.float64)
        for W in mlp.weights[1:]:
            prod = W.astype(np.float64) @ prod
            n = min(W.shape)
            assert not np.array_equal(W[:n, :n], W[:n, :n].T)
        J, _ = nc.input_jacobian(mlp, np.ones(28))
        assert np.array_equal(J, prod) and np.all(prod == np.round(prod)) and np.max(np.abs(prod)) < 2 ** 40
