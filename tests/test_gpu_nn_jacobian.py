"""The MLP's input Jacobian on the MI355X (kr_mlp_input_jacobian_batch, Handle.mlp_input_jacobian) against the chain rule
in NumPy fp64 (tests/nn_adjoint_cases.py).

The bound is derived, not fitted: entry by entry |device - NumPy| <= gamma (|W3| diag|act'2| |W2| diag|act'1| |W1|) with
gamma = (H1 + H2 + 28 + 64) 2^-53 (nn_adjoint_cases.jacobian_gamma).  Inputs are N(0, 1): the bound does not carry |x|,
so the rounding of the pre-activations, which scales with |W1| |x|, is covered by its `28` only for inputs of that size.
Every figure is printed before it is asserted.  The exact cases (integer weights, no activation) pin the operand and
result maps of v_mfma_f64_16x16x4_f64, which a norm would not."""
import ctypes as C

import numpy as np
import pytest

import nn_adjoint_cases as nc
from gpu_helpers import make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def handle(torch_cuda):
    return make_robot(None, 10)._native()


def rows(Q, seed=3):
    return np.random.default_rng(seed).normal(size=(Q, 28))


@pytest.mark.parametrize("name", list(nc.NETWORKS))
def test_jacobian_against_the_chain_rule(torch_cuda, handle, name):
    """Q = 1, 5, 200: one row, a wavefront's group of four plus one, several workgroups with a ragged tail; a row's bits
    do not depend on the batch it rides in."""
    torch = torch_cuda
    mlp = nc.network(name)
    handle.set_mlp(mlp.weights, mlp.biases, mlp.acts)
    gamma = nc.jacobian_gamma(mlp)
    x200 = rows(200)
    got200 = None
    for Q in (1, 5, 200):
        x = x200[:Q]
        got = handle.mlp_input_jacobian(torch.as_tensor(x, device=DEV))
        assert got.shape == (Q, 25, 28) and got.dtype == torch.float64
        got = got.cpu().numpy()
        worst = 0.0
        for q in range(Q):
            ref, bound = nc.input_jacobian(mlp, x[q])
            err = np.abs(got[q] - ref)
            worst = max(worst, float(np.max(err / (gamma * bound + 1e-300))))
            assert np.all(err <= gamma * bound), (name, Q, q, float(err.max()))
        print(f"{name} Q={Q}: largest error / bound {worst:.3f} (gamma {gamma:.2e}, |J| max {np.abs(got).max():.2e})")
        if Q == 200:
            got200 = got
    for Q in (1, 5):
        again = handle.mlp_input_jacobian(torch.as_tensor(x200[:Q], device=DEV)).cpu().numpy()
        assert np.array_equal(again, got200[:Q])


@pytest.mark.parametrize("hidden", [(17,), (33, 20), (130,)])
def test_integer_weights_give_the_exact_product(torch_cuda, handle, hidden):
    """Asymmetric small-integer matrices, activation `none`: jac == W_L ... W_1 bit for bit, in both layouts' element
    types (the fp32 call rounds nothing here either)."""
    torch = torch_cuda
    mlp = nc.integer_mlp(hidden, 5)
    handle.set_mlp(mlp.weights, mlp.biases, mlp.acts)
    want = mlp.weights[0].astype(np.float64)
    for W in mlp.weights[1:]:
        want = W.astype(np.float64) @ want
    assert not np.array_equal(want[:25, :25], want[:25, :25].T)
    for dt in (torch.float64, torch.float32):
        got = handle.mlp_input_jacobian(torch.as_tensor(rows(7), device=DEV).to(dt)).cpu().numpy()
        for q in range(7):
            assert np.array_equal(got[q], want), (hidden, dt, q)


def test_f32_call_is_the_f64_call_rounded(torch_cuda, handle):
    torch = torch_cuda
    for name in ("elu64x64", "relu100"):
        mlp = nc.network(name)
        handle.set_mlp(mlp.weights, mlp.biases, mlp.acts)
        x = torch.as_tensor(rows(37), device=DEV).float()
        lo, hi = handle.mlp_input_jacobian(x), handle.mlp_input_jacobian(x.double())
        assert lo.dtype == torch.float32 and torch.equal(lo, hi.float())


def test_nonfinite_row_is_ordinary_input(torch_cuda, handle):
    """A NaN in one row: that row's entries are NaN (relu included, whose derivative compares), every other row is bit
    for bit the clean call."""
    torch = torch_cuda
    for name in ("relu100", "relu20x33", "tanh17", "elu64x64"):
        mlp = nc.network(name)
        handle.set_mlp(mlp.weights, mlp.biases, mlp.acts)
        x = torch.as_tensor(rows(21), device=DEV)
        clean = handle.mlp_input_jacobian(x)
        bad = x.clone()
        bad[6, 3] = float("nan")
        out = handle.mlp_input_jacobian(bad)
        keep = [q for q in range(21) if q != 6]
        assert torch.isnan(out[6]).all(), name
        assert torch.equal(out[keep], clean[keep]), name


def test_infinite_input_poisons_the_row(torch_cuda, handle):
    """An infinity is not a NaN: relu' and elu' of a = +-inf are 1 or 0, and at widths without padded units (64, 512) the
    products would come back finite.  The row is NaN in every entry all the same, every other row is the clean call."""
    torch = torch_cuda
    for name in ("elu64x64", "elu512", "relu100", "relu20x33"):
        mlp = nc.network(name)
        handle.set_mlp(mlp.weights, mlp.biases, mlp.acts)
        x = torch.as_tensor(rows(21), device=DEV)
        clean = handle.mlp_input_jacobian(x)
        for row, col, v in ((6, 3, float("inf")), (20, 27, float("-inf")), (0, 0, float("inf"))):
            bad = x.clone()
            bad[row, col] = v
            out = handle.mlp_input_jacobian(bad)
            keep = [q for q in range(21) if q != row]
            assert torch.isnan(out[row]).all(), (name, row, v)
            assert torch.equal(out[keep], clean[keep]), (name, row, v)


def test_refusals_leave_every_output_byte(torch_cuda):
    """KR_E_STATE without a network; KR_E_UNSUPPORTED for the 53-wide input, a shape outside the two families, an
    activation on the last layer; KR_E_ARG for null pointers, Q < 1, a bad dtype - each with a message and nothing written."""
    torch = torch_cuda
    import cosserat_oracle as orc
    import krod_native as kn
    h = make_robot(None, 10)._native()
    lib = h.lib
    x = torch.zeros((4, 28), dtype=torch.float64, device=DEV)
    jac = torch.full((4, 25, 28), 7.0, dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(Q=4, x_=x, jac_=jac, dtype=kn.KR_F64):
        return lib.kr_mlp_input_jacobian_batch(h._h, Q, p(x_), p(jac_), dtype, None)
    assert call() == kn.KR_E_STATE and b"no MLP" in lib.kr_last_error()
    rng = np.random.default_rng(0)

    def net(sizes, acts):
        return ([rng.normal(size=(sizes[k + 1], sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)],
                [np.zeros(sizes[k + 1], np.float32) for k in range(len(sizes) - 1)], acts)
    E, NONE = orc.ACT_ELU, orc.ACT_NONE
    for sizes, acts, word in (((28, 513, 25), (E, NONE), b"512"), ((28, 65, 64, 25), (E, E, NONE), b"64"),
                              ((28, 64, 65, 25), (E, E, NONE), b"64"), ((28, 16, 16, 16, 25), (E, E, E, NONE), b"layers"),
                              ((28, 16, 25), (E, E), b"last layer")):
        h.set_mlp(*net(sizes, acts))
        assert call() == kn.KR_E_UNSUPPORTED and word in lib.kr_last_error(), (sizes, lib.kr_last_error())
    h.set_mlp(*net((28, 16, 25), (E, NONE)))
    for kw, word in ((dict(x_=None), b"null"), (dict(jac_=None), b"null"), (dict(Q=0), b"Q < 1"), (dict(dtype=7), b"dtype")):
        assert call(**kw) == kn.KR_E_ARG and word in lib.kr_last_error(), (kw, lib.kr_last_error())
    torch.cuda.synchronize()
    assert bool((jac == 7).all())
    assert call() == 0  # (the same arguments are served once nothing is wrong)
    torch.cuda.synchronize()
    assert not bool((jac == 7).any())
    jac.fill_(7.0)
    rh = make_robot(None, 10)
    rh.nn_input_history = True
    hh = rh._native()
    hh.set_mlp(*net((53, 16, 25), (E, NONE)))
    assert lib.kr_mlp_input_jacobian_batch(hh._h, 4, p(x), p(jac), kn.KR_F64, None) == kn.KR_E_UNSUPPORTED
    assert b"nn_input_history" in lib.kr_last_error()
    torch.cuda.synchronize()
    assert bool((jac == 7).all())
    with pytest.raises(kn.KrError, match=r"\[Q, 28\]"):
        h.mlp_input_jacobian(torch.zeros((4, 27), dtype=torch.float64, device=DEV))
