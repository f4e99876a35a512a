"""CPU checks of tests/train_kernel_cases.py: the integer cases are exact in fp32 and not trivial, the NumPy reference is
torch autograd's, and the row counts derived from the source are the ones the GPU tests were written for."""
import numpy as np
import pytest

import train_kernel_cases as tc

ALL_Q = tc.SMALL_Q + (tc.Q_A, tc.Q_B)


@pytest.fixture(scope="module")
def stats():
    """(name, Q) -> (out, dW, db, stats) of every integer case, computed once"""
    memo = {}

    def get(name, Q):
        if (name, Q) not in memo:
            c = tc.int_case(name, Q)
            memo[name, Q] = tc.reference(c["dims"], c["acts"], c["Ws"], c["bs"], c["x"], c["dout"], stats=True)
        return memo[name, Q]
    return get


def test_row_counts_of_the_shipped_build():
    c = tc.parse_constants()
    assert (c["KR_FUSED_FT"], c["FW2"], c["FW3"], c["BW3"], c["LDS_WGS"], c["FUSED_GRID"]) == (2, 8, 8, 8, 256, 4096)
    assert (tc.FR, tc.Q_A, tc.Q_B) == (32, 65573, 131297)
    assert tc.Q_A == 2048 * tc.FR + tc.FR + 5 and tc.Q_B == 2 * 2048 * tc.FR + 7 * tc.FR + 1
    nblk = lambda q: (q + tc.FR - 1) // tc.FR
    assert nblk(tc.Q_A) == 2048 + 2 and nblk(tc.Q_B) == 4104 > 4096
    assert 2 * nblk(tc.ONE_TRIP_SLICE) <= 2048  # one trip with 32- and with 64-row blocks
    assert tc.rows_for(tc.Q_B, 3) == 131298 and tc.rows_for(tc.Q_B, 4) == 131300
    # the other build of the row blocks (KR_FUSED_FT = 4) gives the row count the integer cases were first checked at
    assert tc.row_counts(dict(c, KR_FUSED_FT=4))[2] == 262593


@pytest.mark.parametrize("gone", ["constexpr int FW3 = 8;", "(w < 256 ? w : 256)", "(nblk < 4096 ? nblk : 4096)",
                                  "#define KR_FUSED_FT 2"])
def test_a_changed_cap_fails_loudly(gone):
    with open(tc.FUSED_SRC) as f:
        text = f.read()
    assert gone in text
    with pytest.raises(AssertionError, match="pattern for"):
        tc.parse_constants(text.replace(gone, "/* rewritten */"))
    # a cap raised so far that Q_B is one trip again is refused too
    with pytest.raises(AssertionError, match="no longer"):
        tc.row_counts(dict(tc.parse_constants(), FUSED_GRID=8192))


@pytest.mark.parametrize("name", list(tc.INT_NETS))
def test_integer_cases_are_exact_in_fp32(stats, name):
    """Every inner product's absolute terms add up to less than 2^24 - the sum is then exact in fp32 in any order - and
    every value is an integer of {-1, 0, 1} on the way in."""
    for Q in ALL_Q:
        c = tc.int_case(name, Q)
        for a in c["Ws"] + c["bs"] + [c["x"], c["dout"]]:
            assert a.dtype == np.float32 and set(np.unique(a)) <= {-1.0, 0.0, 1.0}
        assert not c["x"][:, c["dims"][0]:].any() and not c["dout"][:, c["dims"][-1]:].any()
        out, dW, db, st = stats(name, Q)
        assert st["worst_abs_sum"] < 2.0 ** 24 / 64, (Q, st)  # (1.4e5 at most: a factor 100 below 2^24)
        for a in [out] + dW + db:
            assert np.array_equal(a, np.rint(a)) and np.array_equal(a.astype(np.float32).astype(np.float64), a)


@pytest.mark.parametrize("name", list(tc.INT_NETS))
def test_integer_cases_are_not_trivial(stats, name):
    """Conditions on the reference (not measurements of a kernel): a third of the hidden units is active, and the
    gradient blocks are dense enough that a row dropped anywhere shows.  The first layer of the H = 512 / 600 networks is
    the exception: with weight density 0.03 half of their hidden units feed no output, so that half of dW1 / db1 is 0."""
    wide = name in ("512", "600")
    for Q in ALL_Q:
        out, dW, db, st = stats(name, Q)
        nz = [float((g != 0).mean()) for pair in zip(dW, db) for g in pair]
        assert (out != 0).mean() > 0.8
        assert min(nz) > 0.0, (Q, nz)                 # every block of every case holds a nonzero integer
        if Q >= 31:
            assert 0.25 < st["active"] < 0.5, (Q, st)
            assert min(nz) > 0.1, (Q, nz)
        if Q >= 4099:
            assert min(nz[2:]) > 0.8 and min(nz[:2]) > (0.4 if wide else 0.8), (Q, nz)
        if Q >= tc.Q_A:
            assert min(nz[2:]) > 0.85 and min(nz[:2]) > (0.4 if wide else 0.85), (Q, nz)
            assert max(float(np.abs(g).max()) for g in dW) > 300


@pytest.mark.parametrize("act", ["tanh", "softplus", "relu", "elu"])
@pytest.mark.parametrize("dims", [[28, 64, 64, 25], [28, 100, 25], [32, 33, 20, 32]])
def test_numpy_reference_is_torch_autograd(act, dims):
    import torch
    rng = np.random.default_rng(3)
    n = len(dims) - 1
    Q = 33
    Ws = [(rng.standard_normal((dims[k + 1], dims[k])) / np.sqrt(dims[k])).astype(np.float32) for k in range(n)]
    bs = [(0.1 * rng.standard_normal(dims[k + 1])).astype(np.float32) for k in range(n)]
    x = np.zeros((Q, 32), np.float32)
    x[:, :dims[0]] = rng.standard_normal((Q, dims[0]))
    dout = np.zeros((Q, 32), np.float32)
    dout[:, :dims[-1]] = rng.standard_normal((Q, dims[-1]))
    acts = [tc.ACT_CODE[act]] * (n - 1) + [tc.NONE]
    out, dW, db = tc.reference(dims, acts, Ws, bs, x, dout, chunk=16)  # (three row chunks, the last one ragged)
    fn = {"tanh": torch.tanh, "softplus": torch.nn.functional.softplus, "relu": torch.relu, "elu": torch.nn.functional.elu}[act]
    Wt = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in Ws]
    bt = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    a = torch.tensor(x[:, :dims[0]], dtype=torch.float64)
    for k in range(n):
        a = a @ Wt[k].t() + bt[k]
        if k < n - 1:
            a = fn(a)
    (a * torch.tensor(dout[:, :dims[-1]], dtype=torch.float64)).sum().backward()
    close = lambda got, want: np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    assert close(out, a.detach().numpy())
    for k in range(n):
        assert close(dW[k], Wt[k].grad.numpy()) and close(db[k], bt[k].grad.numpy()), k


def test_real_cases():
    for name in tc.REAL_NETS:
        dims, acts, Ws, bs = tc.real_net(name)
        assert dims[0] == 28 and dims[-1] == 25 and acts[-1] == tc.NONE and len(Ws) == len(dims) - 1
        assert all(w.dtype == np.float32 and (w < 0).mean() > 0.4 for w in Ws)   # signed: not the nearly linear regime
    x, dout, base, target = tc.real_rows(99)
    assert x.shape == (99, 32) and not x[:, 28:].any() and not dout[:, 25:].any()
    assert base[:, 3].mean() > 1.5 and target[:, 3].mean() > 1.5
