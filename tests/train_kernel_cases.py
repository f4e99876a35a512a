"""Shared cases of the training-kernel tests (no test module; importable without a GPU).

Integer networks: every value of x, the weights, the biases and dout lies in {-1, 0, 1}, the hidden activation is relu and
the last layer has none.  Every inner product of the forward pass, the backward pass and the weight gradients is then a sum
of integers whose absolute values add up to far less than 2^24, so it is exact in fp32 IN ANY ORDER - whatever a kernel's
tiling, its slab split or the arrival order of its atomics - and the device result must equal the fp64 NumPy reference
bit for bit.  One wrong, missing or doubled row changes an integer.

Row counts: the forward and the three-layer backward kernels deal row blocks of FR = 16 KR_FUSED_FT rows to at most
256 workgroups of 8 wavefronts, mlp_fwd_fused_kernel to at most 4096 one-wavefront workgroups.  Q_A and Q_B are derived
from those constants as they stand in csrc/kr_mlp_fused.hip, so that a later change of a cap cannot quietly turn the
tests that use them back into one-trip tests."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_SRC = os.path.join(ROOT, "knode-cosserat_amd", "csrc", "kr_mlp_fused.hip")

NONE, TANH, SOFTPLUS, RELU, ELU = range(5)
ACT_CODE = {"none": NONE, "tanh": TANH, "softplus": SOFTPLUS, "relu": RELU, "elu": ELU}

_PATTERNS = {
    "KR_FUSED_FT": r"#ifndef KR_FUSED_FT\s*\n#define KR_FUSED_FT (\d+)\s*\n#endif",
    "FW2": r"constexpr int FW2 = (\d+);",
    "FW3": r"constexpr int FW3 = (\d+);",
    "BW3": r"constexpr int BW3 = (\d+);",
    # static int fwd_lds_wgs(int64_t nblk, int waves) { ...; return (int)(w < 256 ? w : 256); }
    "LDS_WGS": r"static int fwd_lds_wgs\(int64_t nblk, int waves\) \{[^}]*?return \(int\)\(w < (\d+) \? w : \1\);",
    # fused_mlp_forward: const int grid = (int)(nblk < 4096 ? nblk : 4096);
    "FUSED_GRID": r"const int grid = \(int\)\(nblk < (\d+) \? nblk : \1\);",
    "BWD3_WGS": r"static int bwd3_wgs\(int64_t nblk\) \{ return fwd_lds_wgs\(nblk, (BW3)\); \}",
}


def parse_constants(text=None):
    """The caps of the row-block loops, read out of the source.  Raises when a pattern is no longer found."""
    if text is None:
        with open(FUSED_SRC) as f:
            text = f.read()
    out = {}
    for name, pat in _PATTERNS.items():
        m = re.findall(pat, text)
        if len(m) != 1:
            raise AssertionError(f"train_kernel_cases: pattern for {name} matches {len(m)} times in kr_mlp_fused.hip - the "
                                 "row-block loops changed; derive Q_A / Q_B anew before trusting the second-trip tests")
        out[name] = m[0] if name == "BWD3_WGS" else int(m[0])
    return out


def row_counts(c=None):
    """-> (FR, Q_A, Q_B).  With W = 256 x 8 wavefronts of the LDS kernels: Q_A = W FR + FR + 5 (a few wavefronts take a
    second block, ragged tail), Q_B = 2 W FR + 7 FR + 1 (every wavefront takes two blocks, some three; more row blocks than
    mlp_fwd_fused_kernel's grid cap)."""
    c = parse_constants() if c is None else c
    if c["KR_FUSED_FT"] not in (2, 4):
        raise AssertionError("KR_FUSED_FT must be 2 or 4")
    fr = 16 * c["KR_FUSED_FT"]
    waves = c["LDS_WGS"] * max(c["FW2"], c["FW3"], c["BW3"])
    qa = waves * fr + fr + 5
    qb = 2 * waves * fr + 7 * fr + 1
    nblk = lambda q: (q + fr - 1) // fr
    for fw in (c["FW2"], c["FW3"], c["BW3"]):
        w = c["LDS_WGS"] * fw
        if not (nblk(qa) > w and nblk(qb) > 2 * w):
            raise AssertionError("Q_A / Q_B no longer reach a second / third row block per wavefront")
    if not nblk(qb) > c["FUSED_GRID"]:
        raise AssertionError("Q_B no longer exceeds the grid cap of mlp_fwd_fused_kernel")
    return fr, qa, qb


FR, Q_A, Q_B = row_counts()
SMALL_Q = (1, 31, 32, 33, 4099)
ONE_TRIP_SLICE = 32768  # rows per slice of the batch-independence tests: 1024 / 512 blocks, one trip under either KR_FUSED_FT


def rows_for(Q, K):
    """The smallest multiple of K that is >= Q (kr_mlp_forward_loss / kr_train_epoch take S x K rows).  Q_B is prime to
    3 and 4; the few rows added stay inside its last row block, so the number of row blocks is unchanged."""
    q = (Q + K - 1) // K * K
    assert (q + FR - 1) // FR == (Q + FR - 1) // FR
    return q


# name -> (dims, weight-nonzero probability per layer)
INT_NETS = {
    "64x64": ([28, 64, 64, 25], (0.25, 0.125, 0.125)),    # three-layer LDS kernels
    "33x20": ([28, 33, 20, 25], (0.25, 0.2, 0.3)),        # ragged widths
    "100": ([28, 100, 25], (0.25, 0.125)),                # mlp_fwd2_kernel, two chunks, ragged
    "512": ([28, 512, 25], (0.25, 0.03)),                 # eight chunks
    "600": ([28, 600, 25], (0.25, 0.03)),                 # mlp_fwd_fused_kernel, c1 = 10
    "32x64x64x32": ([32, 64, 64, 32], (0.25, 0.125, 0.125)),  # 32 in, 32 out: mlp_fwd_fused_kernel, three layers
    "64to26": ([28, 64, 26], (0.25, 0.125)),              # 26 outputs, two layers: mlp_fwd_fused_kernel
}
FUSED_FWD_NETS = ("600", "32x64x64x32", "64to26")   # served by mlp_fwd_fused_kernel
QB_NETS = ("64x64", "33x20", "100", "512") + FUSED_FWD_NETS
P_X, P_DOUT = 0.25, 0.1


def _ternary(rng, shape, p):
    """-1 / +1 with probability p / 2 each, else 0"""
    return (rng.random(shape) < p) * (2.0 * (rng.random(shape) < 0.5) - 1.0)


@functools.lru_cache(maxsize=4)
def int_case(name, Q):
    """-> dict(dims, acts, Ws, bs, x [Q, 32], dout [Q, 32]) in float32; padding columns zero"""
    dims, probs = INT_NETS[name]
    rng = np.random.default_rng([list(INT_NETS).index(name), Q, 2024])
    n = len(dims) - 1
    Ws = [_ternary(rng, (dims[k + 1], dims[k]), probs[k]).astype(np.float32) for k in range(n)]
    bs = [rng.integers(-1, 2, size=dims[k + 1]).astype(np.float32) for k in range(n)]
    x = np.zeros((Q, 32), np.float32)
    x[:, :dims[0]] = _ternary(rng, (Q, dims[0]), P_X)
    dout = np.zeros((Q, 32), np.float32)
    dout[:, :dims[-1]] = _ternary(rng, (Q, dims[-1]), P_DOUT)
    return dict(name=name, dims=list(dims), acts=[RELU] * (n - 1) + [NONE], Ws=Ws, bs=bs, x=x, dout=dout)


def act_np(code, z):
    if code == NONE:
        return z
    if code == TANH:
        return np.tanh(z)
    if code == SOFTPLUS:
        return np.logaddexp(0.0, z)
    if code == RELU:
        return np.maximum(z, 0.0)
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def act_grad_np(code, z):
    if code == NONE:
        return np.ones_like(z)
    if code == TANH:
        return 1.0 - np.tanh(z) ** 2
    if code == SOFTPLUS:
        return 0.5 * (1.0 + np.tanh(0.5 * z))  # sigmoid
    if code == RELU:
        return (z > 0).astype(z.dtype)
    return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))


def reference(dims, acts, Ws, bs, x, dout, chunk=16384, stats=False):
    """Forward and backward of the MLP over the rows in fp64 (BLAS), in row chunks so that no [Q, H] image is held:
    -> out [Q, nout], dW[k], db[k].  stats = True additionally returns, for the exactness condition, the largest sum of
    absolute terms of any inner product (forward, backward, gradient; a gradient sum taken over ALL rows) and the
    fraction of active (> 0) hidden units."""
    n = len(dims) - 1
    W = [np.asarray(w, np.float64) for w in Ws]
    b = [np.asarray(v, np.float64) for v in bs]
    Q = x.shape[0]
    out = np.empty((Q, dims[-1]))
    dW = [np.zeros_like(w) for w in W]
    db = [np.zeros_like(v) for v in b]
    aW = [np.zeros_like(w) for w in W]
    adb = [np.zeros_like(v) for v in b]
    worst, active, hidden = 0.0, 0, 0
    for r0 in range(0, Q, chunk):
        a = [np.asarray(x[r0:r0 + chunk, :dims[0]], np.float64)]
        z = []
        for k in range(n):
            z.append(a[-1] @ W[k].T + b[k])
            a.append(act_np(acts[k], z[-1]))
            if stats:
                worst = max(worst, float((np.abs(a[k]) @ np.abs(W[k]).T + np.abs(b[k])).max()))
                if k < n - 1:
                    active += int((a[-1] > 0).sum())
                    hidden += a[-1].size
        out[r0:r0 + chunk] = z[-1]
        d = np.asarray(dout[r0:r0 + chunk, :dims[-1]], np.float64)
        for k in range(n - 1, -1, -1):
            dW[k] += d.T @ a[k]
            db[k] += d.sum(0)
            if stats:
                aW[k] += np.abs(d).T @ np.abs(a[k])
                adb[k] += np.abs(d).sum(0)
            if k > 0:
                if stats:
                    worst = max(worst, float((np.abs(d) @ np.abs(W[k])).max()))
                d = (d @ W[k]) * act_grad_np(acts[k - 1], z[k - 1])
    if stats:
        worst = max([worst] + [float(m.max()) for m in aW + adb])
        return out, dW, db, dict(worst_abs_sum=worst, active=active / max(hidden, 1))
    return out, dW, db


@functools.lru_cache(maxsize=4)
def int_reference(name, Q):
    c = int_case(name, Q)
    return reference(c["dims"], c["acts"], c["Ws"], c["bs"], c["x"], c["dout"])


# ---- real-valued networks -----------------------------------------------------------------------------------------------
# name -> (hidden widths, activation, gain) for nn_adjoint_cases.signed_mlp
REAL_NETS = {
    "64x64_elu": ((64, 64), "elu", 0.5),
    "33x20_softplus": ((33, 20), "softplus", 0.5),
    "100_tanh": ((100,), "tanh", 0.5),
    "512_elu": ((512,), "elu", 0.5),
}


@functools.lru_cache(maxsize=None)
def real_net(name, seed=23):
    """-> (dims, act codes, Ws, bs) of a signed network: weights gain N(0, 1) / sqrt(fan_in), biases 0.1 N(0, 1), fp32"""
    import nn_adjoint_cases as nc
    hidden, act, gain = REAL_NETS[name]
    mlp = nc.signed_mlp(hidden, act, gain, seed)
    Ws = [np.ascontiguousarray(w, np.float32) for w in mlp.weights]
    bs = [np.ascontiguousarray(b, np.float32) for b in mlp.biases]
    return [28, *hidden, 25], [ACT_CODE[act]] * len(hidden) + [NONE], Ws, bs


@functools.lru_cache(maxsize=2)
def real_rows(Q, seed=29):
    """x [Q, 32] (28 valid columns, N(0, 1)), dout [Q, 32] (25 valid), base and target [Q, 25] with the quaternion's w + 2
    (as test_forward_loss_fused_equals_two_kernels keeps them away from zero norm), float32"""
    rng = np.random.default_rng(seed)
    x = np.zeros((Q, 32), np.float32)
    x[:, :28] = rng.standard_normal((Q, 28))
    dout = np.zeros((Q, 32), np.float32)
    dout[:, :25] = rng.standard_normal((Q, 25))
    base = rng.standard_normal((Q, 25)).astype(np.float32)
    base[:, 3] += 2.0
    target = rng.standard_normal((Q, 25)).astype(np.float32)
    target[:, 3] += 2.0
    return x, dout, base, target
