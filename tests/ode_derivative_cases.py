"""Shared by tests/test_ode_derivative_cpu.py and tests/test_gpu_ode_derivatives.py: the parameter sets, rows, block
table and comparison of the derivative tests, and the sweep cases of tests/golden/ode_deriv.npz (written by
``gen_ode_deriv`` of tests/golden/make_golden.py from the unmodified reference).

The reference for every derivative is ``oracle/ode_derivative.py``: central differences of the oracle's point map at
50 digits.  A Jacobian is never judged by one norm - its entries span nine orders of magnitude - but block by block:
8 output blocks x 12 input blocks, each either exactly zero in the oracle (then exactly zero in what is tested) or
compared by its own relative L2 error, row by row."""
import numpy as np

# ---------------------------------------------------------------------------
# block table: rows of the Jacobian [y_s(19), z(6)], columns [y(19), yh(19), zh(6), tf(3)]
# ---------------------------------------------------------------------------
OUT_BLOCKS = {"p_s": slice(0, 3), "h_s": slice(3, 7), "n_s": slice(7, 10), "m_s": slice(10, 13),
              "q_s": slice(13, 16), "w_s": slice(16, 19), "v": slice(19, 22), "u": slice(22, 25)}
IN_BLOCKS = {"p": slice(0, 3), "h": slice(3, 7), "n": slice(7, 10), "m": slice(10, 13), "q": slice(13, 16),
             "w": slice(16, 19), "yh_0_13": slice(19, 32), "yh_q": slice(32, 35), "yh_w": slice(35, 38),
             "vh": slice(38, 41), "uh": slice(41, 44), "tf": slice(44, 47)}
Y_IN_BLOCKS = ("p", "h", "n", "m", "q", "w")               # the 19 columns kr_ode_jacobian_batch returns
# the four outputs of kr_ode_vjp_batch and the input blocks each holds (offset of the output's first column)
VJP_OUTPUTS = (("y", 0, ("p", "h", "n", "m", "q", "w")), ("yh", 19, ("yh_0_13", "yh_q", "yh_w")),
               ("zh", 38, ("vh", "uh")), ("tf", 44, ("tf",)))

# ---------------------------------------------------------------------------
# parameter sets
# ---------------------------------------------------------------------------
SETS = ("None", "noair", "dampstiff", "bse_diag", "full")
SWEEP_SETS = ("None", "full")
# "bse_diag": the None preset (Kse = diag(33592, 33592, 87340), c0 = 30) with c0 Bse = 0.11, 0.45, 0.86 of Kse's diagonal
BSE_DIAG = np.diag([120.0, 500.0, 2500.0])
# "full": nothing diagonal, nothing small.  c0 = 300 (del_t = 0.005): c0 Bse = about 1.9 Kse on the diagonal
FULL = dict(
    Bse=np.array([[210.0, 35.0, -20.0], [-50.0, 190.0, 40.0], [25.0, -60.0, 540.0]]),
    Bbt=np.array([[0.03, 0.008, -0.004], [-0.011, 0.025, 0.006], [0.005, -0.009, 0.04]]),
    C=np.array([0.3, 0.7, 1.1]), vstar=np.array([0.1, -0.2, 1.0]), del_t=0.005)
PARAM_FIELDS = ("E", "del_t", "Bse", "Bbt", "C", "vstar")   # what the sets differ in; stored per set in the fixture


def rod_params(name, N=10, fp32=False):
    """Oracle parameters of a set.  ``fp32``: the tensor-valued parameters rounded to float32, which is what a
    ``CosseratRodTorch`` holds (its attributes are float32 tensors) and hands to the library."""
    import cosserat_oracle as orc
    P = orc.setup_params(name if name in ("noair", "dampstiff") else None, N)
    if name == "bse_diag":
        P.Bse = BSE_DIAG.copy()
    elif name == "full":
        for k, v in FULL.items():
            setattr(P, k, np.array(v) if isinstance(v, np.ndarray) else v)
    elif name not in ("None", "noair", "dampstiff"):
        raise ValueError(name)
    if fp32:
        for k in ("Bse", "Bbt", "C", "vstar", "g"):
            setattr(P, k, np.asarray(getattr(P, k), np.float32).astype(np.float64))
    return P


def apply_to_torch_rod(rob, name):
    """The same set on a ``CosseratRodTorch`` (ours or the reference's): ``setup_robot`` and attribute assignment."""
    import torch
    from knode import setup_robot
    setup_robot(rob, name if name in ("noair", "dampstiff") else None)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.get_default_dtype(), device=rob.device)
    if name == "bse_diag":
        rob.Bse = t(BSE_DIAG)
    elif name == "full":
        rob.Bse, rob.Bbt, rob.C, rob.vstar = t(FULL["Bse"]), t(FULL["Bbt"]), t(FULL["C"]), t(FULL["vstar"])
        rob.del_t = FULL["del_t"]
    rob.compute_intermediate_terms()
    return rob


# ---------------------------------------------------------------------------
# rows: 4 per set (the same 4 for every set)
# ---------------------------------------------------------------------------
KAT_ROWS = (3, 29)   # two physical rows of ode_kat.npz (states of a reference run, jittered, |h| in 0.7 .. 1.4)
# two synthetic rows, every component O(1); |h| = 0.745 and 1.368; q covers > 0, < 0 and exactly 0.0
SYN_Y = np.array([
    [0.3, -0.7, 1.1, 0.55, -0.3, 0.35, 0.2, 0.9, -1.2, 0.6, -0.8, 0.5, 1.3, 0.8, -1.3, 0.0, 0.7, -0.4, 1.1],
    [-1.2, 0.4, 0.6, -0.5, 0.9, 0.3, -0.85, -0.6, 0.75, 1.4, 1.1, -0.9, -0.45, 0.0, 0.6, -0.9, -1.2, 0.8, 0.5]])
SYN_YH = np.array([
    [0.5, -1.0, 0.8, 1.2, -0.6, 0.4, 0.9, -0.7, 1.3, 0.6, -1.1, 0.45, 0.75, -0.95, 1.15, 0.65, 0.85, -1.25, 0.55],
    [-0.8, 0.7, 1.4, -0.5, 1.0, -1.3, 0.6, 0.9, -0.4, 1.2, 0.55, -0.65, 1.05, 0.95, -0.75, 1.35, -1.15, 0.45, 0.7]])
SYN_ZH = np.array([[0.7, -1.1, 0.9, 1.3, -0.5, 0.6], [-0.9, 0.8, 1.2, -0.6, 1.1, -1.4]])
SYN_TF = np.array([[0.9, -0.6, 1.2], [-1.1, 0.7, 0.5]])
N_ROWS = 4


def rows():
    """(y[4, 19], yh[4, 19], zh[4, 6], tf[4, 3]) float64."""
    import os
    import cosserat_oracle as orc
    k = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ode_kat.npz"))
    i = list(KAT_ROWS)
    tf = k["tensions"][i] @ orc.RodParams().tendon_dirs
    return (np.concatenate([k["y"][i], SYN_Y]), np.concatenate([k["yh"][i], SYN_YH]),
            np.concatenate([k["zh"][i], SYN_ZH]), np.concatenate([tf, SYN_TF]))


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def block_errors(got, want):
    """{(out block, in block): None where the oracle block ``want`` is exactly zero (and ``got`` is asserted exactly zero
    there), else the largest relative L2 error of that block over the rows}.  got, want: ``[Q, 25, 47]``."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.shape[1:] == (25, 47), (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    out = {}
    for ob, so in OUT_BLOCKS.items():
        for ib, si in IN_BLOCKS.items():
            w, g = want[:, so, si], got[:, so, si]
            if not np.any(w):
                assert not np.any(g), f"block d({ob})/d({ib}) is exactly zero in the oracle, not in what is tested"
                out[ob, ib] = None
                continue
            nw = np.linalg.norm(w, axis=(1, 2))
            assert np.all(nw > 0), f"block d({ob})/d({ib}) is zero in some rows only"
            out[ob, ib] = float(np.max(np.linalg.norm(g - w, axis=(1, 2)) / nw))
    return out


def assert_blocks(got, want, bound, in_blocks=None, what=""):
    """Per-block comparison of Jacobians ``[Q, 25, 47]``; ``bound`` is a number or a function of (out block, in block).
    ``in_blocks`` restricts the columns looked at (the others of ``got`` may hold anything).  Returns the errors."""
    if in_blocks is not None:
        got = np.array(got, dtype=np.float64)
        for ib, si in IN_BLOCKS.items():
            if ib not in in_blocks:
                got[:, :, si] = want[:, :, si]
    errs = block_errors(got, want)
    bad = []
    for (ob, ib), e in errs.items():
        if e is None or (in_blocks is not None and ib not in in_blocks):
            continue
        b = bound(ob, ib) if callable(bound) else bound
        if not e <= b:
            bad.append(f"d({ob})/d({ib}): {e:.3e} > {b:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return errs


def vjp_errors(outs, J, g, support):
    """J^T g as kr_ode_vjp_batch returns it - ``outs`` = (o_y[R, 19], o_yh[R, 19], o_zh[R, 6], o_tf[R, 3]) - against the
    oracle Jacobians ``J[R, 25, 47]`` and cotangents ``g[R, 25]`` that are non-zero on the output blocks ``support``
    only.  Per input block: exactly zero where every oracle block (support x input block) is, else

        max over rows of  |got - J^T g| / sum_ob |J[ob, ib]|_F |g[ob]|,

    the scale against which both a relative error of the block J[ob, ib] and the rounding of the sum over its 3 or 4
    terms are bounded (|dJ^T g| <= |dJ|_F |g|); the norm of J^T g itself can be arbitrarily smaller.
    Returns {in block: (error or None, [out blocks of the support that are non-zero there])}."""
    J, g = np.asarray(J, np.float64), np.asarray(g, np.float64)
    res = {}
    for (name, off, ibs), got_all in zip(VJP_OUTPUTS, outs):
        got_all = np.asarray(got_all, np.float64)
        assert np.all(np.isfinite(got_all))
        for ib in ibs:
            si = IN_BLOCKS[ib]
            got = got_all[:, si.start - off:si.stop - off]
            want = np.zeros_like(got)
            scale = np.zeros(got.shape[0])
            live = []
            for ob in support:
                so = OUT_BLOCKS[ob]
                if np.any(J[:, so, si]):
                    live.append(ob)
                    want += np.einsum("roi,ro->ri", J[:, so, si], g[:, so])
                    scale += np.linalg.norm(J[:, so, si], axis=(1, 2)) * np.linalg.norm(g[:, so], axis=1)
            if not live:
                assert not np.any(got), f"d({support})/d({ib}) is exactly zero in the oracle, the VJP is not"
                res[ib] = (None, live)
                continue
            assert np.all(scale > 0)
            res[ib] = (float(np.max(np.linalg.norm(got - want, axis=1) / scale)), live)
    return res


def assert_vjp(outs, J, g, support, bound, what=""):
    """``bound``: a number or a function of (out block, in block); a sum over several output blocks is held to the
    largest of their bounds.  Returns the errors per input block."""
    res = vjp_errors(outs, J, g, support)
    bad = []
    for ib, (e, live) in res.items():
        if e is None:
            continue
        b = max(bound(ob, ib) for ob in live) if callable(bound) else bound
        if not e <= b:
            bad.append(f"g on {','.join(live)} -> d/d({ib}): {e:.3e} > {b:.3e}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return {ib: e for ib, (e, _) in res.items()}


def zero_pattern(J):
    return {(ob, ib): not np.any(np.asarray(J)[:, so, si]) for ob, so in OUT_BLOCKS.items() for ib, si in IN_BLOCKS.items()}


# ---------------------------------------------------------------------------
# how far an fp64 evaluation of the derivative is from the 50-digit one
# ---------------------------------------------------------------------------
# Largest per-block, per-row relative L2 distance of the REFERENCE's fp64 autograd Jacobian of ODE_parallel (uncut)
# from ``jacobian_mp`` over the 20 committed rows (5 sets x 4 rows), measured on the CPU by
# tests/test_ode_derivative_cpu.py::test_reference_uncut_jacobian_vs_oracle (which fails if a block exceeds its entry)
# and rounded up to two digits.  Blocks not listed are exactly zero in every set.
REF_UNCUT_DIST = {
    ("p_s", "h"): 3.7e-16, ("p_s", "n"): 2.5e-16, ("h_s", "h"): 5.1e-16, ("h_s", "m"): 2.2e-16,
    ("h_s", "uh"): 1.5e-16, ("n_s", "h"): 3.3e-16, ("n_s", "q"): 1.5e-16, ("n_s", "w"): 1.7e-16,
    ("n_s", "yh_q"): 1.2e-16, ("n_s", "tf"): 0.0e+00, ("m_s", "h"): 4.0e-16, ("m_s", "n"): 2.3e-16,
    ("m_s", "w"): 1.8e-16, ("m_s", "yh_w"): 1.4e-16, ("q_s", "h"): 2.6e-16, ("q_s", "n"): 2.3e-16,
    ("q_s", "m"): 2.0e-16, ("q_s", "q"): 2.2e-16, ("q_s", "w"): 2.3e-16, ("q_s", "vh"): 3.6e-16,
    ("q_s", "uh"): 2.0e-16, ("w_s", "h"): 3.3e-16, ("w_s", "m"): 1.7e-16, ("w_s", "w"): 2.2e-16,
    ("w_s", "uh"): 6.7e-15, ("v", "h"): 2.3e-16, ("v", "n"): 2.1e-16, ("u", "h"): 2.4e-16,
    ("u", "m"): 2.1e-16, ("u", "uh"): 1.2e-16, ("p_s", "vh"): 1.7e-16, ("m_s", "vh"): 3.0e-16,
    ("v", "vh"): 1.6e-17,
}
REF_UNCUT_WORST = max(REF_UNCUT_DIST.values())
# The same for the reference's autograd through the serial ODE (cut): its R passes through ``.float()``
# (cosserat_ode_torch.py:161), so this is the reference's fp32 rounding, not the oracle's error.
REF_CUT_WORST = 2.1e-7   # measured 2.06e-7, block d(q_s)/d(h)
CPU_MARGIN = 16    # bound of the CPU tests = CPU_MARGIN x the worst measured block; the margin is for rows not looked at
GPU_MARGIN = 16    # bound of a kernel's block = GPU_MARGIN x that block's distance above, floored; see gpu_block_bound
GPU_FLOOR = 1e-14


def gpu_block_bound(ob, ib):
    """fp64 kernels: 16 x the distance of another fp64 evaluation of the same derivative (the reference's autograd) from
    the 50-digit one in this block, not below 1e-14; the margin is for the kernel's different association and fma
    contraction.  Blocks that exist only in the cut graph's pattern have an uncut twin: the same (out, in) pair."""
    return max(GPU_MARGIN * REF_UNCUT_DIST.get((ob, ib), 0.0), GPU_FLOOR)


FP32_BOUND = 2.0 ** -23   # fp32 arrays: the kernel computes in fp64 and rounds every entry once (2^-24 each) + the fp64 error


# ---------------------------------------------------------------------------
# sweep cases of the fixture: getResidualEuler, L = total + sum(full * Wgt)
# ---------------------------------------------------------------------------
SWEEP_N = (4, 10, 33)
SWEEP_NETS = ("off", "elu64", "hist64")     # no network, 28 -> 64 -> 25, 53 -> 64 -> 25 (history inputs)
NET_SIZES = {"elu64": ([28, 64, 25], False), "hist64": ([53, 64, 25], True)}
NET_SEED = {"elu64": 41, "hist64": 42}
SWEEP_CASES = [(N, s, net) for N in SWEEP_N for s in SWEEP_SETS for net in SWEEP_NETS]


def sweep_tag(N, s, net):
    return f"sw_N{N}_{s}_{net}"


def sweep_mlp(net):
    """The network of a sweep case (weights x 3 like gen_tres_grad, so that the correction matters)."""
    import cosserat_oracle as orc
    if net == "off":
        return None
    sizes, hist = NET_SIZES[net]
    mlp = orc.make_mlp(sizes, "elu", seed=NET_SEED[net], history=hist)
    mlp.weights = [w * 3 for w in mlp.weights]
    return mlp


def sweep_inputs(g, N, s, fp32=True):
    """(D, G, y, z, yh, zh, tens, Wgt) of a case.  ``fp32``: every input rounded the way the torch twins hold it."""
    P = rod_params(s, N, fp32=fp32)
    D = P.derived()
    r = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if fp32 else (lambda a: np.asarray(a, np.float64))
    y, z, yp, zp = (r(g[f"sw_N{N}_{k}"]) for k in ("y", "z", "yp", "zp"))
    yh, zh = r(D.c1 * y + D.c2 * yp), r(D.c1 * z + D.c2 * zp)
    return D, r(g[f"sw_N{N}_G"]), y, z, yh, zh, r(g[f"sw_N{N}_tens"]), r(g[f"sw_N{N}_Wgt"])


def oracle_sweep_loss(D, G, y, z, yh, zh, tens, Wgt, mlp=None):
    """L = total_residual + sum(full_rod * Wgt) of cosserat_ode_torch.py:325-367 from the fp64 oracle sweep; column 0
    of full_rod is [y_0; z[:, 0] of the caller], column j + 1 is [y_{j+1}; z_j]."""
    import cosserat_oracle as orc
    yy, zz = y.copy(), z.copy()
    res = orc.residual_euler(D, G, yy, zz, yh, zh, tens, mlp)
    N = D.N
    full = np.concatenate([np.concatenate([yy[:, :1], z[:, :1]], axis=0),
                           np.concatenate([yy[:, 1:], zz[:, :N - 1]], axis=0)], axis=1)
    return float(np.sum(res ** 2) + np.sum(full * Wgt))


def central_gradient(f, x, step):
    """Central differences of a scalar function of a vector; the step is relative to max(|x_i|, 1)."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    for i in range(x.size):
        e = step * max(abs(x.flat[i]), 1.0)
        xp, xm = x.copy(), x.copy()
        xp.flat[i] += e
        xm.flat[i] -= e
        out.flat[i] = (f(xp) - f(xm)) / (2 * e)
    return out


FD_STEPS = (2e-5, 5e-6)   # central differences in G, relative to max(|G_i|, 1): truncation ~ step^2, rounding ~ 1e-16 |L| / step
W_STEP = 1e-6             # central differences in a weight, absolute step; see oracle_sweep_dparams
_sweep_cache = {}


def oracle_sweep_dG(g, N, s, net):
    """(dL/dG of the fp64 oracle sweep at the finer step, relative L2 distance between the two steps, L), once per case."""
    key = (N, s, net)
    if key not in _sweep_cache:
        D, G, y, z, yh, zh, tens, Wgt = sweep_inputs(g, N, s)
        mlp = sweep_mlp(net)
        f = lambda G_: oracle_sweep_loss(D, G_, y, z, yh, zh, tens, Wgt, mlp)
        a, b = (central_gradient(f, G, st) for st in FD_STEPS)
        b.setflags(write=False)
        _sweep_cache[key] = (b, float(np.linalg.norm(a - b) / np.linalg.norm(b)), f(G))
    return _sweep_cache[key]


def oracle_sweep_dparams(g, N, s, net, n_samples=20, step=W_STEP):
    """Central differences of the oracle sweep in ``n_samples`` entries of every parameter tensor of the network:
    [(parameter index as nn.Module.parameters() orders them, flat indices, gradient entries), ...].  The entries are the
    ones with the largest gradient in the fixture (the reference's, of the cut graph): most entries of a layer's gradient
    are orders of magnitude below its largest, and a difference quotient of L has an absolute floor of about
    1e-16 |L| / step = 5e-7 (|L| up to 5e3).  The step is small because the inputs of the history network reach 1e3
    (yh = c1 y + c2 y_prev): step x input moves a pre-activation by 1e-3, which keeps the truncation near 1e-7."""
    D, G, y, z, yh, zh, tens, Wgt = sweep_inputs(g, N, s)
    mlp = sweep_mlp(net)
    mlp.weights = [np.asarray(w, np.float64) for w in mlp.weights]
    mlp.biases = [np.asarray(b, np.float64) for b in mlp.biases]
    tag = sweep_tag(N, s, net)
    out = []
    for k, arr in enumerate([a for pair in zip(mlp.weights, mlp.biases) for a in pair]):
        ref = np.abs(g[f"{tag}_dparam{k}"]).reshape(-1)
        idx = np.sort(np.argsort(-ref, kind="stable")[:min(n_samples, arr.size)])
        vals = []
        for i in idx:
            keep = arr.flat[i]
            arr.flat[i] = keep + step
            lp = oracle_sweep_loss(D, G, y, z, yh, zh, tens, Wgt, mlp)
            arr.flat[i] = keep - step
            lm = oracle_sweep_loss(D, G, y, z, yh, zh, tens, Wgt, mlp)
            arr.flat[i] = keep
            vals.append((lp - lm) / (2 * step))
        out.append((k, idx, np.array(vals)))
    return out
