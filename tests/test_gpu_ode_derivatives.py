"""GPU tests (``-m gpu``) of the derivative kernels and of the backward passes built on them.

``kr_ode_jacobian_batch`` and ``kr_ode_vjp_batch`` (csrc/kr_vjp.hip) against the 50-digit derivative of the oracle's
point map (oracle/ode_derivative.py), block by block (tests/ode_derivative_cases.py): five parameter sets - among them
a non-zero ``Bse``, non-diagonal material matrices and drag coefficients of order 1, which no preset has -, both
graphs (``cut`` 0 / 1), fp64 and fp32 arrays, launches of one thread to 750 blocks, every ``need`` mask, a live
handle, the argument checks.  Then ``ODE_parallel``'s backward and the adjoint sweep of ``getResidualEuler`` on the 18
sweep cases of tests/golden/ode_deriv.npz (N = 4, 10, 33; no network, 28 inputs, 53 inputs), in the default mode
against the reference's autograd and with ``exact_sweep_gradient`` against the oracle sweep.

Bounds (ode_derivative_cases.py): an fp64 block is held to 16 x the distance of the reference's fp64 autograd from
the 50-digit derivative in that block (CPU-measured, tests/test_ode_derivative_cpu.py), not below 1e-14; fp32 arrays to
2^-23; the torch wrappers to the bounds test_gpu_configs.py already holds the same quantities to.
Every test prints the figures it measured (``pytest -s``)."""

import numpy as np
import pytest

import ode_derivative_cases as dc
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QS = (1, 5, 6, 13, 14, 257, 4099)   # 47 threads per row: 5 / 6 rows straddle a 256-thread block; 19 per row: 13 / 14 do
SENT = -7.25                        # fills the row after the last one of every output buffer


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ---------------------------------------------------------------------------
# shared, read-only: rows, oracle Jacobians (0.1 s per row and mode), handles
# ---------------------------------------------------------------------------
_J = {}
_H = {}


def case_rows(fp32):
    rows = dc.rows()
    return tuple(a.astype(np.float32).astype(np.float64) for a in rows) if fp32 else rows


def oracle_J(s, cut, fp32_rows=False, fp32_params=False):
    """[4, 25, 47] at the committed rows (``fp32_rows``: at those rows rounded to float32)."""
    key = (s, bool(cut), fp32_rows, fp32_params)
    if key not in _J:
        import ode_derivative as od
        J = od.jacobian_mp_batch(dc.rod_params(s, fp32=fp32_params).derived(), *case_rows(fp32_rows), cut=cut)
        J.setflags(write=False)
        _J[key] = J
    return _J[key]


def kr_params(s):
    import krod_native as kn
    P = dc.rod_params(s)
    return kn.params_from_dict(dict(L=P.L, N=P.N, E=P.E, r=P.r, rho=P.rho, vstar=P.vstar, g=P.g, Bse=P.Bse, Bbt=P.Bbt,
                                    C=P.C, del_t=P.del_t))


def handle(s):
    if s not in _H:
        import krod_native as kn
        _H[s] = kn.Handle(kr_params(s), 0)
    return _H[s]


def cotangents():
    """g[4, 25], one per distinct row, O(1) in every component"""
    return np.random.default_rng(12).uniform(0.5, 1.5, size=(4, 25)) * np.random.default_rng(13).choice([-1.0, 1.0], size=(4, 25))


def device_rows(torch, Q, dtype, fp32_rows=False):
    idx = np.arange(Q) % dc.N_ROWS
    return [torch.tensor(a[idx], dtype=dtype, device=DEV).contiguous() for a in case_rows(fp32_rows)]


def run_jacobian(torch, h, Q, dtype, cut, ins=None, fp32_rows=False):
    """kr_ode_jacobian_batch through the C ABI into a buffer with one row too many: float64 [Q, 25, 19]."""
    import krod_native as kn
    ins = ins if ins is not None else device_rows(torch, Q, dtype, fp32_rows)
    jac = torch.full((Q + 1, 25, 19), SENT, dtype=dtype, device=DEV)
    kn.check(h.lib.kr_ode_jacobian_batch(h._h, Q, *[kn._ptr(a) for a in ins], int(cut), kn._ptr(jac), kn.dtype_code(dtype),
                                         kn._stream()))
    out = jac.cpu().numpy()
    assert np.all(out[Q] == SENT), "the Jacobian kernel wrote past its last row"
    return out[:Q]


def run_vjp(torch, h, Q, dtype, cut, g, need=(True, True, True, True), fp32_rows=False):
    """kr_ode_vjp_batch through the C ABI; g[4, 25] is tiled like the rows.  Outputs not needed are passed as null and
    come back None; the others are float64 [Q, n], each from a buffer with one row too many."""
    import krod_native as kn
    ins = device_rows(torch, Q, dtype, fp32_rows)
    gt = torch.tensor(g[np.arange(Q) % dc.N_ROWS], dtype=dtype, device=DEV)
    g_ys, g_z = gt[:, :19].contiguous(), gt[:, 19:].contiguous()
    bufs = [torch.full((Q + 1, n), SENT, dtype=dtype, device=DEV) if w else None for n, w in zip((19, 19, 6, 3), need)]
    kn.check(h.lib.kr_ode_vjp_batch(h._h, Q, *[kn._ptr(a) for a in ins], kn._ptr(g_ys), kn._ptr(g_z), int(cut),
                                    *[kn._ptr(b) for b in bufs], kn.dtype_code(dtype), kn._stream()))
    outs = []
    for b in bufs:
        if b is None:
            outs.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(o[Q] == SENT), "the VJP kernel wrote past its last row"
        outs.append(o[:Q])
    return outs


def assert_repeats(a, what):
    """rows are tiled with period 4: every repeat is bit-identical to the first occurrence"""
    Q = a.shape[0]
    if Q > dc.N_ROWS:
        assert np.array_equal(a, a[np.arange(Q) % dc.N_ROWS]), f"{what}: a repeated row differs from its first occurrence"


def padded(J19):
    """[R, 25, 19] -> [R, 25, 47] with zeros in the columns the Jacobian kernel does not return"""
    out = np.zeros(J19.shape[:2] + (47,))
    out[:, :, :19] = J19
    return out


def report(what, errs):
    live = {k: v for k, v in errs.items() if v is not None}
    worst = max(live, key=live.get)
    print(f"MEASURED {what}: worst {live[worst]:.2e} at {worst}; " + " ".join(f"{k}={v:.1e}" for k, v in live.items()))


# ---------------------------------------------------------------------------
# the kernels, fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0, 1])
@pytest.mark.parametrize("s", dc.SETS)
def test_jacobian_fp64(torch_cuda, s, cut):
    torch = torch_cuda
    want = oracle_J(s, cut)
    worst = {}
    for Q in QS:
        J = run_jacobian(torch, handle(s), Q, torch.float64, cut)
        assert_repeats(J, f"Q={Q}")
        R = min(Q, dc.N_ROWS)
        errs = dc.assert_blocks(padded(J[:R]), want[:R], dc.gpu_block_bound, in_blocks=dc.Y_IN_BLOCKS,
                                what=f"kr_ode_jacobian_batch set {s} cut {cut} Q {Q}")
        for k, e in errs.items():
            if e is not None and k[1] in dc.Y_IN_BLOCKS:
                worst[k] = max(worst.get(k, 0.0), e)
    report(f"jacobian fp64 {s} cut={cut}", worst)


@pytest.mark.parametrize("cut", [0, 1])
@pytest.mark.parametrize("s", dc.SETS)
def test_vjp_fp64(torch_cuda, s, cut):
    """All four outputs per input block against J_mp^T g: g on one output block at a time (a small block is then not
    drowned by a large one) at Q = 6, and a dense g at every Q."""
    torch = torch_cuda
    want, g = oracle_J(s, cut), cotangents()
    worst = {}

    def note(tag, errs):
        for ib, e in errs.items():
            if e is not None:
                worst[tag, ib] = max(worst.get((tag, ib), 0.0), e)

    for ob, so in dc.OUT_BLOCKS.items():
        g1 = np.zeros_like(g)
        g1[:, so] = g[:, so]
        outs = run_vjp(torch, handle(s), 6, torch.float64, cut, g1)
        for o in outs:
            assert_repeats(o, f"g on {ob}")
        note(ob, dc.assert_vjp([o[:4] for o in outs], want, g1, [ob], dc.gpu_block_bound,
                               what=f"kr_ode_vjp_batch set {s} cut {cut} g on {ob}"))
    for Q in QS:
        outs = run_vjp(torch, handle(s), Q, torch.float64, cut, g)
        for o in outs:
            assert_repeats(o, f"Q={Q}")
        R = min(Q, dc.N_ROWS)
        note("dense", dc.assert_vjp([o[:R] for o in outs], want[:R], g[:R], list(dc.OUT_BLOCKS), dc.gpu_block_bound,
                                    what=f"kr_ode_vjp_batch set {s} cut {cut} dense g Q {Q}"))
    report(f"vjp fp64 {s} cut={cut}", worst)


def test_vjp_agrees_with_the_jacobian_kernel(torch_cuda):
    """The two entry points evaluate one point map: J^T g formed on the host from the Jacobian kernel's output agrees
    with the VJP kernel's to the rounding of two 25-term sums, 2 x 25 x 2^-53 of sum |J| |g|."""
    torch = torch_cuda
    g = cotangents()
    for cut in (0, 1):
        J = run_jacobian(torch, handle("full"), 4, torch.float64, cut)
        vy = run_vjp(torch, handle("full"), 4, torch.float64, cut, g)[0]
        want = np.einsum("roi,ro->ri", J, g)
        scale = np.einsum("roi,ro->ri", np.abs(J), np.abs(g))
        assert np.all(np.abs(vy - want) <= 50 * 2.0 ** -53 * scale)


# ---------------------------------------------------------------------------
# fp32 arrays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [0, 1])
@pytest.mark.parametrize("s", dc.SETS)
def test_fp32_arrays(torch_cuda, s, cut):
    """VjpArgs<float>: the inputs are float32 numbers, the arithmetic is fp64, every output is rounded once - 2^-24 per
    entry, so 2^-24 per block in relative L2, plus the fp64 error (1e-14): bound 2^-23."""
    torch = torch_cuda
    want = oracle_J(s, cut, fp32_rows=True)
    g = cotangents().astype(np.float32).astype(np.float64)
    for Q in (6, 14):
        J = run_jacobian(torch, handle(s), Q, torch.float32, cut, fp32_rows=True)
        assert_repeats(J, f"Q={Q}")
        errs = dc.assert_blocks(padded(J[:4]), want, dc.FP32_BOUND, in_blocks=dc.Y_IN_BLOCKS,
                                what=f"fp32 Jacobian set {s} cut {cut} Q {Q}")
    report(f"jacobian fp32 {s} cut={cut}", {k: e for k, e in errs.items() if k[1] in dc.Y_IN_BLOCKS})
    worst = {}
    for ob, so in list(dc.OUT_BLOCKS.items()) + [("dense", slice(0, 25))]:
        g1 = np.zeros_like(g)
        g1[:, so] = g[:, so]
        outs = run_vjp(torch, handle(s), 6, torch.float32, cut, g1, fp32_rows=True)
        for o in outs:
            assert_repeats(o, f"g on {ob}")
        errs = dc.assert_vjp([o[:4] for o in outs], want, g1, list(dc.OUT_BLOCKS) if ob == "dense" else [ob],
                             dc.FP32_BOUND, what=f"fp32 VJP set {s} cut {cut} g on {ob}")
        worst.update({(ob, ib): e for ib, e in errs.items()})
    report(f"vjp fp32 {s} cut={cut}", worst)


# ---------------------------------------------------------------------------
# need masks, live handle, argument checks
# ---------------------------------------------------------------------------
def test_need_masks(torch_cuda):
    """All 16 combinations of the four optional outputs at Q = 6 (282 threads: two blocks): what is written is
    bit-identical to the call that asks for everything, what is not asked for is not touched (null pointer)."""
    torch = torch_cuda
    g = cotangents()
    for cut in (0, 1):
        full = run_vjp(torch, handle("full"), 6, torch.float64, cut, g)
        for mask in range(16):
            need = tuple(bool(mask >> k & 1) for k in range(4))
            outs = run_vjp(torch, handle("full"), 6, torch.float64, cut, g, need=need)
            for k in range(4):
                if need[k]:
                    assert np.array_equal(outs[k], full[k]), (cut, need, k)
                else:
                    assert outs[k] is None


def test_set_params_on_a_live_handle(torch_cuda):
    """kr_set_params with another del_t and a full Bse on a handle that has already launched: the derivative kernels
    then compute what a fresh handle with those parameters computes, bit for bit."""
    torch = torch_cuda
    import krod_native as kn
    g = cotangents()
    live = kn.Handle(kr_params("None"), 0)
    before = run_jacobian(torch, live, 6, torch.float64, 0)
    live.set_params(kr_params("full"))
    fresh = kn.Handle(kr_params("full"), 0)
    assert kr_params("full").del_t != kr_params("None").del_t and np.all(np.array(kr_params("full").Bse) != 0)
    for cut in (0, 1):
        a, b = run_jacobian(torch, live, 6, torch.float64, cut), run_jacobian(torch, fresh, 6, torch.float64, cut)
        assert np.array_equal(a, b)
        for x, y_ in zip(run_vjp(torch, live, 6, torch.float64, cut, g), run_vjp(torch, fresh, 6, torch.float64, cut, g)):
            assert np.array_equal(x, y_)
    assert not np.array_equal(before, a)
    dc.assert_blocks(padded(b[:4]), oracle_J("full", 1), dc.gpu_block_bound, in_blocks=dc.Y_IN_BLOCKS, what="fresh handle")
    live.close()
    fresh.close()


def test_argument_checks(torch_cuda):
    """Q = 0 is a no-op; Q < 0, an unknown dtype and a null input are KR_E_ARG with a message.  All of them return
    before anything is launched."""
    torch = torch_cuda
    import krod_native as kn
    h = handle("full")
    lib = h.lib
    f64 = torch.float64
    ins = device_rows(torch, 4, f64)
    p = [kn._ptr(a) for a in ins]
    gt = torch.tensor(cotangents(), dtype=f64, device=DEV)
    g_ys, g_z = gt[:, :19].contiguous(), gt[:, 19:].contiguous()
    jac = torch.full((4, 25, 19), SENT, dtype=f64, device=DEV)
    outs = [torch.full((4, n), SENT, dtype=f64, device=DEV) for n in (19, 19, 6, 3)]
    po = [kn._ptr(o) for o in outs]
    st = kn._stream()

    def jcall(Q=4, y=p[0], yh=p[1], zh=p[2], tf=p[3], out=kn._ptr(jac), dtype=kn.KR_F64):
        return lib.kr_ode_jacobian_batch(h._h, Q, y, yh, zh, tf, 0, out, dtype, st)

    def vcall(Q=4, y=p[0], yh=p[1], zh=p[2], tf=p[3], gy=kn._ptr(g_ys), gz=kn._ptr(g_z), dtype=kn.KR_F64):
        return lib.kr_ode_vjp_batch(h._h, Q, y, yh, zh, tf, gy, gz, 0, *po, dtype, st)

    assert jcall(Q=0) == 0 and vcall(Q=0) == 0
    bad = [lambda: jcall(Q=-1), lambda: vcall(Q=-1), lambda: jcall(dtype=7), lambda: vcall(dtype=7),
           lambda: jcall(y=None), lambda: jcall(yh=None), lambda: jcall(zh=None), lambda: jcall(tf=None),
           lambda: jcall(out=None), lambda: vcall(y=None), lambda: vcall(yh=None), lambda: vcall(zh=None),
           lambda: vcall(tf=None), lambda: vcall(gy=None), lambda: vcall(gz=None)]
    for k, call in enumerate(bad):
        assert call() == kn.KR_E_ARG, k
        msg = lib.kr_last_error()
        assert msg and len(msg.decode()) > 3, k
    assert lib.kr_ode_jacobian_batch(None, 4, *p, 0, kn._ptr(jac), kn.KR_F64, st) == kn.KR_E_ARG
    torch.cuda.synchronize()
    assert bool((jac == SENT).all()) and all(bool((o == SENT).all()) for o in outs), "a refused or empty call wrote"


# ---------------------------------------------------------------------------
# backward of ODE_parallel (fp32 torch wrapper)
# ---------------------------------------------------------------------------
def torch_rod(torch, s, N=10, net="off"):
    from cosserat_ode_torch import CosseratRodTorch
    mlp = dc.sweep_mlp(net)
    rob = CosseratRodTorch(DEV, 64, nn_input_history=bool(mlp is not None and mlp.history))
    rob.N = N
    dc.apply_to_torch_rod(rob, s)
    if mlp is not None:
        with torch.no_grad():
            rob.nn_models[0].weight.copy_(torch.tensor(mlp.weights[0]))
            rob.nn_models[0].bias.copy_(torch.tensor(mlp.biases[0]))
            rob.nn_models[2].weight.copy_(torch.tensor(mlp.weights[1]))
            rob.nn_models[2].bias.copy_(torch.tensor(mlp.biases[1]))
    rob.use_nn = mlp is not None
    return rob


@pytest.mark.parametrize("which", ["dys", "z", "only_yhs"])
@pytest.mark.parametrize("s", ["bse_diag", "full"])
def test_ode_parallel_backward(torch_cuda, s, which):
    """Input gradients of ``ODE_parallel`` (physics; ``_OdePhysicsFunction.backward``) against J_mp^T g at 2e-5, the
    bound test_ode_parallel_input_gradients holds them to.  ``dys`` / ``z``: the loss reaches one output only, the
    other cotangent arrives as None.  ``only_yhs``: one input requires a gradient, the others come back without."""
    torch = torch_cuda
    rob = torch_rod(torch, s)
    J = oracle_J(s, 0, fp32_rows=True, fp32_params=True)
    g = cotangents().astype(np.float32).astype(np.float64)
    if which == "dys":
        g[:, 19:] = 0
    elif which == "z":
        g[:, :19] = 0
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    only = which == "only_yhs"
    ins = [t(a).requires_grad_(not only or k == 1) for k, a in enumerate(case_rows(True))]
    dys, z = rob.ODE_parallel(*ins)
    L = 0
    if which != "z":
        L = L + (dys * t(g[:, :19])).sum()
    if which != "dys":
        L = L + (z * t(g[:, 19:])).sum()
    L.backward()
    want = np.einsum("roi,ro->ri", J, g)
    for k, (name, off, n) in enumerate((("y", 0, 19), ("yh", 19, 19), ("zh", 38, 6), ("tf", 44, 3))):
        if only and k != 1:
            assert ins[k].grad is None
            continue
        got, w = ins[k].grad.cpu().numpy(), want[:, off:off + n]
        if not np.any(w):   # z does not see yh or the tendon force
            assert not np.any(got), name
            continue
        e = rel_l2(got, w)
        print(f"MEASURED ODE_parallel backward {s} {which} d/d{name}: {e:.2e}")
        assert e < 2e-5, (name, e)


# ---------------------------------------------------------------------------
# adjoint sweep of getResidualEuler (fp32 torch wrapper)
# ---------------------------------------------------------------------------
def run_sweep(torch, rob, g, N, s, exact):
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)
    y, z, yp, zp = (t(g[f"sw_N{N}_{k}"]) for k in ("y", "z", "yp", "zp"))
    rob.exact_sweep_gradient = exact
    rob.y, rob.z = y.clone(), z.clone()
    rob.tendon_tensions = t(g[f"sw_N{N}_tens"])
    rob.residualArgs["yh"] = rob.c1 * y + rob.c2 * yp
    rob.residualArgs["zh"] = rob.c1 * z + rob.c2 * zp
    for prm in rob.nn_models.parameters():
        prm.grad = None
    G = t(g[f"sw_N{N}_G"]).requires_grad_(True)
    total, full = rob.getResidualEuler(G)
    assert full.shape == (25, N)
    L = total + (full * t(g[f"sw_N{N}_Wgt"])).sum()
    L.backward()
    return float(L.detach()), G.grad.cpu().numpy(), [p.grad.cpu().numpy() if p.grad is not None else None
                                                     for p in rob.nn_models.parameters()]


@pytest.mark.parametrize("N,s,net", dc.SWEEP_CASES)
def test_sweep_backward_default_mode(torch_cuda, N, s, net):
    """The adjoint sweep as ``getResidualEuler`` differentiates by default (the reference's cut graph) against the
    reference's autograd: L at 2e-5, dL/dG at 1e-4, dL/d(parameters) at 1e-3 - the bounds of
    test_torch_full_sweep_autograd.  Q = N - 1 is 3, 9 and 32; ``hist64`` runs the 53-input branch (z0 = 38)."""
    torch = torch_cuda
    g = load_golden("ode_deriv")
    tag = dc.sweep_tag(N, s, net)
    L, dG, dparams = run_sweep(torch, torch_rod(torch, s, N, net), g, N, s, exact=False)
    eL, eG = abs(L - float(g[f"{tag}_L"])) / abs(float(g[f"{tag}_L"])), rel_l2(dG, g[f"{tag}_dG"])
    eP = [rel_l2(p, g[f"{tag}_dparam{k}"]) for k, p in enumerate(dparams)] if net != "off" else []
    print(f"MEASURED sweep default {tag}: L {eL:.2e} dG {eG:.2e} dparam " + " ".join(f"{e:.2e}" for e in eP))
    assert eL < 2e-5
    assert eG < 1e-4
    if net == "off":
        assert all(p is None for p in dparams)
    else:
        assert len(eP) == 4 and all(e < 1e-3 for e in eP), eP


@pytest.mark.parametrize("N,s,net", dc.SWEEP_CASES)
def test_sweep_backward_exact_mode(torch_cuda, N, s, net):
    """``exact_sweep_gradient = True``: the gradient of the function itself, against central differences of the fp64
    oracle sweep - dL/dG at 1e-4 (the default mode's bound for dG; the oracle's two steps agree to 1e-8), and 20
    entries of every parameter tensor at 1e-3 (its bound for the parameters; ``oracle_sweep_dparams``)."""
    torch = torch_cuda
    g = load_golden("ode_deriv")
    tag = dc.sweep_tag(N, s, net)
    want, _, _ = dc.oracle_sweep_dG(g, N, s, net)
    L, dG, dparams = run_sweep(torch, torch_rod(torch, s, N, net), g, N, s, exact=True)
    eG = rel_l2(dG, want)
    eP = []
    if net != "off":
        for k, idx, vals in dc.oracle_sweep_dparams(g, N, s, net):
            eP.append(rel_l2(dparams[k].reshape(-1)[idx], vals))
    print(f"MEASURED sweep exact {tag}: dG {eG:.2e} dparam " + " ".join(f"{e:.2e}" for e in eP))
    assert eG < 1e-4
    assert all(e < 1e-3 for e in eP), eP
