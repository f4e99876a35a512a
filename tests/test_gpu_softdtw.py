"""Soft-DTW on the MI355X (kr_softdtw_batch, Handle.softdtw, krod_grad.softdtw_loss) against the 50-digit fixture
(tests/golden/softdtw.npz) within the two derived bounds of tests/softdtw_cases.py - the bounds the host statement
``krod_eval.softdtw_grad`` meets in tests/test_softdtw_cpu.py, which also shows that five mistakes a kernel could make miss
them.  What is a property of the layout and of the order of operations - strided output, shared reference, position in the
batch, repeated calls, value only - is compared bit for bit.  Every figure is printed before it is asserted.

Measured on the MI355X, as this file prints it (LABBOOK.md holds the same figures): max over the 72 fixture cases, fp64,
value error / tolR 8.8e-3, gradient error / tolG 4.3e-4 (the host statement: 8.8e-3 - the same case, the rounding of the cost -
and 6.3e-4); fp32 inputs against the host statement on the upcast samples: value error / tolR at most 3.3e-3, every gradient
entry the host's entry rounded to fp32; 1024 x 1024 at gamma 1e-9: every gradient entry an integer exactly; end to end
(N = 10, T = 5, B = 2): <ctl.grad, d> against the central difference of the device's own forward, error / tolerance 3.5e-2."""
import ctypes as C

import numpy as np
import pytest

import softdtw_cases as sc
from gpu_helpers import make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def robot(torch_cuda):
    return make_robot(None, 10)


@pytest.fixture(scope="module")
def h(robot):
    return robot._native()


def dev(torch, x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype or torch.float64).contiguous()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint64 if t.element_size() == 8 else np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))


def walks(seed, B, Ta, Tb):
    """B pairs of random walks of step 2e-3 around 0.1, the scale of tip paths"""
    rng = np.random.default_rng(seed)
    a = 0.1 + np.cumsum(2e-3 * rng.standard_normal((B, Ta, 3)), axis=1)
    b = 0.1 + np.cumsum(2e-3 * rng.standard_normal((B, Tb, 3)), axis=1)
    return a, b


def batch_around(c, B=3, at=1):
    """B rods, rod `at` the fixture case and the others its sequences reversed in time or shifted: the case is not rod 0"""
    a = np.stack([c["a"] if r == at else (c["a"][::-1] if r % 2 == 0 else c["a"] + 1e-3) for r in range(B)])
    b = np.stack([c["b"] if r == at else (c["b"] + 2e-3 if r % 2 == 0 else c["b"][::-1]) for r in range(B)])
    return a, b


# ---------------------------------------------------------------------------
# 1. value and gradient against the fixture, every case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_fixture_case_within_the_bounds(torch_cuda, h, name):
    torch = torch_cuda
    c = sc.fixture()[name]
    a, b = batch_around(c)
    value, g = h.softdtw(dev(torch, a), dev(torch, b), c["gamma"], cost=c["cost"], grad=True)
    assert g.dtype == torch.float64 and tuple(g.shape) == a.shape and tuple(value.shape) == (3,)
    rv, rg = sc.ratios(c, float(value[1]), g[1].cpu().numpy())
    print(f"{name}: value error / tolR = {rv:.3g}, gradient error / tolG = {rg:.3g}")
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)
    assert torch.isfinite(value).all() and torch.isfinite(g).all()


@pytest.mark.parametrize("cost", ["l1", "sq"])
def test_one_by_one_is_exact(torch_cuda, h, cost):
    torch = torch_cuda
    for gamma in (1e-6, 1e-3, 1e-1):
        c = sc.fixture()[f"1x1_c{0 if cost == 'l1' else 1}_g{gamma:g}"]
        a, b = batch_around(c, B=4, at=2)
        d = a - b
        want = (np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2]) if cost == "l1" else \
            (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        value, g = h.softdtw(dev(torch, a), dev(torch, b), gamma, cost=cost, grad=True)
        assert np.array_equal(value.cpu().numpy().view(np.uint64), want[:, 0].view(np.uint64))
        assert np.array_equal(g.cpu().numpy(), np.sign(d) if cost == "l1" else 2.0 * d)


@pytest.mark.parametrize("Ta,Tb", [(5, 4), (64, 65), (101, 101), (130, 67)])
def test_fp32_inputs_against_the_host_statement(torch_cuda, h, Ta, Tb):
    """The arithmetic is fp64 on the upcast samples; the gradient leaves in the inputs' type, so the bound is taken through
    that (monotone) rounding: fl32(host - tolG) <= g <= fl32(host + tolG)."""
    import krod_eval as ke
    torch = torch_cuda
    B = 3
    a64, b64 = walks(100 * Ta + Tb, B, Ta, Tb)
    ad, bd = dev(torch, a64, torch.float32), dev(torch, b64, torch.float32)
    a, b = ad.cpu().numpy().astype(np.float64), bd.cpu().numpy().astype(np.float64)
    worst = [0.0, 0]
    for cost in ("l1", "sq"):
        for gamma in (1e-6, 1e-3, 1e-1):
            value, g = h.softdtw(ad, bd, gamma, cost=cost, grad=True)
            assert g.dtype == torch.float32 and value.dtype == torch.float64
            value, g = value.cpu().numpy(), g.cpu().numpy()
            for r in range(B):
                d, R, E = ke._softdtw_tables(a[r], b[r], gamma, cost)
                hv, hg = ke.softdtw_grad(a[r], b[r], gamma, cost)
                A = (E[1:-1, 1:-1, None] * np.abs(np.sign(d) if cost == "l1" else 2.0 * d)).sum(1)
                Rmax = float(np.abs(R[1:-1, 1:-1]).max())
                tr, tg = sc.tol_R(Ta, Tb, gamma, Rmax), sc.tol_G(Ta, Tb, gamma, Rmax, A)
                worst[0] = max(worst[0], abs(value[r] - hv) / tr)
                assert abs(value[r] - hv) <= tr, (cost, gamma, r)
                lo, hi = (hg - tg).astype(np.float32), (hg + tg).astype(np.float32)
                assert ((lo <= g[r]) & (g[r] <= hi)).all(), (cost, gamma, r)
                worst[1] += int(np.count_nonzero(g[r] != hg.astype(np.float32)))
    print(f"fp32 {Ta}x{Tb}: value error / tolR = {worst[0]:.3g}; gradient entries that are not the rounded host entry: {worst[1]}")


# ---------------------------------------------------------------------------
# 2. the hard DTW as the limit
# ---------------------------------------------------------------------------
def _sandwich(torch, h, a, b, gamma):
    ad, bd = dev(torch, a), dev(torch, b)
    value, g = h.softdtw(ad, bd, gamma, grad=True)
    dtw = h.dtw(ad, bd)
    Ta, Tb = a.shape[1], b.shape[1]
    n = Ta + Tb - 1
    value, dtw = value.cpu().numpy(), dtw.cpu().numpy()
    for r in range(len(a)):
        tr = sc.tol_R(Ta, Tb, gamma, dtw[r])  # (the DTW itself in place of max |R|, which is not smaller: not a looser bound)
        print(f"{Ta}x{Tb} rod {r}: dtw {dtw[r]:.17g} softdtw {value[r]:.17g} tolR {tr:.3g}")
        assert dtw[r] - gamma * np.log(3.0) * n - tr <= value[r] <= dtw[r] + tr
    return g


def test_sandwich_against_the_device_dtw(torch_cuda, h):
    """gamma = 1e-9: dtw - n gamma ln 3 - tolR <= value <= dtw + tolR against kr_dtw_batch"""
    for seed, (Ta, Tb) in enumerate([(33, 37), (101, 101), (130, 67)]):
        a, b = walks(500 + seed, 4, Ta, Tb)
        _sandwich(torch_cuda, h, a, b, 1e-9)


def test_max_len_is_served_and_one_more_is_refused(torch_cuda, h):
    import krod_native as kn
    torch = torch_cuda
    L = kn.KR_SOFTDTW_MAX_LEN
    a, b = walks(77, 1, L, L)
    g = _sandwich(torch, h, a, b, 1e-9).cpu().numpy()
    off = np.abs(g - np.rint(g)).max()
    print(f"{L}x{L}: largest distance of a gradient entry from an integer {off:.3g}")
    assert off <= 1e-6  # (a hard table: E is 1 on the one warp path and 0 off it, the L1 derivative is a sign)
    long = dev(torch, np.zeros((1, L + 1, 3)))
    short = dev(torch, a[:, :8])
    for x, y in ((long, short), (short, long)):
        with pytest.raises(kn.KrError) as e:
            h.softdtw(x, y, 1e-2)
        assert e.value.code == kn.KR_E_UNSUPPORTED


# ---------------------------------------------------------------------------
# 3. layout and order: bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Ta,Tb", [(5, 7), (70, 101)])
def test_one_launch_seeds_the_cotangent_history(torch_cuda, h, Ta, Tb):
    """g_out = g[1:, :, N - 1, 12:15].permute(1, 0, 2) of a zeroed [T + 1, B, N, KR_SLOTS]: the contiguous call's gradient
    bit for bit, every other element still zero; the same from a tip path read in place out of a state history"""
    import krod_native as kn
    torch = torch_cuda
    B, N, T = 4, h.N, Ta
    a, b = walks(9, B, Ta, Tb)
    ad, bd = dev(torch, a), dev(torch, b)
    for dtype in (torch.float64, torch.float32):
        ad_t, bd_t = ad.to(dtype), bd.to(dtype)
        v0, g0 = h.softdtw(ad_t, bd_t, 1e-2, grad=True)
        states = torch.zeros((T + 1, B, N, kn.KR_SLOTS), dtype=dtype, device=DEV)
        states[1:, :, N - 1, 12:15] = ad_t.permute(1, 0, 2)
        g = torch.zeros_like(states)
        view = g[1:, :, N - 1, 12:15].permute(1, 0, 2)
        v1, g1 = h.softdtw(states[1:, :, N - 1, 12:15].permute(1, 0, 2), bd_t, 1e-2, g_out=view)
        assert g1.data_ptr() == view.data_ptr()
        assert same_bits(v1, v0) and same_bits(view.contiguous(), g0)
        assert g0.abs().sum() > 0
        mask = torch.ones_like(g, dtype=torch.bool)
        mask[1:, :, N - 1, 12:15] = False
        assert torch.count_nonzero(g[mask]) == 0


def test_shared_reference_equals_the_expanded_one(torch_cuda, h):
    torch = torch_cuda
    a, b = walks(11, 5, 70, 66)
    ad, b1 = dev(torch, a), dev(torch, b[0])
    v0, g0 = h.softdtw(ad, b1, 1e-2, cost="sq", grad=True)
    v1, g1 = h.softdtw(ad, b1.unsqueeze(0).repeat(5, 1, 1), 1e-2, cost="sq", grad=True)
    assert same_bits(v0, v1) and same_bits(g0, g1)


@pytest.mark.parametrize("Ta,Tb", [(40, 70), (101, 101)])
def test_rod_of_a_batch_equals_its_own_call_and_calls_repeat(torch_cuda, h, Ta, Tb):
    torch = torch_cuda
    a, b = walks(13, 5, Ta, Tb)
    ad, bd = dev(torch, a), dev(torch, b)
    v, g = h.softdtw(ad, bd, 1e-3, grad=True)
    v2, g2 = h.softdtw(ad, bd, 1e-3, grad=True)
    assert same_bits(v, v2) and same_bits(g, g2)
    only = h.softdtw(ad, bd, 1e-3)  # g_a == NULL: value only
    assert same_bits(only, v)
    for r in range(5):
        vr, gr = h.softdtw(ad[r:r + 1], bd[r:r + 1], 1e-3, grad=True)
        assert same_bits(vr, v[r:r + 1]) and same_bits(gr, g[r:r + 1]), r


def test_large_batch_rods_equal_their_own_calls(torch_cuda, h):
    torch = torch_cuda
    B = 1024
    a, b = walks(17, B, 33, 37)
    ad, bd = dev(torch, a), dev(torch, b)
    v, g = h.softdtw(ad, bd, 1e-2, grad=True)
    assert same_bits(h.softdtw(ad, bd, 1e-2), v)
    for r in (0, 511, 1023):
        vr, gr = h.softdtw(ad[r:r + 1], bd[r:r + 1], 1e-2, grad=True)
        assert same_bits(vr, v[r:r + 1]) and same_bits(gr, g[r:r + 1]), r


@pytest.mark.parametrize("Ta,Tb", [(5, 4), (101, 101)])
def test_a_non_finite_rod_is_nan_and_alone(torch_cuda, h, Ta, Tb):
    torch = torch_cuda
    a, b = walks(19, 4, Ta, Tb)
    ad, bd = dev(torch, a), dev(torch, b)
    v0, g0 = h.softdtw(ad, bd, 1e-2, grad=True)
    for where, bad in (("a", float("nan")), ("a", float("inf")), ("b", float("nan")), ("b", -float("inf"))):
        a2, b2 = ad.clone(), bd.clone()
        (a2 if where == "a" else b2)[2, (Ta if where == "a" else Tb) - 1, 1] = bad
        v, g = h.softdtw(a2, b2, 1e-2, grad=True)
        assert torch.isnan(v[2]) and torch.isnan(g[2]).all(), (where, bad)
        keep = [0, 1, 3]
        assert same_bits(v[keep], v0[keep]) and same_bits(g[keep], g0[keep]), (where, bad)
        assert torch.isnan(h.softdtw(a2, b2, 1e-2)[2])


def test_every_refusal_leaves_the_outputs_untouched(torch_cuda, h):
    import krod_native as kn
    torch = torch_cuda
    lib, S = h.lib, kn._stream()
    B, Ta, Tb = 2, 101, 101
    a, b = walks(23, B, Ta, Tb)
    ad, bd = dev(torch, a), dev(torch, b)
    value = torch.full((B,), SENTINEL, dtype=torch.float64, device=DEV)
    g = torch.full((B, Ta, 3), SENTINEL, dtype=torch.float64, device=DEV)
    nbytes = int(lib.kr_softdtw_ws_bytes(B, Ta, Tb, 1))
    assert nbytes > 0
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    L = kn.KR_SOFTDTW_MAX_LEN

    def args(**kw):
        d = dict(h=h._h, B=B, a=P(ad), Ta=Ta, ars=3 * Ta, ass=3, b=P(bd), Tb=Tb, brs=3 * Tb, bss=3, gamma=1e-2, cost=0,
                 value=P(value), g=P(g), grs=3 * Ta, gss=3, ws=P(ws), dtype=kn.KR_F64)
        d.update(kw)
        return tuple(d.values())

    refusals = [("null handle", dict(h=None), kn.KR_E_ARG), ("null a", dict(a=None), kn.KR_E_ARG), ("null b", dict(b=None), kn.KR_E_ARG),
                ("null value", dict(value=None), kn.KR_E_ARG), ("B = 0", dict(B=0), kn.KR_E_ARG), ("Ta = 0", dict(Ta=0), kn.KR_E_ARG),
                ("Tb = 0", dict(Tb=0), kn.KR_E_ARG), ("a rod stride < 0", dict(ars=-1), kn.KR_E_ARG),
                ("a step stride < 0", dict(ass=-3), kn.KR_E_ARG), ("b rod stride < 0", dict(brs=-1), kn.KR_E_ARG),
                ("b step stride < 0", dict(bss=-3), kn.KR_E_ARG), ("g rod stride 0", dict(grs=0), kn.KR_E_ARG),
                ("g step stride 0", dict(gss=0), kn.KR_E_ARG), ("g step stride < 0", dict(gss=-3), kn.KR_E_ARG),
                ("gamma = 0", dict(gamma=0.0), kn.KR_E_ARG), ("gamma < 0", dict(gamma=-1e-2), kn.KR_E_ARG),
                ("gamma = inf", dict(gamma=float("inf")), kn.KR_E_ARG), ("gamma = nan", dict(gamma=float("nan")), kn.KR_E_ARG),
                ("cost = 2", dict(cost=2), kn.KR_E_ARG), ("cost = -1", dict(cost=-1), kn.KR_E_ARG), ("dtype = 7", dict(dtype=7), kn.KR_E_ARG),
                ("ws NULL, size nonzero", dict(ws=None), kn.KR_E_ARG), ("Ta > max", dict(Ta=L + 1), kn.KR_E_UNSUPPORTED),
                ("Tb > max", dict(Tb=L + 1), kn.KR_E_UNSUPPORTED)]
    for label, kw, code in refusals:
        assert lib.kr_softdtw_batch(*args(**kw), S) == code, label
        assert lib.kr_last_error(), label
    torch.cuda.synchronize()
    assert (value == SENTINEL).all() and (g == SENTINEL).all()
    # what is not refused: ws NULL with value only; strides of g are not looked at without g_a
    assert lib.kr_softdtw_batch(*args(g=None, grs=0, gss=0, ws=None), S) == 0
    assert lib.kr_softdtw_batch(*args(), S) == 0
    torch.cuda.synchronize()
    assert (value != SENTINEL).all() and (g != SENTINEL).all()
    with pytest.raises(kn.KrError, match="strides > 0"):
        h.softdtw(ad, bd, 1e-2, g_out=g[:1].expand(B, Ta, 3))
    with pytest.raises(kn.KrError, match="g_out must be"):
        h.softdtw(ad, bd, 1e-2, g_out=g[:, :50])


# ---------------------------------------------------------------------------
# 4. end to end: the loss on a rollout's tip path
# ---------------------------------------------------------------------------
def test_loss_on_a_rollout_end_to_end(torch_cuda, robot, h):
    """softdtw_loss(simulate_tips(robot, ctl), ref).sum().backward() = rollout_grad(g_states = g) with g seeded by
    Handle.softdtw(g_out = ...), bit for bit; and along one fixed random direction <ctl.grad, d> is the central difference
    of the same loss through the device's own forward call (tol 1e-12) under the rule of the adjoint tests: ten times the
    disagreement of the step sizes 1e-4 and 5e-5, plus what the quotient cannot resolve (one rounding of the loss over 2 h,
    step_adjoint_cases.fd_floor)."""
    import cosserat_oracle as orc
    import krod_grad as kg
    torch = torch_cuda
    N, T, B, gamma = 10, 5, 2, 1e-2
    assert h.N == N
    ctl = dev(torch, orc.batch_sine_controls(B, T, robot.del_t, 5))
    states, tip, status = kg.forward_states(h, ctl, tol=1e-12)
    assert (status == 0).all()
    # a recorded path that is not sample-aligned: 7 samples along rod 0's tip path, shifted
    tp = tip[0].cpu().numpy()
    ref = dev(torch, np.stack([np.interp(np.linspace(0, T - 1, 7), np.arange(T), tp[:, k]) for k in range(3)], axis=1)
              + np.array([2e-3, -1e-3, 1.5e-3]))
    leaf = ctl.clone().requires_grad_(True)
    loss = kg.softdtw_loss(robot, kg.simulate_tips(robot, leaf), ref, gamma)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (B,)
    loss.sum().backward()
    assert leaf.grad is not None and torch.isfinite(leaf.grad).all() and leaf.grad.abs().sum() > 0
    g = torch.zeros_like(states)
    value, _ = h.softdtw(states[1:, :, N - 1, 12:15].permute(1, 0, 2), ref, gamma, g_out=g[1:, :, N - 1, 12:15].permute(1, 0, 2))
    assert same_bits(value, loss.detach())
    res = kg.rollout_grad(robot, ctl, states, g_states=g)
    assert np.array_equal(res["ctl"].view(np.uint64), leaf.grad.cpu().numpy().view(np.uint64))

    d = dev(torch, np.random.default_rng(3).standard_normal((B, T, 4)))

    def total(x):
        tips = kg.forward_states(h, x.contiguous(), tol=1e-12)[1]
        return h.softdtw(tips, ref, gamma).cpu().numpy()

    fd = {}
    for step in (1e-4, 5e-5):
        up, down = total(ctl + step * d), total(ctl - step * d)
        fd[step] = float((up.sum() - down.sum()) / (2 * step))
    got = float((leaf.grad * d).sum())
    floor = 2.0 ** -52 * float(np.abs(value.cpu().numpy()).sum()) / (2 * 5e-5)
    tol = 10.0 * abs(fd[1e-4] - fd[5e-5]) + floor
    err = abs(got - fd[5e-5])
    print(f"<ctl.grad, d> = {got:.12e}, central differences {fd[1e-4]:.12e} (1e-4) {fd[5e-5]:.12e} (5e-5): "
          f"error {err:.3e}, tolerance {tol:.3e}, ratio {err / tol:.3g}")
    assert err <= tol
