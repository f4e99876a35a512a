"""GPU tests of the optimizer kernels (``-m gpu``): kr_adam_step / kr_adam_plateau_step entry by entry against the same
formula in fp64 NumPy with a counted rounding bound, and the device-side plateau schedule step by step against
torch.optim.lr_scheduler.ReduceLROnPlateau on scripted losses."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24           # unit roundoff of fp32 (round to nearest)
SECOND_ORDER = 1 + 1e-6  # (1 + U)^count - 1 <= count U (1 + 1e-6) for the counts below
B1, B2, EPS = 0.9, 0.999, 1e-8
PAD = 64                 # sentinel entries behind every buffer


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import krod_native as kn
    p = kn.KrParams()
    kn.check(kn.load().kr_default_params(C.byref(p)))
    p.N = 10
    return torch, kn, kn.Handle(p)


@pytest.fixture(scope="module")
def inputs():
    """n -> p0, g, m0, v0 (float32).  Gradients span eight decades, a tenth of them exact zeros; the first tenth of the
    entries is 'fresh' (g = m = v = 0: the update is 0 / eps = 0); the rest carries moments of the gradient's size."""
    memo = {}

    def get(n):
        if n not in memo:
            rng = np.random.default_rng(n)
            g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
            g[rng.random(n) < 0.1] = 0.0
            m0 = (np.abs(g) + 1e-3) * rng.standard_normal(n)
            v0 = (np.abs(g) + 1e-3) ** 2 * rng.uniform(0.1, 2.0, n)
            p0 = 0.02 * rng.standard_normal(n)
            fresh = np.arange(n) < max(n // 10, 1)
            g[fresh], m0[fresh], v0[fresh] = 0.0, 0.0, 0.0
            memo[n] = tuple(a.astype(np.float32) for a in (p0, g, m0, v0)) + (fresh,)
        return memo[n]
    return get


def adam_reference(p0, g, m0, v0, step_size, wd, inv_sqrt_bc2):
    """adam_kernel's formula in fp64 on the fp32 inputs, with the fp32-rounded constants the kernel receives, and the
    entrywise bounds of the module's rounding count.  -> (m, bound_m, v, bound_v, update(m_dev, v_dev))"""
    f32 = lambda a: float(np.float32(a))
    b1, b2, eps, wd = f32(B1), f32(B2), f32(EPS), f32(wd)
    c1, c2 = f32(np.float32(1) - np.float32(B1)), f32(np.float32(1) - np.float32(B2))  # (exact in fp32: Sterbenz)
    p0, g, m0, v0 = (np.asarray(a, np.float64) for a in (p0, g, m0, v0))
    gi = wd * p0 + g
    agi = np.abs(wd * p0) + np.abs(g)
    m = b1 * m0 + c1 * gi
    v = b2 * v0 + c2 * gi * gi
    prop = 1 if wd != 0.0 else 0                       # the rounding of fmaf(wd, p, g), carried once into m, twice into v
    bound_m = (2 + prop) * U * SECOND_ORDER * (np.abs(b1 * m0) + c1 * agi)
    bound_v = (3 + 2 * prop) * U * SECOND_ORDER * (np.abs(b2 * v0) + c2 * agi * agi)

    def update(m_dev, v_dev):
        """p0 - step_size m / (sqrt(v) isb + eps) from the DEVICE's m and v (they are the kernel's operands), and its bound"""
        upd = step_size * (np.asarray(m_dev, np.float64) / (np.sqrt(np.asarray(v_dev, np.float64)) * inv_sqrt_bc2 + eps))
        return p0 - upd, 6 * U * SECOND_ORDER * (np.abs(p0) + np.abs(upd))
    return m, bound_m, v, bound_v, update


NS = [1, 255, 257, 27000, 2 * 262144 + 37]


@pytest.mark.parametrize("kind", ["adam", "plateau"])
@pytest.mark.parametrize("n", NS)
def test_adam_kernels_entrywise(env, inputs, n, kind):
    """kr_adam_step (adam_kernel) and kr_adam_plateau_step (adam_plateau_kernel), n_zero in {n, n + 1, n + 300} (the
    plateau call needs a loss slot: the last two), lower NULL / given, weight decay 0 / 1e-3, step 1 / 2 / 1000;
    n = 524 325 runs the grid-stride loop (1024 x 256 threads).

    fp32 roundings on each value's path (the library is built without fast-math, and hipcc's default keeps sqrtf and /
    correctly rounded: one rounding each; -ffp-contract=fast can only fuse a product into a sum, i.e. remove one):
      gi  = fmaf(wd, p, g)                       1 (weight decay only)
      m   = fmaf(b1, m0, (1 - b1) gi)            2: the product, the fma (+ 1 carried from gi); 1 - b1 is exact
      v   = fmaf(b2, v0, ((1 - b2) gi) gi)       3: two products, the fma (+ 2 carried from gi)
      p   = p0 - step_size (m / (sqrtf(v) isb + eps))   6: sqrt, product, sum (all terms positive: relative), quotient,
            product, difference - from the m and v the kernel itself wrote, which are its operands
    bound = count x 2^-24 x sum of the magnitudes of the terms (x (1 + 1e-6) for the second order).  The clamp max(p,
    lower) is 1-Lipschitz: the same bound holds behind it, and p >= lower holds exactly."""
    torch, kn, h = env
    p0, g, m0, v0, fresh = inputs(n)
    lower_np = np.where(np.arange(n) % 2 == 0, 0.0, -np.inf).astype(np.float32)
    worst = {"exp_avg": 0.0, "exp_avg_sq": 0.0, "params": 0.0}
    bound_hits = 0
    extras = (0, 1, 300) if kind == "adam" else (1, 300)
    for extra, clamp, wd, step in itertools.product(extras, (False, True), (0.0, 1e-3), (1, 2, 1000)):
        n_zero = n + extra
        lr = 1e-2
        bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
        isb = float(np.float32(1.0 / math.sqrt(bc2)))
        if kind == "adam":
            step_size = float(np.float32(lr / bc1))
        else:
            step_size = float(np.float32(lr * float(np.float32(1.0 / bc1))))
        sentinel = lambda k: np.full(k, 123.25, np.float32)
        dev = lambda a, size: torch.tensor(np.concatenate([a, sentinel(size - a.size + PAD)]), device=DEV)
        loss_value = np.float32(0.75)
        g_full = np.concatenate([g, np.full(extra, loss_value, np.float32)])  # trailing slots: the loss and other sums
        P, G, M, V = dev(p0, n), dev(g_full, n_zero), dev(m0, n), dev(v0, n)
        L = torch.tensor(lower_np, device=DEV) if clamp else None
        if kind == "adam":
            kn.check(h.lib.kr_adam_step(h._h, n, kn._ptr(P), kn._ptr(G), kn._ptr(M), kn._ptr(V), kn._ptr(L), lr, B1, B2, EPS, wd,
                                        step, n_zero, kn._stream()))
        else:
            sched = torch.tensor([lr, lr, float("inf"), 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
            log = torch.zeros(1, dtype=torch.float32, device=DEV)
            kn.check(h.lib.kr_adam_plateau_step(h._h, n, kn._ptr(P), kn._ptr(G), kn._ptr(M), kn._ptr(V), kn._ptr(L), kn._ptr(sched),
                                                B1, B2, EPS, wd, step, n_zero, n, 0.5, 10, 1e-4, 0.0, kn._ptr(log), kn._stream()))
        torch.cuda.synchronize()
        P, G, M, V = (t.cpu().numpy() for t in (P, G, M, V))
        what = (kind, n, n_zero, clamp, wd, step)
        # exact: the gradient buffer is zero up to n_zero and nothing behind any buffer's end was touched
        assert not G[:n_zero].any(), what
        assert np.array_equal(G[n_zero:], sentinel(PAD)), what
        for a in (P, M, V):
            assert np.array_equal(a[n:], sentinel(PAD)), what
        if kind == "plateau":
            s = sched.cpu().numpy()
            assert float(log) == float(loss_value) and s[4] == float(loss_value) and s[2] == float(loss_value), what
            assert s[step & 1] == lr and s[3] == 0.0 and s[5] == 0.0, what
        m_ref, bm, v_ref, bv, update = adam_reference(p0, g, m0, v0, step_size, wd, isb)
        p_ref, bp = update(M[:n], V[:n])
        if clamp:
            assert np.all(P[:n] >= lower_np), what                          # exactly
            binds = p_ref < lower_np - bp
            assert np.array_equal(P[:n][binds], lower_np[binds]), what      # where the clamp binds: the bound itself
            bound_hits += int(binds.sum())
            p_ref = np.maximum(p_ref, lower_np)
        if wd == 0.0:
            assert np.array_equal(P[:n][fresh], np.maximum(p0[fresh], lower_np[fresh]) if clamp else p0[fresh]), what
            assert not M[:n][fresh].any() and not V[:n][fresh].any(), what
        for name, got, ref, bound in (("exp_avg", M[:n], m_ref, bm), ("exp_avg_sq", V[:n], v_ref, bv), ("params", P[:n], p_ref, bp)):
            err = np.abs(got.astype(np.float64) - ref)
            ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
            worst[name] = max(worst[name], ratio)
            assert ratio <= 1.0, (what, name, ratio, int(np.argmax(err - bound)))
    print(f"D1 {kind} n = {n}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; entries held at the clamp: {bound_hits}")
    assert bound_hits > 0 or n == 1


SCRIPTS = {
    # name: (losses, lr, factor, patience, threshold, min_lr)
    "strictly_improving": ([0.9 ** k for k in range(12)], 1e-2, 0.5, 2, 1e-4, 0.0),
    "flat": ([1.0] * 14, 1e-2, 0.5, 2, 1e-4, 0.0),
    # strictly decreasing, but never by more than 0.9e-4 of the first loss in total: no epoch is "better"
    "improving_by_less_than_the_threshold": ([1.0 - 0.9e-4 * (1.0 - 0.5 ** k) for k in range(14)], 1e-2, 0.5, 3, 1e-4, 0.0),
    "nan_in_the_middle": ([1.0, 0.9, float("nan"), 0.8, 0.85, 0.85, 0.85, float("nan"), float("nan"), float("nan"), 0.5, 0.6],
                          1e-2, 0.5, 1, 1e-4, 0.0),
    "patience_0_next_to_improving": ([1.0, 0.9, 0.95, 0.8, 0.7, 0.75, 0.6, 0.6, 0.59], 1e-2, 0.5, 0, 1e-4, 0.0),
    "min_lr_binds": ([1.0] * 8, 1e-2, 0.1, 0, 1e-4, 3e-4),
    "rate_too_small_to_reduce": ([1.0] * 8, 1.5e-8, 0.5, 1, 1e-4, 0.0),
}


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_plateau_schedule_step_by_step(env, name):
    """adam_plateau_kernel's schedule on scripted losses (n = 1; the loss is written into grads[loss_index] before each
    call) against torch's ReduceLROnPlateau(mode min, relative threshold, cooldown 0) after EVERY step: the next rate as
    doubles, best, bad epochs, the number of reductions, the logged loss."""
    torch, kn, h = env
    losses, lr, factor, patience, threshold, min_lr = SCRIPTS[name]
    probe = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(probe, "min", factor=factor, patience=patience, threshold=threshold,
                                                     threshold_mode="rel", cooldown=0, min_lr=min_lr, eps=1e-8)
    z = lambda k: torch.zeros(k, dtype=torch.float32, device=DEV)
    p, g, m, v, log = torch.full((1,), 0.5, device=DEV), z(2), z(1), z(1), z(1)
    sched = torch.tensor([lr, lr, float("inf"), 0.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    reductions, rates = 0, []
    for step, loss in enumerate(losses, start=1):
        loss32 = float(np.float32(loss))
        g.copy_(torch.tensor([0.25, loss32], dtype=torch.float32))
        kn.check(h.lib.kr_adam_plateau_step(h._h, 1, kn._ptr(p), kn._ptr(g), kn._ptr(m), kn._ptr(v), None, kn._ptr(sched), B1, B2, EPS,
                                            0.0, step, 2, 1, factor, patience, threshold, min_lr, kn._ptr(log), kn._stream()))
        torch.cuda.synchronize()
        before = probe.param_groups[0]["lr"]
        ref.step(loss32)
        after = probe.param_groups[0]["lr"]
        reductions += int(after != before)
        s = sched.cpu().numpy()
        what = (name, step, s.tolist(), after, ref.best, ref.num_bad_epochs)
        assert s[step & 1] == after, what
        assert s[(step - 1) & 1] == before, what      # the rate this step used stays where it was
        assert s[2] == ref.best, what
        assert s[3] == float(ref.num_bad_epochs), what
        assert s[5] == float(reductions), what
        got_log = float(log)
        assert (math.isnan(got_log) and math.isnan(s[4])) if math.isnan(loss32) else (got_log == loss32 and s[4] == loss32), what
        assert float(g.abs().max()) == 0.0, what
        rates.append(after)
    expect_reductions = {"strictly_improving": 0, "rate_too_small_to_reduce": 0, "min_lr_binds": 2}
    if name in expect_reductions:
        assert reductions == expect_reductions[name], (name, reductions, rates)
    else:
        assert reductions >= 2, (name, reductions, rates)
    if name == "min_lr_binds":
        assert rates[-1] == min_lr
    if name == "nan_in_the_middle":
        assert not math.isnan(float(sched[2])) and float(sched[2]) == 0.5
