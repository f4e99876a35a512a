"""The parameter adjoint on the MI355X (kr_step_vjp_par_batch, kr_simulate_vjp_par_batch, krod_grad's physical
gradients) against central finite differences of the oracle's own step and rollout in the 43 material parameters (fixture
param_adjoint.npz, written by tests/golden/make_golden_param_adjoint.py; tests/param_adjoint_cases.py says how the step of
each block is chosen and why one step does not serve all).

Every comparison is per parameter block (E, r, rho, L, vstar, g, Bse, Bbt, C, tendon_dirs), never under one norm: the
sensitivities span twenty orders of magnitude.  A block's tolerance is the project's rule - ten times the disagreement of
the estimates at H and 2 H plus what the quotient cannot resolve - and is itself required to be at most 1e-2 of the block's
largest entry; a tendon_dirs row of a slack tendon is exactly zero.  Forward states are produced on the device with
tol = 1e-12.  Every figure is printed before it is asserted.
Measured (861 compared blocks): largest error / tolerance 0.78 (r; every other block <= 0.33); every tolerance at most 8e-4 of
its block's largest entry."""
import ctypes as C

import numpy as np
import pytest

import param_adjoint_cases as pc
import step_adjoint_cases as sc
from conftest import load_golden
from gpu_helpers import make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OTHERS = ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return load_golden("step_adjoint")


@pytest.fixture(scope="module")
def fp():
    return load_golden("param_adjoint")


_robots = {}


def robot_for(ps, N):
    if (ps, N) not in _robots:
        P = sc.params(ps, N)
        r = make_robot("noair" if ps == "noair" else None, N)
        for k in ("Bse", "Bbt", "F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
            setattr(r, k, np.array(getattr(P, k), dtype=np.float64))
        r.compute_intermediate_terms()
        _robots[(ps, N)] = r
    return _robots[(ps, N)]


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype or torch.float64).contiguous()


def step_batch(torch, fx, ps, N, state, rods, B, tens0=None):
    """B rods from the fixture's: rod b has the inputs of fixture rod b % rods, its tensions scaled by 1 + 0.003 (b // rods)
    - the first `rods` are the oracle's own.  The forward step runs here (tol 1e-12)."""
    h = robot_for(ps, N)._native()
    keys = [pc.step_key(ps, N, b % rods, state) for b in range(B)]
    prev = _dev(torch, np.stack([fx[k + "prev"] for k in keys]))
    cur = prev if state == "straight" else _dev(torch, np.stack([fx[k + "cur"] for k in keys]))
    tens = _dev(torch, np.stack([(fx[k + "tens"] if tens0 is None else tens0) * (1 + 0.003 * (b // rods)) for b, k in enumerate(keys)]))
    nxt = torch.zeros_like(prev)
    G = torch.zeros((B, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((B,), dtype=torch.int32, device=DEV)
    h.step(prev, cur, nxt, G, tens, tol=1e-12, status=status)
    assert (status == 0).all(), status
    return h, keys, prev, cur, nxt, tens


def same_bits(torch, a, b, names=OTHERS):
    return all(torch.equal(a[k], b[k], ) for k in names)


_worst = {}


@pytest.mark.parametrize("ps,N,rods,state", pc.STEP_CASES)
def test_step_par_against_the_oracle(torch_cuda, fx, fp, ps, N, rods, state):
    """g_par of the oracle's rods, block by block, against the finite differences for the first two cotangents; every other
    output bit for bit that of kr_step_vjp_batch; B = 3 and the same rods inside B = 5 (more than the four rods of a
    workgroup: the last workgroup is ragged) give the same bits per rod."""
    torch = torch_cuda
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, ps, N, state, rods, 5)
    for b in range(rods):  # (the device's step is the oracle's)
        assert np.max(np.abs(nxt[b].cpu().numpy() - fx[keys[b] + "next"])) < 1e-9
    for c in range(pc.N_COT):
        g_next = _dev(torch, np.stack([fx[k + "gbar"][c] * (1 + 0.1 * (b // rods)) for b, k in enumerate(keys)]))
        out = h.step_vjp(prev, cur, nxt, tens, g_next, need_par=True)
        assert (out["status"] == 0).all() and tuple(out["g_par"].shape) == (5, pc.KR_PAR)
        assert same_bits(torch, out, h.step_vjp(prev, cur, nxt, tens, g_next))
        small = h.step_vjp(prev[:3], cur[:3], nxt[:3], tens[:3], g_next[:3], need_par=True)
        assert same_bits(torch, small, {k: v[:3] for k, v in out.items()}, OTHERS + ("g_par",))
        for b in range(rods):
            pc.assert_blocks(out["g_par"][b].cpu().numpy(), fp[keys[b] + "fd_h"][c], fp[keys[b] + "fd_2h"][c], fp[keys[b] + "floor"][c],
                             f"{ps} N={N} {state} cot {c} rod {b}", _worst)
    print("largest error / tolerance per block so far:", {k: round(v, 3) for k, v in _worst.items()})


def test_slack_tendon_row_is_exactly_zero(torch_cuda, fx, fp):
    """tensions[2] = 0: the oracle's differences in that row of tendon_dirs are exactly zero, and so is the device's row."""
    torch = torch_cuda
    ps, N, rod, state = pc.ZERO_T_CASE
    key = "zeroT_" + pc.step_key(ps, N, rod, state)
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, ps, N, state, 1, 1, tens0=fp[key + "tens"])
    assert float(tens[0, 2]) == 0.0 and np.max(np.abs(nxt[0].cpu().numpy() - fp[key + "next"])) < 1e-9
    for c in range(pc.N_COT):
        out = h.step_vjp(prev, cur, nxt, tens, _dev(torch, fx[keys[0] + "gbar"][c][None]), need_par=True)
        got = out["g_par"][0].cpu().numpy()
        assert not np.any(fp[key + "fd_h"][c][37:40]) and not np.any(got[37:40]) and np.any(got[31:37])
        pc.assert_blocks(got, fp[key + "fd_h"][c], fp[key + "fd_2h"][c], fp[key + "floor"][c], f"slack tendon cot {c}")


def test_step_par_f32_is_the_f64_call_rounded(torch_cuda, fx):
    """dtype = KR_F32 is the element type only: g_par and every other output equal the fp64 call on the upcast inputs,
    rounded to float; and the fp32 call's other outputs are those of kr_step_vjp_batch in fp32, bit for bit."""
    torch = torch_cuda
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    f32 = [t.float().contiguous() for t in (prev, cur, nxt, tens, g_next)]
    lo = h.step_vjp(*f32, need_par=True)
    hi = h.step_vjp(*[t.double().contiguous() for t in f32], need_par=True)
    assert (lo["status"] == 0).all() and lo["g_par"].dtype == torch.float32
    for k in ("g_cur", "g_prev", "g_tensions", "g_bnd", "g_par"):
        assert torch.equal(lo[k], hi[k].float()), k
    assert torch.equal(lo["resid"], hi["resid"]) and torch.equal(lo["status"], hi["status"])
    assert same_bits(torch, lo, h.step_vjp(*f32))


def composition(torch, h, ctl, states, g):
    """kr_simulate_vjp_par_batch as the header defines it: the loop of step calls, g_par summed from zero, t = T - 1 first."""
    B, T = ctl.shape[0], ctl.shape[1]
    g = g.clone()
    g_par = torch.zeros((B, pc.KR_PAR), dtype=ctl.dtype, device=DEV)
    for t in range(T - 1, -1, -1):
        o = h.step_vjp(states[t - 1] if t > 0 else states[0], states[t], states[t + 1], ctl[:, t].contiguous(), g[t + 1], need_par=True)
        g[t] += o["g_cur"]
        g[max(t - 1, 0)] += o["g_prev"]
        g_par += o["g_par"]
    return g, g_par


def rollout_batch(torch, fx, ps, N, T, B=3):
    import krod_grad as kg
    h = robot_for(ps, N)._native()
    ctl0 = fx[pc.roll_key(ps, N, T) + "ctl"]
    ctl = _dev(torch, np.stack([ctl0 * (1 + 0.01 * b) for b in range(B)]))
    states, tip, status = kg.forward_states(h, ctl, tol=1e-12)
    assert (status == 0).all()
    return h, ctl, states


@pytest.mark.parametrize("ps,N,T", pc.ROLLOUT_CASES)
def test_simulate_par_against_the_oracle_and_the_step_calls(torch_cuda, fx, fp, ps, N, T):
    """g_par of rod 0, block by block, against the finite differences of the oracle's rollout (its straight initial state
    rebuilt from the perturbed parameters: no initial-state term is needed) for both cotangents; g_par is bit for bit the sum
    of the step calls in the defined order; every other output is bit for bit that of kr_simulate_vjp_batch, in fp64 and fp32."""
    torch = torch_cuda
    h, ctl, states = rollout_batch(torch, fx, ps, N, T)
    k = pc.roll_key(ps, N, T)
    for c in range(2):
        g0 = _dev(torch, np.repeat(fx[k + "gbar"][c][:, None], ctl.shape[0], axis=1))
        g, g_old = g0.clone(), g0.clone()
        out = h.simulate_vjp(ctl, states, g, need_par=True)
        old = h.simulate_vjp(ctl, states, g_old)
        assert (out["status"] == 0).all()
        assert torch.equal(g, g_old) and all(torch.equal(out[n], old[n]) for n in ("g_ctl", "g_bnd", "resid", "status"))
        ref_g, ref_par = composition(torch, h, ctl, states, g0)
        assert torch.equal(g, ref_g) and torch.equal(out["g_par"], ref_par)
        pc.assert_blocks(out["g_par"][0].cpu().numpy(), fp[k + "fd_h"][c], fp[k + "fd_2h"][c], fp[k + "floor"][c],
                         f"{ps} N={N} T={T} cot {c}", _worst)
        if c == 0:
            c32, s32, g32, g32_old = ctl.float(), states.float().contiguous(), g0.float().contiguous(), g0.float().contiguous()
            lo, lo_old = h.simulate_vjp(c32, s32, g32, need_par=True), h.simulate_vjp(c32, s32, g32_old)
            assert torch.equal(g32, g32_old) and all(torch.equal(lo[n], lo_old[n]) for n in ("g_ctl", "g_bnd", "resid", "status"))
            assert lo["g_par"].dtype == torch.float32 and bool(torch.isfinite(lo["g_par"]).all())
    print("largest error / tolerance per block so far:", {k: round(v, 3) for k, v in _worst.items()})


def test_nonfinite_rod_gets_nan_in_all_43(torch_cuda, fx):
    """One NaN rod in a batch of five: NaN in its 43 values, status KR_ST_NONFINITE; the other four rods are bit for bit the
    clean call.  Through the rollout: NaN in all of that rod's g_par, the others untouched."""
    torch = torch_cuda
    import krod_native as kn
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    clean = h.step_vjp(prev, cur, nxt, tens, g_next, need_par=True)
    assert bool(torch.isfinite(clean["g_par"]).all())
    bad_next = nxt.clone()
    bad_next[2, 4, 19] = float("nan")
    out = h.step_vjp(prev, cur, bad_next, tens, g_next, need_par=True)
    assert out["status"].tolist() == [0, 0, kn.ST_NONFINITE, 0, 0]
    assert bool(torch.isnan(out["g_par"][2]).all()) and bool(torch.isnan(out["g_tensions"][2]).all())
    keep = [0, 1, 3, 4]
    assert same_bits(torch, {k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in clean.items()}, OTHERS + ("g_par",))
    hr, ctl, states = rollout_batch(torch, fx, "bc", 10, 3)
    g0 = torch.zeros_like(states)
    g0[1:, :, 9, 12:15] = 1.0
    o_clean = hr.simulate_vjp(ctl, states, g0.clone(), need_par=True)
    bad = states.clone()
    bad[2, 1, 3, 20] = float("nan")
    o_bad = hr.simulate_vjp(ctl, bad, g0.clone(), need_par=True)
    assert bool(torch.isnan(o_bad["g_par"][1]).all())
    for b in (0, 2):
        assert torch.equal(o_bad["g_par"][b], o_clean["g_par"][b])


def test_refusals_leave_every_output_byte(torch_cuda, fx):
    """RK4: KR_E_UNSUPPORTED with a message; a null required pointer, B < 1, T < 1, a bad dtype: KR_E_ARG; nothing is launched
    or written, g_par included."""
    torch = torch_cuda
    import krod_native as kn
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "plain", 10, "sine30", 3, 3)
    lib, B, N = h.lib, 3, 10
    g_next = torch.ones_like(nxt)
    full = lambda *shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=DEV)
    outs = [full(B, N, 28), full(B, N, 28), full(B, 4), full(B, 19), full(B, pc.KR_PAR), full(B), full(B, dtype=torch.int32)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def step(B=B, scheme=kn.KR_EULER, g=g_next, dtype=kn.KR_F64, cur_=cur, tens_=tens):
        return lib.kr_step_vjp_par_batch(h._h, B, scheme, p(prev), p(cur_), p(nxt), p(tens_), p(g), *[p(o) for o in outs], dtype, None)
    for kw, want, word in ((dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"RK4"), (dict(g=None), kn.KR_E_ARG, b"null"),
                           (dict(cur_=None), kn.KR_E_ARG, b"null"), (dict(tens_=None), kn.KR_E_ARG, b"null"), (dict(B=0), kn.KR_E_ARG, b"B"),
                           (dict(dtype=5), kn.KR_E_ARG, b"dtype")):
        rc = step(**kw)
        assert rc == want and word in lib.kr_last_error() and (want != kn.KR_E_UNSUPPORTED or b"kr_step_vjp_par_batch" in lib.kr_last_error()), \
            (kw, rc, want, lib.kr_last_error())
    T = 2
    states = torch.zeros((T + 1, B, N, 28), dtype=torch.float64, device=DEV)
    ctl = torch.zeros((B, T, 4), dtype=torch.float64, device=DEV)
    g_states = full(T + 1, B, N, 28)
    souts = [full(B, N, 28), full(B, T, 4), full(B, 19), full(B, pc.KR_PAR), full(B, T), full(B, T, dtype=torch.int32)]

    def sim(B=B, T=T, scheme=kn.KR_EULER, st=states, dtype=kn.KR_F64):
        return lib.kr_simulate_vjp_par_batch(h._h, B, T, scheme, p(ctl), p(st), None, p(g_states), *[p(o) for o in souts], dtype, None)
    for kw, want, word in ((dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"RK4"), (dict(st=None), kn.KR_E_ARG, b"null"),
                           (dict(T=0), kn.KR_E_ARG, b"T < 1"), (dict(B=0), kn.KR_E_ARG, b"B"), (dict(dtype=-1), kn.KR_E_ARG, b"dtype")):
        rc = sim(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    assert lib.kr_step_vjp_par_batch(None, B, kn.KR_EULER, p(prev), p(cur), p(nxt), p(tens), p(g_next), *[p(o) for o in outs], kn.KR_F64,
                                     None) == kn.KR_E_ARG and b"handle" in lib.kr_last_error()
    torch.cuda.synchronize()
    for o in outs + souts + [g_states]:
        assert bool((o == 7).all())
    with pytest.raises(kn.KrError, match="MLP off only"):
        h.step_vjp(prev, cur, nxt, tens, g_next, use_nn=True, need_par=True)


def test_simulate_tips_physical_backward_is_the_direct_call(torch_cuda, fx):
    """theta = {E, Bbt, L}, B = 2, N = 10, T = 4: after backward() theta.grad and ctl.grad equal the direct
    simulate_vjp(need_par=True) results (g_par summed over B); rollout_grad(physical=True) returns the per-rod values; and
    dL/dE equals the central difference of the DEVICE's own forward loss, at two step sizes, by the tolerance rule - set_params,
    forward and backward are consistent end to end."""
    torch = torch_cuda
    import krod_grad as kg
    import krod_native as kn
    ps, N, T, B = "plain", 10, 4, 2
    P = sc.params(ps, N)
    r = make_robot(None, N)
    ctl = _dev(torch, sc.orc.batch_sine_controls(B, T, P.del_t, 11))
    theta = {"E": torch.tensor(float(r.E), dtype=torch.float64, requires_grad=True),
             "Bbt": torch.tensor(np.array(r.Bbt, dtype=np.float64), requires_grad=True),
             "L": torch.tensor(float(r.L), dtype=torch.float64, requires_grad=True)}
    w = _dev(torch, np.random.default_rng(3).normal(size=(B, T, 3)))
    leaf = ctl.clone().requires_grad_(True)
    tips = kg.simulate_tips_physical(r, leaf, theta)
    assert tuple(tips.shape) == (B, T, 3)
    (tips * w).sum().backward()
    h = r._native()
    states, tip, status = kg.forward_states(h, ctl, tol=1e-12)
    assert (status == 0).all() and torch.equal(tip, tips.detach())
    g = torch.zeros_like(states)
    g[1:, :, N - 1, 12:15] = w.permute(1, 0, 2)
    direct = h.simulate_vjp(ctl, states, g.clone(), need_par=True)
    by_name = kn.split_par(direct["g_par"].sum(dim=0))
    assert torch.equal(leaf.grad, direct["g_ctl"])
    for k in theta:
        assert theta[k].grad is not None and tuple(theta[k].grad.shape) == tuple(theta[k].shape)
        assert torch.equal(theta[k].grad.to(DEV), by_name[k]), k
    res = kg.rollout_grad(r, ctl, states, g_tips=w.cpu().numpy(), physical=True)
    assert set(res["physical"]) == set(pc.BLOCK_NAMES) and res["physical"]["tendon_dirs"].shape == (B, 4, 3)
    assert res["physical"]["Bse"].shape == (B, 3, 3) and res["physical"]["E"].shape == (B,)
    assert np.array_equal(res["physical"]["E"], direct["g_par"][:, 0].cpu().numpy())
    assert np.array_equal(res["physical"]["Bbt"].reshape(B, 9), direct["g_par"][:, 19:28].cpu().numpy())

    E0 = float(r.E)

    def loss_at(E):
        r.E = E
        r.compute_intermediate_terms()
        _, tp, st = kg.forward_states(r._native(), ctl, tol=1e-12)
        assert (st == 0).all()
        return float((tp * w).sum())
    H = 1e-4  # the device's forward stops at its tolerance, not at rounding: a step large enough to stand above it
    fd = [(loss_at(E0 * (1 + s)) - loss_at(E0 * (1 - s))) / (2 * s * E0) for s in (H, 2 * H)]
    r.E = E0
    r.compute_intermediate_terms()
    # What the quotient cannot resolve.  A forward step stops with its tip residual (a force, a moment) within 1e-12; M =
    # d(n, m)_tip / dG has entries of order one and cond(M) ~ 2, so the base wrench is within ~2e-12 of the root; the
    # tip moves by at most the cantilever's compliance L^3 / (3 E I) per unit of base force; every one of the T steps adds
    # its own miss to the states the later ones start from.  Two evaluations per quotient.
    compliance = float(r.L) ** 3 / (3 * E0 * np.pi * float(r.r) ** 4 / 4)
    tip_miss = 2e-12 * compliance * T
    floor = 2 * tip_miss * float(w.abs().sum()) / (2 * H * E0)
    got = float(theta["E"].grad)
    tol = sc.block_tol(fd[0], fd[1], floor)
    print(f"dL/dE adjoint {got:.6e} device fd {fd[0]:.6e} (2H: {fd[1]:.6e}) err {abs(got - fd[0]):.2e} tol {tol:.2e}")
    assert tol <= pc.MAX_REL_TOL * abs(fd[0]) and abs(got - fd[0]) <= tol
    with pytest.raises(kn.KrError, match="unknown parameter"):
        kg.simulate_tips_physical(r, leaf, {"del_t": torch.tensor(0.05)})
    with pytest.raises(kn.KrError, match="shape"):
        kg.simulate_tips_physical(r, leaf, {"Bbt": torch.zeros(3)})
