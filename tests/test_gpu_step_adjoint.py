"""The step adjoint on the MI355X (kr_step_vjp_batch, kr_simulate_vjp_batch, krod_grad) against central finite
differences of the oracle's own step and rollout (fixture step_adjoint.npz, written by
tests/golden/make_golden_step_adjoint.py from cosserat_oracle.residual_euler + newton_shoot; solved to 1e-15, tighter than
the 1e-13 first planned, which leaves a bias the two step sizes agree on: step_adjoint_cases.py says why).

Tolerances are not fixed in advance: every finite difference exists at two step sizes, H and 2 H, and a block's
tolerance is ten times the two estimates' disagreement (truncation falls by four between them) plus what the difference
quotient itself cannot resolve (step_adjoint_cases.fd_floor: one rounding of the loss over 2 H - without it a block on
which the two estimates agree to the last bit, e.g. the pass-through of v, u of the last point, would demand more digits
than the quotient holds).  Blocks are compared one by one (q, w, v, u of g_cur and g_prev, the tensions, the six parts
of the boundary), never under one norm.  Forward states are produced on the device with tol = 1e-12.  Every figure is
printed before it is asserted.
Measured (2241 compared blocks): largest error / tolerance 0.47; resid <= 2.1e-15.
Oracle comparison covers three rods per case up to N = 33 and one rod at N = 100, 130 (the fixture's cost is in the
long rods); every rod of every batch is compared bit for bit with its own B = 1 call."""
import ctypes as C

import numpy as np
import pytest

import step_adjoint_cases as sc
from conftest import load_golden
from gpu_helpers import make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESID_MAX = 1e-10  # cond(M) ~ 2 on every fixture: the 6 x 6 solve leaves rounding only


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return load_golden("step_adjoint")


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


def step_batch(torch, fx, ps, N, state, rods, B):
    """B rods from the fixture's: rod b has the inputs of fixture rod b % rods, its tensions scaled by 1 + 0.003 (b // rods)
    - the first `rods` are the oracle's own.  The forward step runs here (tol 1e-12)."""
    h = robot_for(ps, N)._native()
    keys = [sc.case_key(ps, N, state) + f"_r{b % rods}_" for b in range(B)]
    prev = _dev(torch, np.stack([fx[k + "prev"] for k in keys]))
    cur = prev if state == "straight" else _dev(torch, np.stack([fx[k + "cur"] for k in keys]))
    tens = _dev(torch, np.stack([fx[k + "tens"] * (1 + 0.003 * (b // rods)) for b, k in enumerate(keys)]))
    nxt = torch.zeros_like(prev)
    G = torch.zeros((B, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((B,), dtype=torch.int32, device=DEV)
    h.step(prev, cur, nxt, G, tens, tol=1e-12, status=status)
    assert (status == 0).all(), status
    for b in range(min(rods, B)):  # (the device's step is the oracle's)
        assert np.max(np.abs(nxt[b].cpu().numpy() - fx[keys[b] + "next"])) < 1e-9
    return h, keys, prev, cur, nxt, tens


def got_vector(out, b):
    return np.concatenate([out["g_cur"][b, :, :12].cpu().numpy().ravel(), out["g_prev"][b, :, :12].cpu().numpy().ravel(),
                           out["g_tensions"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy()])


def same_bits(torch, a, b):
    return all(torch.equal(a[k], b[k]) for k in ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status"))


STEP_RUNS = [(ps, N, rods, state, 5) for ps, N, rods, state in sc.STEP_CASES] + \
            [(ps, N, rods, state, B) for ps, N, rods, state in (("bc", 10, 3, "sine30"), ("plain", 2, 3, "sine30"), ("plain", 130, 1, "sine30"))
             for B in (1, 70)]


@pytest.mark.parametrize("ps,N,rods,state,B", STEP_RUNS)
def test_step_vjp_against_the_oracle(torch_cuda, fx, ps, N, rods, state, B):
    """Every output block of the oracle's rods against the finite differences, for the three cotangents (all 25 slots of
    all points; tip position only; v, u of the last point only); structural zeros exact; resid; every rod bit-identical
    to its own B = 1 call.  state "straight": q = 0 (the kink of q|q|) and state_prev ALIASES state_cur."""
    torch = torch_cuda
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, ps, N, state, rods, B)
    for c in range(3):
        gbar = np.stack([fx[k + "gbar"][c] * (1 + 0.1 * (b // rods)) for b, k in enumerate(keys)])
        g_next = _dev(torch, gbar)
        out = h.step_vjp(prev, cur, nxt, tens, g_next)
        assert (out["status"] == 0).all()
        resid = out["resid"].cpu().numpy()
        print(f"{ps} N={N} {state} B={B} cotangent {c}: resid max {resid.max():.2e}")
        assert np.all(resid <= RESID_MAX)
        for name in ("g_cur", "g_prev"):
            assert torch.count_nonzero(out[name][:, :, 12:]) == 0, name  # slots 12..24 (p columns among them) and the pads
        for b in range(min(rods, B)):
            floor = sc.fd_floor(gbar[b], nxt[b].cpu().numpy())
            for name, err, tol, size in sc.block_report(got_vector(out, b), fx[keys[b] + "fd_h"][c], fx[keys[b] + "fd_2h"][c], N, floor):
                print(f"  rod {b} {name:14s} err {err:.3e} tol {tol:.3e} size {size:.3e}")
                assert err <= tol, (ps, N, state, c, b, name, err, tol)
        if c == 2:  # the pass-through: v, u of the last point go to state_cur unchanged, nothing else moves
            assert torch.equal(out["g_cur"][:, N - 1, 6:12], g_next[:, N - 1, 6:12])
            assert torch.count_nonzero(out["g_cur"][:, :N - 1]) == 0 and torch.count_nonzero(out["g_prev"]) == 0
            assert torch.count_nonzero(out["g_tensions"]) == 0 and torch.count_nonzero(out["g_bnd"]) == 0
        for b in (range(B) if c == 0 else range(min(3, B))):
            one = h.step_vjp(prev[b:b + 1], cur[b:b + 1], nxt[b:b + 1], tens[b:b + 1], g_next[b:b + 1])
            assert same_bits(torch, one, {k: v[b:b + 1] for k, v in out.items()}), (c, b)


def test_step_vjp_f32_is_the_f64_call_rounded(torch_cuda, fx):
    """dtype = KR_F32 is the element type only: the call equals the fp64 call on the upcast inputs, rounded to float."""
    torch = torch_cuda
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    f32 = [t.float().contiguous() for t in (prev, cur, nxt, tens, g_next)]
    lo = h.step_vjp(*f32)
    hi = h.step_vjp(*[t.double().contiguous() for t in f32])
    assert (lo["status"] == 0).all() and lo["g_cur"].dtype == torch.float32
    for k in ("g_cur", "g_prev", "g_tensions", "g_bnd"):
        assert torch.equal(lo[k], hi[k].float()), k
    assert torch.equal(lo["resid"], hi["resid"]) and torch.equal(lo["status"], hi["status"])


def composition(torch, h, ctl, states, g, prev_init=None):
    """kr_simulate_vjp_batch as the header defines it: the loop of step adjoints."""
    B, T = ctl.shape[0], ctl.shape[1]
    g = g.clone()
    g_ctl = torch.zeros((B, T, 4), dtype=ctl.dtype, device=DEV)
    g_bnd = torch.zeros((B, 19), dtype=ctl.dtype, device=DEV)
    resid = torch.zeros((B, T), dtype=torch.float64, device=DEV)
    status = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    g_prev_init = None
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else (prev_init if prev_init is not None else states[0])
        o = h.step_vjp(prev, states[t], states[t + 1], ctl[:, t].contiguous(), g[t + 1])
        g[t] += o["g_cur"]
        if t > 0 or prev_init is None:
            g[max(t - 1, 0)] += o["g_prev"]
        else:
            g_prev_init = o["g_prev"]
        g_ctl[:, t] = o["g_tensions"]
        g_bnd += o["g_bnd"]
        resid[:, t], status[:, t] = o["resid"], o["status"]
    return dict(g_states=g, g_ctl=g_ctl, g_bnd=g_bnd, resid=resid, status=status, g_prev_init=g_prev_init)


def rollout_batch(torch, fx, ps, N, T, B=3):
    import krod_grad as kg
    h = robot_for(ps, N)._native()
    ctl0 = fx[f"roll_{ps}_N{N}_T{T}_ctl"]
    ctl = _dev(torch, np.stack([ctl0 * (1 + 0.01 * b) for b in range(B)]))
    states, tip, status = kg.forward_states(h, ctl, tol=1e-12)
    assert (status == 0).all()
    return h, ctl, states


@pytest.mark.parametrize("ps,N,T", sc.ROLLOUT_CASES)
def test_simulate_vjp_against_the_oracle_and_the_step_calls(torch_cuda, fx, ps, N, T):
    """g_ctl (all 4 T entries, a block per step), g_bnd (six blocks) and the chosen entries of g_states[0] (a block per
    q, w, v, u) of rod 0 against the finite differences of the oracle's rollout - for a tip cotangent on every step and
    for a cotangent at ONE interior state only; and the call is bit for bit the loop of kr_step_vjp_batch calls."""
    torch = torch_cuda
    h, ctl, states = rollout_batch(torch, fx, ps, N, T)
    k = f"roll_{ps}_N{N}_T{T}_"
    ent = sc.rollout_state0_entries(N)
    for c in range(2):
        gbar = fx[k + "gbar"][c]
        g0 = _dev(torch, np.repeat(gbar[:, None], ctl.shape[0], axis=1))
        g = g0.clone()
        out = h.simulate_vjp(ctl, states, g)
        assert (out["status"] == 0).all() and float(out["resid"].max()) <= RESID_MAX
        ref = composition(torch, h, ctl, states, g0)
        assert torch.equal(g, ref["g_states"]) and all(torch.equal(out[n], ref[n]) for n in ("g_ctl", "g_bnd", "resid", "status"))
        got = np.concatenate([out["g_ctl"][0].cpu().numpy().ravel(), out["g_bnd"][0].cpu().numpy(),
                              [float(g[0, 0, j, s]) for j, s in ent]])
        a, b = fx[k + "fd_h"][c], fx[k + "fd_2h"][c]
        floor = sc.fd_floor(gbar, states[:, 0].cpu().numpy())
        blocks = [(f"g_ctl[{t}]", list(range(4 * t, 4 * t + 4))) for t in range(T)]
        blocks += [(bl[0], list(range(4 * T + bl[2].start, 4 * T + bl[2].stop))) for bl in sc.BLOCKS if bl[1] == "bnd"]
        blocks += [(f"g_states[0].{n}", [4 * T + 19 + i for i, (j, s) in enumerate(ent) if s // 3 == q]) for q, n in enumerate("qwvu")]
        for name, idx in blocks:
            err, tol = np.max(np.abs(got[idx] - a[idx])), sc.block_tol(a[idx], b[idx], floor)
            print(f"{ps} N={N} T={T} cotangent {c} {name:16s} err {err:.3e} tol {tol:.3e} size {np.max(np.abs(a[idx])):.3e}")
            assert err <= tol, (name, err, tol)


def test_simulate_vjp_continued_run(torch_cuda, fx):
    """state_prev_init given: the second half of a run, continued, gives the g_ctl of the whole run's second half (bit for
    bit: the same step adjoints), its g_prev_init is what the whole run adds to the state before, and the call is the
    composition with that argument too."""
    torch = torch_cuda
    ps, N, T = "bc", 10, 8
    h, ctl, states = rollout_batch(torch, fx, ps, N, T)
    g0 = torch.zeros_like(states)
    g0[5:, :, N - 1, 12:15] = 1.0  # a tip loss on the second half
    whole = g0.clone()
    out_w = h.simulate_vjp(ctl, states, whole)
    half = g0[4:].clone()
    out_h = h.simulate_vjp(ctl[:, 4:].contiguous(), states[4:].contiguous(), half, prev_init=states[3].contiguous())
    assert torch.equal(out_h["g_ctl"], out_w["g_ctl"][:, 4:]) and torch.equal(half[1:], whole[5:])
    ref = composition(torch, h, ctl[:, 4:].contiguous(), states[4:].contiguous(), g0[4:].clone(), prev_init=states[3].contiguous())
    assert torch.equal(out_h["g_prev_init"], ref["g_prev_init"]) and torch.equal(half, ref["g_states"])
    assert torch.count_nonzero(out_h["g_prev_init"][:, :, 12:]) == 0 and torch.count_nonzero(out_h["g_prev_init"]) > 0


def test_nonfinite_rod_is_ordinary_input(torch_cuda, fx):
    """One NaN state value - in a slot the equations read (n of a grid point) and in one they do not (v of state_next,
    which is only checked): that rod gets status 2 and NaN gradients, every other rod is bit for bit the clean call, and the
    next call on the handle is unaffected.  The same through the rollout: the bad step and every earlier one."""
    torch = torch_cuda
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    clean = h.step_vjp(prev, cur, nxt, tens, g_next)
    for slot in (19, 7):
        bad_next = nxt.clone()
        bad_next[2, 4, slot] = float("nan")
        out = h.step_vjp(prev, cur, bad_next, tens, g_next)
        assert out["status"].tolist() == [0, 0, 2, 0, 0]
        for name in ("g_cur", "g_prev"):
            assert torch.isnan(out[name][2, :, :12]).all() and torch.count_nonzero(out[name][2, :, 12:]) == 0
        assert torch.isnan(out["g_tensions"][2]).all() and torch.isnan(out["g_bnd"][2]).all() and torch.isnan(out["resid"][2])
        keep = [0, 1, 3, 4]
        assert same_bits(torch, {k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in clean.items()})
        assert same_bits(torch, h.step_vjp(prev, cur, nxt, tens, g_next), clean)
    hr, ctl, states = rollout_batch(torch, fx, "bc", 10, 3)
    g0 = torch.zeros_like(states)
    g0[1:, :, 9, 12:15] = 1.0
    g_clean = g0.clone()
    o_clean = hr.simulate_vjp(ctl, states, g_clean)
    bad = states.clone()
    bad[2, 1, 3, 20] = float("nan")  # read as state_next of step 1, as state_cur's tail (not read) of step 2
    g_bad = g0.clone()
    o_bad = hr.simulate_vjp(ctl, bad, g_bad)
    assert o_bad["status"][1].tolist() == [2, 2, 0] and torch.isnan(o_bad["g_ctl"][1, :2]).all()
    assert torch.equal(o_bad["g_ctl"][1, 2], o_clean["g_ctl"][1, 2])
    for b in (0, 2):
        assert torch.equal(g_bad[:, b], g_clean[:, b]) and all(torch.equal(o_bad[n][b], o_clean[n][b]) for n in ("g_ctl", "g_bnd", "resid", "status"))


def test_refusals_leave_every_output_byte(torch_cuda, fx):
    """use_nn != 0 and RK4: KR_E_UNSUPPORTED with a message; a null required pointer, B < 1, T < 1, a bad dtype: KR_E_ARG;
    nothing is launched or written."""
    torch = torch_cuda
    import krod_native as kn
    h, keys, prev, cur, nxt, tens = step_batch(torch, fx, "plain", 10, "sine30", 3, 3)
    lib, B, N = h.lib, 3, 10
    g_next = torch.ones_like(nxt)
    outs = [torch.full((B, N, 28), 7.0, dtype=torch.float64, device=DEV) for _ in range(2)] + \
           [torch.full((B, 4), 7.0, dtype=torch.float64, device=DEV), torch.full((B, 19), 7.0, dtype=torch.float64, device=DEV),
            torch.full((B,), 7.0, dtype=torch.float64, device=DEV), torch.full((B,), 7, dtype=torch.int32, device=DEV)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def step(B=B, scheme=kn.KR_EULER, g=g_next, use_nn=0, dtype=kn.KR_F64, cur_=cur):
        return lib.kr_step_vjp_batch(h._h, B, scheme, p(prev), p(cur_), p(nxt), p(tens), p(g), *[p(o) for o in outs], use_nn, dtype, None)
    for kw, want, word in ((dict(use_nn=1), kn.KR_E_UNSUPPORTED, b"MLP"), (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"RK4"),
                           (dict(g=None), kn.KR_E_ARG, b"null"), (dict(cur_=None), kn.KR_E_ARG, b"null"), (dict(B=0), kn.KR_E_ARG, b"B"),
                           (dict(dtype=5), kn.KR_E_ARG, b"dtype")):
        rc = step(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    T = 2
    states = torch.zeros((T + 1, B, N, 28), dtype=torch.float64, device=DEV)
    ctl = torch.zeros((B, T, 4), dtype=torch.float64, device=DEV)
    g_states = torch.full((T + 1, B, N, 28), 7.0, dtype=torch.float64, device=DEV)
    souts = [torch.full((B, N, 28), 7.0, dtype=torch.float64, device=DEV), torch.full((B, T, 4), 7.0, dtype=torch.float64, device=DEV),
             torch.full((B, 19), 7.0, dtype=torch.float64, device=DEV), torch.full((B, T), 7.0, dtype=torch.float64, device=DEV),
             torch.full((B, T), 7, dtype=torch.int32, device=DEV)]

    def sim(B=B, T=T, scheme=kn.KR_EULER, st=states, use_nn=0, dtype=kn.KR_F64):
        return lib.kr_simulate_vjp_batch(h._h, B, T, scheme, p(ctl), p(st), None, p(g_states), *[p(o) for o in souts], use_nn, dtype, None)
    for kw, want, word in ((dict(use_nn=1), kn.KR_E_UNSUPPORTED, b"MLP"), (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"RK4"),
                           (dict(st=None), kn.KR_E_ARG, b"null"), (dict(T=0), kn.KR_E_ARG, b"T < 1"), (dict(B=0), kn.KR_E_ARG, b"B"),
                           (dict(dtype=-1), kn.KR_E_ARG, b"dtype")):
        rc = sim(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    torch.cuda.synchronize()
    for o in outs + souts + [g_states]:
        assert bool((o == 7).all())
    with pytest.raises(kn.KrError, match="ring"):  # the Python surface names the ring
        h.simulate_vjp(ctl, states[:2], g_states[:2])


def test_simulate_tips_backward_is_the_direct_call(torch_cuda, fx):
    """simulate_tips(...).sum().backward() fills ctl.grad with the g_ctl of kr_simulate_vjp_batch for a unit tip cotangent;
    rollout_grad with g_tips returns the same."""
    torch = torch_cuda
    import krod_grad as kg
    ps, N, T = "plain", 33, 3
    r = robot_for(ps, N)
    h, ctl, states = rollout_batch(torch, fx, ps, N, T)
    g = torch.zeros_like(states)
    g[1:, :, N - 1, 12:15] = 1.0
    direct = h.simulate_vjp(ctl, states, g)
    leaf = ctl.clone().requires_grad_(True)
    tips = kg.simulate_tips(r, leaf)
    assert tips.shape == (3, T, 3) and torch.equal(tips.detach(), states[1:, :, N - 1, 12:15].permute(1, 0, 2))
    tips.sum().backward()
    assert torch.equal(leaf.grad, direct["g_ctl"])
    res = kg.rollout_grad(r, ctl, states, g_tips=np.ones((3, T, 3)))
    assert np.array_equal(res["ctl"], direct["g_ctl"].cpu().numpy()) and np.array_equal(res["states"], g.cpu().numpy())
    assert res["boundary"].shape == (3, 19) and (res["status"] == 0).all()
