"""The step adjoint with the residual MLP on (kr_step_vjp_nn_batch, kr_simulate_vjp_nn_batch, krod_grad.rollout_grad_nn /
simulate_tips_nn) on the MI355X against central finite differences of the oracle's own step and rollout with the network
in the sweep (fixture step_adjoint_nn.npz, written by tests/golden/make_golden_step_adjoint_nn.py from
cosserat_oracle.residual_euler(..., mlp) + newton_shoot, solved to 1e-15).

The rule is the parent's (tests/test_gpu_step_adjoint.py): every finite difference exists at H and 2 H, a block's tolerance
is ten times their disagreement plus step_adjoint_cases.fd_floor, blocks are compared one by one, and every figure is
printed before it is asserted.  Forward states are produced on the device with use_nn and tol = 1e-12, status 0 asserted,
and held within 1e-9 of the oracle's.  Weight gradients are checked in two stages: the rows (x_j, c_j) the fp64 call emits
go through an fp64 NumPy backward pass and are held against the fixture's directional and corner differences by the same
rule (a block per layer); the device's fp32 backward over the same rows is held to that NumPy pass at relative L2 < 2e-5 per
layer, the bound tests/test_gpu_train.py holds kr_mlp_backward to.
Measured (2253 compared blocks): largest error / tolerance 0.45; resid <= 1.2e-15; fp32 against fp64 weight backward
<= 1.2e-7 relative L2 per layer."""
import ctypes as C

import numpy as np
import pytest

import nn_adjoint_cases as nc
import step_adjoint_cases as sc
from conftest import load_golden
from gpu_helpers import inject, make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESID_MAX = 1e-10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return load_golden("step_adjoint_nn")


def fixture_mlp(fx, net):
    import cosserat_oracle as orc
    n = len(nc.NETWORKS[net][0]) + 1
    return orc.Mlp([fx[f"net_{net}_W{k}"] for k in range(n)], [fx[f"net_{net}_b{k}"] for k in range(n)],
                   [int(a) for a in fx[f"net_{net}_acts"]], False)


_robots = {}


def robot_for(ps, N, mlp, tag):
    if (ps, N, tag) not in _robots:
        P = sc.params(ps, N)
        r = make_robot("noair" if ps == "noair" else None, N)
        for k in ("Bse", "Bbt", "F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
            setattr(r, k, np.array(getattr(P, k), dtype=np.float64))
        r.compute_intermediate_terms()
        if mlp is not None:
            inject(r, mlp)
        _robots[(ps, N, tag)] = r
    return _robots[(ps, N, tag)]


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype or torch.float64).contiguous()


def step_batch(torch, fx, ps, N, state, net, rods, B):
    """B rods from the fixture's (rod b: fixture rod b % rods, tensions scaled by 1 + 0.003 (b // rods)); the forward step
    runs here with the network on, tol 1e-12."""
    mlp = fixture_mlp(fx, net)
    h = robot_for(ps, N, mlp, net)._native()
    keys = [nc.nn_case_key(ps, N, state, net) + f"_r{b % rods}_" for b in range(B)]
    prev = _dev(torch, np.stack([fx[k + "prev"] for k in keys]))
    cur = prev if state == "straight" else _dev(torch, np.stack([fx[k + "cur"] for k in keys]))
    tens = _dev(torch, np.stack([fx[k + "tens"] * (1 + 0.003 * (b // rods)) for b, k in enumerate(keys)]))
    nxt = torch.zeros_like(prev)
    G = torch.zeros((B, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((B,), dtype=torch.int32, device=DEV)
    h.step(prev, cur, nxt, G, tens, tol=1e-12, status=status, use_nn=True)
    assert (status == 0).all(), status
    for b in range(min(rods, B)):  # (the device's step is the oracle's)
        dist = np.max(np.abs(nxt[b].cpu().numpy() - fx[keys[b] + "next"]))
        assert dist < 1e-9, (b, dist)
    return h, mlp, keys, prev, cur, nxt, tens


NAMES = ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status", "nn_x", "nn_g")


def got_vector(out, b):
    return np.concatenate([out["g_cur"][b, :, :12].cpu().numpy().ravel(), out["g_prev"][b, :, :12].cpu().numpy().ravel(),
                           out["g_tensions"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy()])


def same_bits(torch, a, b, names=NAMES):
    return all(torch.equal(a[k], b[k]) for k in names)


def check_weight_blocks(tag, mlp, X, Cc, a, b, floor):
    """fp64 NumPy backward over the rows against the fixture's directional / corner differences, a block per layer"""
    gw = nc.weight_directions(mlp) @ nc.mlp_backward_rows(mlp, X, Cc)
    for lo in range(0, len(gw), 6):
        err, tol = np.max(np.abs(gw[lo:lo + 6] - a[lo:lo + 6])), sc.block_tol(a[lo:lo + 6], b[lo:lo + 6], floor)
        print(f"  {tag} weights layer {lo // 6} err {err:.3e} tol {tol:.3e} size {np.max(np.abs(a[lo:lo + 6])):.3e}")
        assert err <= tol, (tag, lo, err, tol)


STEP_RUNS = [(ps, N, rods, state, net, 5) for ps, N, rods, state, net in nc.NN_STEP_CASES] + \
            [(ps, N, rods, state, net, B) for ps, N, rods, state, net in (("bc", 10, 3, "sine30", "elu64x64"), ("plain", 2, 3, "sine30", "tanh17"),
                                                                       ("bc", 10, 3, "sine30", "elu512"))
             for B in (1, 70)]


@pytest.mark.parametrize("ps,N,rods,state,net,B", STEP_RUNS)
def test_step_vjp_nn_against_the_oracle(torch_cuda, fx, ps, N, rods, state, net, B):
    """Every output block of the oracle's rods against the finite differences for the three cotangents; the weight rows
    through the fp64 NumPy backward against the fixture's weight differences; structural zeros exact; resid; every rod bit
    identical to its own B = 1 call.  The forward step needed neither a raised maxit nor single shooting to reach 1e-12."""
    torch = torch_cuda
    h, mlp, keys, prev, cur, nxt, tens = step_batch(torch, fx, ps, N, state, net, rods, B)
    for c in range(3):
        gbar = np.stack([fx[k + "gbar"][c] * (1 + 0.1 * (b // rods)) for b, k in enumerate(keys)])
        g_next = _dev(torch, gbar)
        out = h.step_vjp_nn(prev, cur, nxt, tens, g_next)
        assert (out["status"] == 0).all()
        resid = out["resid"].cpu().numpy()
        print(f"{ps} N={N} {state} {net} B={B} cotangent {c}: resid max {resid.max():.2e}")
        assert np.all(resid <= RESID_MAX)
        for name in ("g_cur", "g_prev"):
            assert torch.count_nonzero(out[name][:, :, 12:]) == 0, name
        assert torch.count_nonzero(out["nn_x"][:, :, 28:]) == 0 and torch.count_nonzero(out["nn_g"][:, :, 25:]) == 0
        for b in range(min(rods, B)):
            floor = sc.fd_floor(gbar[b], nxt[b].cpu().numpy())
            for name, err, tol, size in sc.block_report(got_vector(out, b), fx[keys[b] + "fd_h"][c], fx[keys[b] + "fd_2h"][c], N, floor):
                print(f"  rod {b} {name:14s} err {err:.3e} tol {tol:.3e} size {size:.3e}")
                assert err <= tol, (ps, N, state, net, c, b, name, err, tol)
            check_weight_blocks(f"rod {b}", mlp, out["nn_x"][b, :, :28].cpu().numpy(), out["nn_g"][b, :, :25].cpu().numpy(),
                                fx[keys[b] + "wfd_h"][:, c], fx[keys[b] + "wfd_2h"][:, c], floor)
        if c == 2:  # the pass-through: v, u of the last point go to state_cur unchanged, nothing else moves
            assert torch.equal(out["g_cur"][:, N - 1, 6:12], g_next[:, N - 1, 6:12])
            assert torch.count_nonzero(out["g_cur"][:, :N - 1]) == 0 and torch.count_nonzero(out["g_prev"]) == 0
            assert torch.count_nonzero(out["g_tensions"]) == 0 and torch.count_nonzero(out["g_bnd"]) == 0
            assert torch.count_nonzero(out["nn_g"]) == 0
        for b in range(B):
            one = h.step_vjp_nn(prev[b:b + 1], cur[b:b + 1], nxt[b:b + 1], tens[b:b + 1], g_next[b:b + 1])
            assert same_bits(torch, one, {k: v[b:b + 1] for k, v in out.items()}), (c, b)


def test_step_vjp_nn_f32_is_the_f64_call_rounded(torch_cuda, fx):
    """dtype = KR_F32 is the element type only: the call equals the fp64 call on the upcast inputs, rounded to float - the
    weight rows included."""
    torch = torch_cuda
    h, mlp, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", "elu64x64", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    f32 = [t.float().contiguous() for t in (prev, cur, nxt, tens, g_next)]
    lo = h.step_vjp_nn(*f32)
    hi = h.step_vjp_nn(*[t.double().contiguous() for t in f32])
    assert (lo["status"] == 0).all() and lo["g_cur"].dtype == torch.float32 and lo["nn_x"].dtype == torch.float32
    for k in ("g_cur", "g_prev", "g_tensions", "g_bnd", "nn_x", "nn_g"):
        assert torch.equal(lo[k], hi[k].float()), k
    assert torch.equal(lo["resid"], hi["resid"]) and torch.equal(lo["status"], hi["status"])


def test_zero_network_gives_the_physics_adjoint(torch_cuda, fx):
    """A network of zero weights and biases: Jn = 0 exactly, every product with it is a zero, and adding a zero changes no
    value - g_cur, g_prev, g_tensions, g_bnd, resid and status EQUAL those of kr_step_vjp_batch on the same states (value for
    value; only the sign of a zero may differ, which torch.equal does not see).  The rows hold x and c_j, with
    c_j[19:25] = g_z[j] exactly."""
    torch = torch_cuda
    import cosserat_oracle as orc
    zero = orc.Mlp([np.zeros((64, 28), np.float32), np.zeros((64, 64), np.float32), np.zeros((25, 64), np.float32)],
                   [np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(25, np.float32)], [orc.ACT_ELU, orc.ACT_ELU, orc.ACT_NONE], False)
    pfx = load_golden("step_adjoint")
    ps, N = "bc", 10
    h = robot_for(ps, N, zero, "zero")._native()
    keys = [sc.case_key(ps, N, "sine30") + f"_r{b % 3}_" for b in range(5)]
    prev, cur = (_dev(torch, np.stack([pfx[k + n] for k in keys])) for n in ("prev", "cur"))
    tens = _dev(torch, np.stack([pfx[k + "tens"] for k in keys]))
    nxt = torch.zeros_like(prev)
    G = torch.zeros((5, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((5,), dtype=torch.int32, device=DEV)
    h.step(prev, cur, nxt, G, tens, tol=1e-12, status=status, use_nn=True)
    assert (status == 0).all()
    for c in range(3):
        g_next = _dev(torch, np.stack([pfx[k + "gbar"][c] for k in keys]))
        a, b = h.step_vjp_nn(prev, cur, nxt, tens, g_next), h.step_vjp(prev, cur, nxt, tens, g_next)
        for n in ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid"):
            print(f"zero network, cotangent {c}, {n}: largest difference {float((a[n] - b[n]).abs().max()):.3e}")
        assert same_bits(torch, a, b, ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status")), c
        assert torch.equal(a["nn_g"][:, :, 19:25], g_next[:, :N - 1, 6:12])
        y = nxt[:, :N - 1][:, :, torch.as_tensor(sc.ROW_TO_SLOT[:19], device=DEV)]
        assert torch.equal(a["nn_x"][:, :, :19], y)


def composition(torch, h, ctl, states, g):
    """kr_simulate_vjp_nn_batch as the header defines it: the loop of step adjoints."""
    B, T = ctl.shape[0], ctl.shape[1]
    N = states.shape[2]
    g = g.clone()
    g_ctl = torch.zeros((B, T, 4), dtype=ctl.dtype, device=DEV)
    g_bnd = torch.zeros((B, 19), dtype=ctl.dtype, device=DEV)
    resid = torch.zeros((B, T), dtype=torch.float64, device=DEV)
    status = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    nn_x = torch.zeros((T, B, N - 1, 32), dtype=ctl.dtype, device=DEV)
    nn_g = torch.zeros_like(nn_x)
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else states[0]
        o = h.step_vjp_nn(prev, states[t], states[t + 1], ctl[:, t].contiguous(), g[t + 1])
        g[t] += o["g_cur"]
        g[max(t - 1, 0)] += o["g_prev"]
        g_ctl[:, t] = o["g_tensions"]
        g_bnd += o["g_bnd"]
        resid[:, t], status[:, t] = o["resid"], o["status"]
        nn_x[t], nn_g[t] = o["nn_x"], o["nn_g"]
    return dict(g_states=g, g_ctl=g_ctl, g_bnd=g_bnd, resid=resid, status=status, nn_x=nn_x, nn_g=nn_g)


def rollout_batch(torch, fx, ps, N, T, net, B=3):
    import krod_grad as kg
    mlp = fixture_mlp(fx, net)
    r = robot_for(ps, N, mlp, net)
    h = r._native()
    ctl0 = fx[f"roll_{ps}_N{N}_T{T}_{net}_ctl"]
    ctl = _dev(torch, np.stack([ctl0 * (1 + 0.01 * b) for b in range(B)]))
    states, tip, status = kg.forward_states(h, ctl, tol=1e-12, use_nn=True)
    assert (status == 0).all()
    return r, h, mlp, ctl, states


def torch_params(torch, mlp):
    ps = []
    for W, b in zip(mlp.weights, mlp.biases):
        ps += [torch.as_tensor(W, device=DEV), torch.as_tensor(b, device=DEV)]
    return ps


@pytest.mark.parametrize("ps,N,T,net", nc.NN_ROLLOUT_CASES)
def test_simulate_vjp_nn_against_the_oracle_and_the_step_calls(torch_cuda, fx, ps, N, T, net):
    """g_ctl (a block per step), g_bnd (six blocks), the chosen entries of g_states[0] and the weight gradient (a block per
    layer) of rod 0 against the finite differences of the oracle's rollout, for both cotangents; the call is bit for bit
    the loop of kr_step_vjp_nn_batch calls, rows included; rollout_grad_nn's fp32 weight gradient is the fp64 NumPy backward
    over the same rows to 2e-5 per layer, and two identical calls give identical bits."""
    torch = torch_cuda
    import krod_grad as kg
    r, h, mlp, ctl, states = rollout_batch(torch, fx, ps, N, T, net)
    k = f"roll_{ps}_N{N}_T{T}_{net}_"
    ent = sc.rollout_state0_entries(N)
    for c in range(2):
        gbar = fx[k + "gbar"][c]
        g0 = _dev(torch, np.repeat(gbar[:, None], ctl.shape[0], axis=1))
        g = g0.clone()
        out = h.simulate_vjp_nn(ctl, states, g)
        assert (out["status"] == 0).all() and float(out["resid"].max()) <= RESID_MAX
        ref = composition(torch, h, ctl, states, g0)
        assert torch.equal(g, ref["g_states"]) and all(torch.equal(out[n], ref[n]) for n in ("g_ctl", "g_bnd", "resid", "status", "nn_x", "nn_g"))
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
        X = out["nn_x"][:, 0, :, :28].reshape(-1, 28).cpu().numpy()
        Cc = out["nn_g"][:, 0, :, :25].reshape(-1, 25).cpu().numpy()
        check_weight_blocks(f"T={T} cotangent {c}", mlp, X, Cc, fx[k + "wfd_h"][:, c], fx[k + "wfd_2h"][:, c], floor)
        # the device's fp32 backward over ALL rods' rows against the fp64 NumPy backward over the same rows
        params = torch_params(torch, mlp)
        res = kg.rollout_grad_nn(r, ctl, states, g_states=g0, params=params)
        again = kg.rollout_grad_nn(r, ctl, states, g_states=g0, params=params)
        assert np.array_equal(res["ctl"], out["g_ctl"].cpu().numpy()) and np.array_equal(res["states"], g.cpu().numpy())
        want = nc.mlp_backward_rows(mlp, out["nn_x"][..., :28].reshape(-1, 28).cpu().numpy(), out["nn_g"][..., :25].reshape(-1, 25).cpu().numpy())
        o = 0
        for li in range(len(mlp.weights)):
            n = mlp.weights[li].size + mlp.biases[li].size
            gotw = np.concatenate([res["params"][2 * li].ravel(), res["params"][2 * li + 1]]).astype(np.float64)
            rel = np.linalg.norm(gotw - want[o:o + n]) / np.linalg.norm(want[o:o + n])
            print(f"  T={T} cotangent {c} layer {li}: fp32 device backward vs fp64 NumPy, relative L2 {rel:.2e}")
            assert rel < 2e-5, (li, rel)
            assert all(np.array_equal(x, y) for x, y in zip(res["params"], again["params"]))
            o += n


def test_rollout_forms_share_one_workspace(torch_cuda, fx):
    """The rollout calls carve one workspace: a typed head, then the tail the form asks for (the network's rows and
    Jacobians, or the step's parameter gradient).  On one handle with a network set (N = 9, T = 3, fp64): simulate_vjp_nn at
    B = 5, then simulate_vjp(need_par=True) with the MLP off at B = 2 - the same allocation at another carving - then the
    first call again.  The third call is the first in every output bit, the second is the same call on a fresh handle."""
    torch = torch_cuda
    import krod_grad as kg
    import krod_native as kn
    N, T = 9, 3
    r = robot_for("bc", N, fixture_mlp(fx, "elu64x64"), "elu64x64")
    h = r._native()
    ctl0 = fx["roll_bc_N10_T3_elu64x64_ctl"]
    ctl5 = _dev(torch, np.stack([ctl0 * (1 + 0.01 * b) for b in range(5)]))
    ctl2 = ctl5[:2].contiguous()
    st5, _, status5 = kg.forward_states(h, ctl5, tol=1e-12, use_nn=True)
    st2, _, status2 = kg.forward_states(h, ctl2, tol=1e-12)
    assert (status5 == 0).all() and (status2 == 0).all()
    rng = np.random.default_rng(9)
    g5, g2 = _dev(torch, rng.standard_normal(tuple(st5.shape))), _dev(torch, rng.standard_normal(tuple(st2.shape)))

    def call(vjp, ctl, states, g0, **kw):
        g = g0.clone()
        out = vjp(ctl, states, g, **kw)
        assert (out["status"] == 0).all()
        return dict(out, g_states=g)

    first = call(h.simulate_vjp_nn, ctl5, st5, g5)
    par = call(h.simulate_vjp, ctl2, st2, g2, need_par=True)
    third = call(h.simulate_vjp_nn, ctl5, st5, g5)
    fresh = kn.Handle(r._params(), r.device)
    alone = call(fresh.simulate_vjp, ctl2, st2, g2, need_par=True)
    fresh.close()
    for n in ("g_states", "g_ctl", "g_bnd", "resid", "status", "nn_x", "nn_g"):
        assert torch.equal(third[n], first[n]), n
    for n in ("g_states", "g_ctl", "g_bnd", "g_par", "resid", "status"):
        assert torch.equal(par[n], alone[n]), n


def test_simulate_tips_nn_backward_is_the_direct_call(torch_cuda, fx):
    """simulate_tips_nn(...).sum().backward() fills ctl.grad and every p.grad with what rollout_grad_nn returns for a unit
    tip cotangent."""
    torch = torch_cuda
    import krod_grad as kg
    ps, N, T, net = "bc", 10, 3, "elu64x64"
    r, h, mlp, ctl, states = rollout_batch(torch, fx, ps, N, T, net)
    params = [p.clone().requires_grad_(True) for p in torch_params(torch, mlp)]
    leaf = ctl.clone().requires_grad_(True)
    tips = kg.simulate_tips_nn(r, leaf, params)
    assert tips.shape == (3, T, 3) and torch.equal(tips.detach(), states[1:, :, N - 1, 12:15].permute(1, 0, 2))
    tips.sum().backward()
    res = kg.rollout_grad_nn(r, ctl, states, g_tips=np.ones((3, T, 3)), params=[p.detach() for p in params])
    assert np.array_equal(leaf.grad.cpu().numpy(), res["ctl"]) and (res["status"] == 0).all()
    for p, gw in zip(params, res["params"]):
        assert p.grad is not None and np.array_equal(p.grad.cpu().numpy(), gw) and np.any(gw != 0)


def test_robot_keeps_its_own_weights_across_simulate_tips_nn(torch_cuda, fx):
    """simulate_tips_nn pushes OTHER weights than the robot's into the shared handle, in forward and again in backward; a
    plain use of the robot in between and afterwards must find the robot's own network, not the pushed one."""
    torch = torch_cuda
    import krod_grad as kg
    ps, N, T, net = "bc", 10, 3, "elu64x64"
    r, h, mlp, ctl, states = rollout_batch(torch, fx, ps, N, T, net)
    params = [(1.05 * p).clone().requires_grad_(True) for p in torch_params(torch, mlp)]
    tips = kg.simulate_tips_nn(r, ctl.clone().requires_grad_(True), params)
    assert not torch.equal(tips.detach(), states[1:, :, N - 1, 12:15].permute(1, 0, 2))  # (the pushed weights were used)
    assert r._mlp_key is None
    between = kg.forward_states(r._native(), ctl, tol=1e-12, use_nn=True)[0]  # (an evaluation rollout between forward and backward)
    assert torch.equal(between, states) and r._mlp_key is not None
    tips.sum().backward()
    assert r._mlp_key is None and all(p.grad is not None for p in params)
    after = kg.forward_states(r._native(), ctl, tol=1e-12, use_nn=True)[0]
    assert torch.equal(after, states)


@pytest.mark.parametrize("net", ["elu64x64", "elu512"])
def test_weight_grads_are_bit_reproducible_at_many_slabs(torch_cuda, fx, net, monkeypatch):
    """38 016 rows (T = 4, B = 96, N = 100): the fused backward leaves more than a hundred per-workgroup slabs of partial
    gradients, so the order of their sum matters - repeated calls give identical bits (option "mlp_grad_ordered": a fixed
    order, no atomics), in one chunk and in four, the option is restored afterwards, and the sum is the fp64 NumPy backward
    over the same rows to 2e-5 relative L2 per layer (the bound tests/test_gpu_train.py holds kr_mlp_backward to).  A network
    the fused kernels do not serve is refused, not summed with atomics."""
    torch = torch_cuda
    import krod_grad as kg
    import krod_native as kn
    mlp = fixture_mlp(fx, net)
    h = make_robot(None, 10)._native()
    rng = np.random.default_rng(5)
    T, B, M = 4, 96, 99
    x = np.zeros((T, B, M, 32))
    g = np.zeros((T, B, M, 32))
    x[..., :28] = rng.normal(size=(T, B, M, 28))
    g[..., :25] = rng.normal(size=(T, B, M, 25))
    nn_x, nn_g = _dev(torch, x), _dev(torch, g)
    p32 = torch_params(torch, mlp)
    acts = [int(a) for a in mlp.acts]
    runs = [kg.weight_grads(h, p32, acts, nn_x, nn_g) for _ in range(3)]
    assert all(torch.equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))
    assert h.get_option("mlp_grad_ordered") == 0 and h.get_option("mlp_grad_accumulate") == 0
    monkeypatch.setattr(kg, "ROWS_PER_CHUNK", B * M)  # one step per chunk: four kr_mlp_backward calls adding up
    chunked = [kg.weight_grads(h, p32, acts, nn_x, nn_g) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*chunked))
    # fp32 rows, as the device sees them, through the fp64 NumPy backward
    want = nc.mlp_backward_rows(mlp, x[..., :28].reshape(-1, 28).astype(np.float32), g[..., :25].reshape(-1, 25).astype(np.float32))
    for tag, got in (("one chunk", runs[0]), ("four chunks", chunked[0])):
        o = 0
        for li in range(len(mlp.weights)):
            n = mlp.weights[li].size + mlp.biases[li].size
            gotw = np.concatenate([got[2 * li].cpu().numpy().ravel(), got[2 * li + 1].cpu().numpy()]).astype(np.float64)
            rel = np.linalg.norm(gotw - want[o:o + n]) / np.linalg.norm(want[o:o + n])
            print(f"{net} {tag} layer {li}: relative L2 {rel:.2e}")
            assert rel < 2e-5, (tag, li, rel)
            o += n
    if len(acts) == 3:
        with pytest.raises(kn.KrError, match="mlp_grad_ordered"):
            kg.weight_grads(h, p32, [kn.ACT_ELU, kn.ACT_TANH, kn.ACT_NONE], nn_x, nn_g)
        assert h.get_option("mlp_grad_ordered") == 0


def test_nonfinite_rod_is_ordinary_input(torch_cuda, fx):
    """One NaN state value: that rod gets status 2, NaN gradients and NaN weight cotangents, every other rod is bit for bit
    the clean call, and the next call on the handle is unaffected."""
    torch = torch_cuda
    h, mlp, keys, prev, cur, nxt, tens = step_batch(torch, fx, "bc", 10, "sine30", "elu64x64", 3, 5)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    clean = h.step_vjp_nn(prev, cur, nxt, tens, g_next)
    for slot in (19, 7):
        bad_next = nxt.clone()
        bad_next[2, 4, slot] = float("nan")
        out = h.step_vjp_nn(prev, cur, bad_next, tens, g_next)
        assert out["status"].tolist() == [0, 0, 2, 0, 0]
        for name in ("g_cur", "g_prev"):
            assert torch.isnan(out[name][2, :, :12]).all() and torch.count_nonzero(out[name][2, :, 12:]) == 0
        assert torch.isnan(out["g_tensions"][2]).all() and torch.isnan(out["g_bnd"][2]).all() and torch.isnan(out["resid"][2])
        assert torch.isnan(out["nn_g"][2, :, :25]).all() and torch.count_nonzero(out["nn_g"][2, :, 25:]) == 0
        keep = [0, 1, 3, 4]
        assert same_bits(torch, {k: v[keep] for k, v in out.items()}, {k: v[keep] for k, v in clean.items()})
        assert same_bits(torch, h.step_vjp_nn(prev, cur, nxt, tens, g_next), clean)


def test_refusals_leave_every_output_byte(torch_cuda, fx):
    """No network: KR_E_STATE.  RK4, nn_input_history = 1, a shape outside the Jacobian kernel's, an activation on the last
    layer: KR_E_UNSUPPORTED.  A null required pointer, B < 1, T < 1, a bad dtype: KR_E_ARG.  Each with a message, nothing
    launched or written."""
    torch = torch_cuda
    import cosserat_oracle as orc
    import krod_native as kn
    B, N, T = 3, 10, 2
    new = lambda *s, v=7.0, dt=torch.float64: torch.full(s, v, dtype=dt, device=DEV)
    st = torch.zeros((B, N, 28), dtype=torch.float64, device=DEV)
    tens = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
    outs = [new(B, N, 28), new(B, N, 28), new(B, 4), new(B, 19), new(B), new(B, v=7, dt=torch.int32), new(B, N - 1, 32), new(B, N - 1, 32)]
    states = torch.zeros((T + 1, B, N, 28), dtype=torch.float64, device=DEV)
    ctl = torch.zeros((B, T, 4), dtype=torch.float64, device=DEV)
    g_states = new(T + 1, B, N, 28)
    souts = [new(B, N, 28), new(B, T, 4), new(B, 19), new(B, T), new(B, T, v=7, dt=torch.int32), new(T, B, N - 1, 32), new(T, B, N - 1, 32)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def calls(h):
        lib = h.lib

        def step(B=B, scheme=kn.KR_EULER, g=st, dtype=kn.KR_F64, cur_=st):
            return lib.kr_step_vjp_nn_batch(h._h, B, scheme, p(st), p(cur_), p(st), p(tens), p(g), *[p(o) for o in outs], dtype, None)

        def sim(B=B, T=T, scheme=kn.KR_EULER, s_=states, dtype=kn.KR_F64):
            return lib.kr_simulate_vjp_nn_batch(h._h, B, T, scheme, p(ctl), p(s_), None, p(g_states), *[p(o) for o in souts], dtype, None)
        return lib, step, sim
    rng = np.random.default_rng(0)

    def net(sizes, acts):
        return ([rng.normal(size=(sizes[k + 1], sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)],
                [np.zeros(sizes[k + 1], np.float32) for k in range(len(sizes) - 1)], acts)
    E, NONE = orc.ACT_ELU, orc.ACT_NONE
    h = make_robot(None, N)._native()
    lib, step, sim = calls(h)
    for fn in (step, sim):
        assert fn() == kn.KR_E_STATE and b"no MLP" in lib.kr_last_error()
    for sizes, acts, word in (((28, 600, 25), (E, NONE), b"512"), ((28, 100, 64, 25), (E, E, NONE), b"64"), ((28, 16, 25), (E, E), b"last layer")):
        h.set_mlp(*net(sizes, acts))
        for fn in (step, sim):
            assert fn() == kn.KR_E_UNSUPPORTED and word in lib.kr_last_error(), (sizes, lib.kr_last_error())
    h.set_mlp(*net((28, 16, 25), (E, NONE)))
    for fn in (step, sim):
        assert fn(scheme=kn.KR_RK4) == kn.KR_E_UNSUPPORTED and b"RK4" in lib.kr_last_error()
        assert fn(B=0) == kn.KR_E_ARG and b"B" in lib.kr_last_error()
        assert fn(dtype=5) == kn.KR_E_ARG and b"dtype" in lib.kr_last_error()
    assert step(g=None) == kn.KR_E_ARG and b"null" in lib.kr_last_error()
    assert step(cur_=None) == kn.KR_E_ARG and b"null" in lib.kr_last_error()
    assert sim(s_=None) == kn.KR_E_ARG and b"null" in lib.kr_last_error()
    assert sim(T=0) == kn.KR_E_ARG and b"T < 1" in lib.kr_last_error()
    rh = make_robot(None, N)
    rh.nn_input_history = True
    hh = rh._native()
    hh.set_mlp(*net((53, 16, 25), (E, NONE)))
    lib, step, sim = calls(hh)
    for fn in (step, sim):
        assert fn() == kn.KR_E_UNSUPPORTED and b"nn_input_history" in lib.kr_last_error()
    torch.cuda.synchronize()
    for o in outs + souts + [g_states]:
        assert bool((o == 7).all())
    with pytest.raises(kn.KrError, match="ring"):
        h.simulate_vjp_nn(ctl, states[:2], g_states[:2])
    # the physics-only calls keep refusing a request for the network
    assert lib.kr_step_vjp_batch(h._h, B, kn.KR_EULER, p(st), p(st), p(st), p(tens), p(st), *[p(o) for o in outs[:6]], 1, kn.KR_F64,
                                 None) == kn.KR_E_UNSUPPORTED
