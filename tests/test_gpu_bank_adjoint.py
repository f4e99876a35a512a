"""The step adjoint of a heterogeneous batch with the MLP on, on the MI355X (kr_step_vjp_bank_batch,
kr_simulate_vjp_bank_batch, krod_grad.rollout_grad_bank / simulate_tips_bank): rod b with row b of a parameter table AND
network net_of_rod[b] of a bank, the boundary gradient per step.

Steps and rollouts are held to bank_adjoint.npz (tests/golden/make_golden_bank_adjoint.py: B = 5 rods at N = 9, T = 4, three
rows, K = 3 networks with net_of_rod = [1, 0, 1, 1, 0], once per kernel family of the input Jacobian), every block under the
tolerance RECORDED in the file; mixed bank calls at N = 10 are held, rod by rod, to the existing step_adjoint_nn.npz under that
fixture's rule.  The calls run on a carrier handle whose own parameters belong to no row and whose own network to no bank.
The stored states are the oracle's (the file's), so that the adjoint is taken where the differences were; the forward bank call
of simulate_tips_bank is held to them within 1e-9.  Every figure is printed before it is asserted.
Weight gradients are checked as in tests/test_gpu_nn_adjoint.py: the rows (x_j, c_j) of a network's rods go through the fp64
NumPy backward pass and are held to the fixture's directional differences, a block per layer.
The elu512 case (one hidden layer over eight chunks, B = 3, K = 2, N = 10) against kr_step_vjp_nn_batch on handles set to each
network is held under the fixture rule's tolerance; whether it is bit for bit is printed, not promised.
Measured (MI355X, this file): largest error / tolerance 0.44 over the step blocks, 0.21 over the rollout blocks, 0.45 over the
mixed calls held to step_adjoint_nn.npz; resid <= 1e-9 asserted; the elu512 bank call came out bit for bit the handle calls in
every output of every rod; fp32 against fp64 weight backward <= 1.2e-7 relative L2."""
import ctypes as C

import numpy as np
import pytest

import bank_adjoint_cases as bc
import nn_adjoint_cases as nc
import step_adjoint_cases as sc
import table_adjoint_cases as tc
from conftest import load_golden
from gpu_helpers import inject, make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_NAMES = ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status", "nn_x", "nn_g")
RESID_MAX = 1e-9
N, B, T, K = bc.N_FIX, bc.B_FIX, bc.T_FIX, bc.K_FIX
NETS = list(bc.NET_OF_ROD)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fb():
    return load_golden("bank_adjoint")


@pytest.fixture(scope="module")
def fn():
    return load_golden("step_adjoint_nn")


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype or torch.float64).contiguous()


def same_bits(torch, a, b, names=STEP_NAMES):
    return all(torch.equal(a[k], b[k]) for k in names)


def pick(out, idx, names=STEP_NAMES):
    return {k: out[k][idx] for k in names}


def as_network(m):
    return (list(m.weights), list(m.biases), list(m.acts))


def as_params(torch, m):
    """nn.Linear order W1, b1, W2, b2, ... as float32 host tensors"""
    out = []
    for W, b in zip(m.weights, m.biases):
        out += [torch.tensor(np.asarray(W, np.float32)), torch.tensor(np.asarray(b, np.float32))]
    return out


_carriers = {}


def carrier_for(n, family):
    """The robot whose handle carries a bank call: the `youngs` preset (E = 10 GPa, no row's) with a network of the family's
    shape and a seed of its own (no bank's): a kernel that read the handle's constants or the handle's network would miss"""
    if (n, family) not in _carriers:
        hidden, act, gain = nc.NETWORKS[family]
        r = make_robot("youngs", n)
        inject(r, nc.signed_mlp(hidden, act, gain, 99))
        _carriers[(n, family)] = r
    return _carriers[(n, family)]


_setups = {}


def setup(torch, fb, fam):
    """-> dict: the carrier's handle, the table of the five rods' rows, the bank of the family's three networks, and the
    fixture's rollout on the device (the oracle's states)"""
    if fam not in _setups:
        nets = bc.fixture_networks(fb, fam)
        robots = [tc.robot_for(bc.SETS[bc.ROW_OF_ROD[b]], N) for b in range(B)]
        carrier = carrier_for(N, fam)
        hc = carrier._native()
        ks = [bc.key(fam, b) for b in range(B)]
        _setups[fam] = dict(nets=nets, robots=robots, carrier=carrier, hc=hc, ks=ks, table=hc.param_table([r._params() for r in robots]),
                            bank=hc.mlp_bank([as_network(m) for m in nets]),
                            ctl=_dev(torch, np.stack([fb[k + "ctl"] for k in ks])), bnd=_dev(torch, np.stack([fb[k + "bnd"] for k in ks])),
                            states=_dev(torch, np.stack([fb[k + "states"] for k in ks], axis=1)))
    return _setups[fam]


def got_vector(out, b):
    return np.concatenate([out["g_cur"][b, :, :12].cpu().numpy().ravel(), out["g_prev"][b, :, :12].cpu().numpy().ravel(),
                           out["g_tensions"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy()])


def step_args(s, t):
    st = s["states"]
    return (st[t - 1] if t > 0 else st[0], st[t], st[t + 1], s["ctl"][:, t].contiguous())


_worst = {}


@pytest.mark.parametrize("fam", bc.FAMILIES)
def test_step_bank_against_the_fixture(torch_cuda, fb, fam):
    """1. Both stored steps, three cotangents: every rod's g_cur, g_prev, g_tensions, g_bnd under the recorded tolerances, the
    weight blocks of each network with rods from the rows of ITS rods (rod order), structural zeros exact; rod b is bit for
    bit its own B = 1 call, and bit for bit the same rod in another place of another batch with another net_of_rod in which
    network 1 (or 0) does not occur at all."""
    torch = torch_cuda
    s = setup(torch, fb, fam)
    hc, table, bank, ks, nets, robots = s["hc"], s["table"], s["bank"], s["ks"], s["nets"], s["robots"]
    worst = {}
    for t in bc.STEP_TS:
        args = step_args(s, t)
        for c in range(3):
            g_next = _dev(torch, np.stack([fb[k + f"s{t}_gbar"][c] for k in ks]))
            out = hc.step_vjp_bank(table, bank, NETS, *args, g_next)
            assert (out["status"] == 0).all() and float(out["resid"].max()) <= RESID_MAX
            for name in ("g_cur", "g_prev"):
                assert torch.count_nonzero(out[name][:, :, 12:]) == 0, name
            assert torch.count_nonzero(out["nn_x"][:, :, 28:]) == 0 and torch.count_nonzero(out["nn_g"][:, :, 25:]) == 0
            for b, k in enumerate(ks):
                bc.step_check(f"{k} step {t} cot {c}", got_vector(out, b), fb[k + f"s{t}_fd_h"][c], fb[k + f"s{t}_tol"][c], worst)
            for kk in range(K):
                rods = bc.rods_of(kk)
                if not rods: continue
                gw = bc.weight_grad(nets[kk], out["nn_x"][rods][:, :, :28].cpu().numpy(), out["nn_g"][rods][:, :, :25].cpu().numpy())
                pre = f"{fam}_net{kk}_s{t}_"
                bc.w_check(f"{fam} net {kk} step {t} cot {c}", gw, fb[pre + "wfd_h"][c], fb[pre + "w_tol"][c], worst)
            if c != 0: continue
            for b in range(B):
                with hc.param_table([robots[b]._params()]) as t1:
                    one = hc.step_vjp_bank(t1, bank, [NETS[b]], *[a[b:b + 1].contiguous() for a in args], g_next[b:b + 1].contiguous())
                assert same_bits(torch, one, pick(out, slice(b, b + 1))), (t, b)
            for idx in ([4, 1, 4], [2, 0, 3, 0, 2, 3, 0]):  # network 0 alone; network 1 alone, past one workgroup of four rods
                with hc.param_table([robots[i]._params() for i in idx]) as tp:
                    moved = hc.step_vjp_bank(tp, bank, [NETS[i] for i in idx], *[a[idx].contiguous() for a in args], g_next[idx].contiguous())
                assert same_bits(torch, moved, pick(out, idx)), (t, idx)
    _worst[f"step {fam}"] = max(worst.values())
    print("largest error / tolerance so far:", {k: round(v, 3) for k, v in _worst.items()})


def composition(torch, h, table, bank, nets, ctl, states, g):
    """kr_simulate_vjp_bank_batch as the header defines it: the loop of kr_step_vjp_bank_batch calls; g_bnd kept per step"""
    Bc, Tc = ctl.shape[0], ctl.shape[1]
    g = g.clone()
    g_ctl = torch.zeros((Bc, Tc, 4), dtype=ctl.dtype, device=DEV)
    g_bnd = torch.zeros((Bc, Tc, 19), dtype=ctl.dtype, device=DEV)
    resid = torch.zeros((Bc, Tc), dtype=torch.float64, device=DEV)
    status = torch.zeros((Bc, Tc), dtype=torch.int32, device=DEV)
    nn_x = torch.zeros((Tc, Bc, states.shape[2] - 1, 32), dtype=ctl.dtype, device=DEV)
    nn_g = torch.zeros_like(nn_x)
    for t in range(Tc - 1, -1, -1):
        o = h.step_vjp_bank(table, bank, nets, states[t - 1] if t > 0 else states[0], states[t], states[t + 1], ctl[:, t].contiguous(), g[t + 1])
        g[t] += o["g_cur"]
        g[max(t - 1, 0)] += o["g_prev"]
        g_ctl[:, t], g_bnd[:, t] = o["g_tensions"], o["g_bnd"]
        resid[:, t], status[:, t], nn_x[t], nn_g[t] = o["resid"], o["status"], o["nn_x"], o["nn_g"]
    return dict(g_states=g, g_ctl=g_ctl, g_bnd=g_bnd, resid=resid, status=status, nn_x=nn_x, nn_g=nn_g)


@pytest.mark.parametrize("fam", bc.FAMILIES)
def test_rollout_bank_against_the_fixture_and_the_step_calls(torch_cuda, fb, fam):
    """2. bnd_per_step = 1: g_ctl, g_bnd[b][t], the entries of g_states[0] and the weight blocks of each network with rods, block
    by block under the recorded tolerances, for both cotangents and every rod; the call is bit for bit the loop of step calls;
    bnd_per_step = 0 is the sum of the per-step values from zero, t = T - 1 first, bit for bit; two identical calls give identical
    bits; rollout_grad_bank's params[k] is weight_grads over the gathered rows of the direct call bit for bit, and exactly zero
    for the network without rods."""
    torch = torch_cuda
    import krod_grad as kg
    s = setup(torch, fb, fam)
    hc, table, bank, ks, nets, ctl, states = s["hc"], s["table"], s["bank"], s["ks"], s["nets"], s["ctl"], s["states"]
    worst = {}
    names = ("g_ctl", "g_bnd", "resid", "status", "nn_x", "nn_g")
    for c in range(2):
        g0 = _dev(torch, np.stack([fb[k + "gbar"][c] for k in ks], axis=1))
        g = g0.clone()
        out = hc.simulate_vjp_bank(table, bank, NETS, ctl, states, g, bnd_per_step=True)
        assert (out["status"] == 0).all() and tuple(out["g_bnd"].shape) == (B, T, 19) and float(out["resid"].max()) <= RESID_MAX
        assert tuple(out["nn_x"].shape) == (T, B, N - 1, 32)
        ref = composition(torch, hc, table, bank, NETS, ctl, states, g0)
        assert torch.equal(g, ref["g_states"]) and all(torch.equal(out[n], ref[n]) for n in names)
        g2 = g0.clone()
        again = hc.simulate_vjp_bank(table, bank, NETS, ctl, states, g2, bnd_per_step=True)
        assert torch.equal(g2, g) and all(torch.equal(again[n], out[n]) for n in names)
        g3 = g0.clone()
        summed = hc.simulate_vjp_bank(table, bank, NETS, ctl, states, g3)
        acc = torch.zeros((B, 19), dtype=torch.float64, device=DEV)
        for t in range(T - 1, -1, -1):
            acc = acc + out["g_bnd"][:, t]
        assert tuple(summed["g_bnd"].shape) == (B, 19) and torch.equal(summed["g_bnd"], acc) and torch.equal(g3, g)
        assert all(torch.equal(summed[n], out[n]) for n in names if n != "g_bnd")
        norows = hc.simulate_vjp_bank(table, bank, NETS, ctl, states, g0.clone(), need_bnd=False, need_rows=False)
        assert norows["g_bnd"] is None and norows["nn_x"] is None and torch.equal(norows["g_ctl"], out["g_ctl"])
        for b, k in enumerate(ks):
            got = bc.x_got(out["g_ctl"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy(), g[0, b].cpu().numpy())
            bc.x_check(f"{k} cot {c}", got, fb[k + "x_fd_h"][c], fb[k + "x_tol"][c], worst)
        for kk in range(K):
            rods = bc.rods_of(kk)
            if not rods: continue
            gw = bc.weight_grad(nets[kk], out["nn_x"][:, rods][..., :28].cpu().numpy(), out["nn_g"][:, rods][..., :25].cpu().numpy())
            bc.w_check(f"{fam} net {kk} cot {c}", gw, fb[f"{fam}_net{kk}_wfd_h"][c], fb[f"{fam}_net{kk}_w_tol"][c], worst)
        if c == 0:
            params = [as_params(torch, m) for m in nets]
            res = kg.rollout_grad_bank(s["carrier"], s["robots"], ctl, states, params, NETS, g_states=g0, per_step_boundary=True)
            assert np.array_equal(res["ctl"], out["g_ctl"].cpu().numpy()) and np.array_equal(res["boundary"], out["g_bnd"].cpu().numpy())
            assert np.array_equal(res["states"], g.cpu().numpy()) and len(res["params"]) == K
            acts = [int(a) for a in nets[0].acts]
            for kk in range(K):
                rods = bc.rods_of(kk)
                if not rods:
                    assert all(not np.any(a) for a in res["params"][kk]) and len(res["params"][kk]) == 2 * len(acts)
                    continue
                p32 = [p.to(DEV) for p in params[kk]]
                want = kg.weight_grads(hc, p32, acts, out["nn_x"][:, rods].contiguous(), out["nn_g"][:, rods].contiguous())
                assert all(np.array_equal(a, w.cpu().numpy()) for a, w in zip(res["params"][kk], want)), kk
                # the device's fp32 backward over the rows against the fp64 NumPy pass (the bound of tests/test_gpu_nn_adjoint.py)
                ref64 = nc.mlp_backward_rows(nets[kk], out["nn_x"][:, rods][..., :28].cpu().numpy().reshape(-1, 28),
                                             out["nn_g"][:, rods][..., :25].cpu().numpy().reshape(-1, 25))
                flat = np.concatenate([np.asarray(a, np.float64).ravel() for a in res["params"][kk]])
                rel = float(np.linalg.norm(flat - ref64) / np.linalg.norm(ref64))
                print(f"{fam} net {kk}: fp32 weight backward against fp64 NumPy, relative L2 {rel:.2e}")
                assert rel < 2e-5
            summed_res = kg.rollout_grad_bank(s["carrier"], s["robots"], ctl, states, params, NETS, g_states=g0)
            assert summed_res["boundary"].shape == (B, 19) and np.array_equal(summed_res["boundary"], summed["g_bnd"].cpu().numpy())
    _worst[f"rollout {fam}"] = max(worst.values())
    print("largest error / tolerance so far:", {k: round(v, 3) for k, v in _worst.items()})


def nn_fixture_mlp(fn, net):
    import cosserat_oracle as orc
    n = len(nc.NETWORKS[net][0]) + 1
    return orc.Mlp([fn[f"net_{net}_W{k}"] for k in range(n)], [fn[f"net_{net}_b{k}"] for k in range(n)], [int(a) for a in fn[f"net_{net}_acts"]], False)


def nn_fixture_batch(torch, fn, rods):
    """rods = [(set, N, state, net, fixture rod)] of step_adjoint_nn.npz -> (keys, prev, cur, next, tensions): the oracle's step"""
    keys = [nc.nn_case_key(ps, n, state, net) + f"_r{r}_" for ps, n, state, net, r in rods]
    prev = _dev(torch, np.stack([fn[k + "prev"] for k in keys]))
    cur = _dev(torch, np.stack([fn[k + ("prev" if rods[i][2] == "straight" else "cur")] for i, k in enumerate(keys)]))
    return keys, prev, cur, _dev(torch, np.stack([fn[k + "next"] for k in keys])), _dev(torch, np.stack([fn[k + "tens"] for k in keys]))


MIXED = {"tanh17": [("bc", 0), ("bc", 1), ("bc", 2), ("bc", 0)],
         "softplus33x20": [("bc", 0), ("bc", 1), ("bc", 2), ("bc", 1)],
         "elu64x64": [("bc", 0), ("plain", 0), ("bc", 1), ("plain", 1), ("bc", 2), ("plain", 2), ("bc", 2)]}


@pytest.mark.parametrize("net", list(MIXED))
def test_mixed_bank_call_against_the_existing_nn_fixture(torch_cuda, fn, net):
    """3. N = 10: rods of step_adjoint_nn.npz (for elu64x64 of two parameter sets, `bc` from a sine run and `plain` from the
    straight rod) in ONE bank call in which the fixture's network is network 1 of K = 2 and the last rod runs network 0, a
    network of another seed: every rod on the fixture's network is held to its own entry under that fixture's rule."""
    torch = torch_cuda
    n = 10
    rods = [(ps, n, "straight" if ps == "plain" else "sine30", net, r) for ps, r in MIXED[net]]
    keys, prev, cur, nxt, tens = nn_fixture_batch(torch, fn, rods)
    mlp = nn_fixture_mlp(fn, net)
    hidden, act, gain = nc.NETWORKS[net]
    other = nc.signed_mlp(hidden, act, gain, 12)
    nets = [1] * (len(rods) - 1) + [0]
    hc = carrier_for(n, net)._native()
    worst = 0.0
    with hc.param_table([tc.robot_for(ps, n)._params() for ps, *_ in rods]) as table, hc.mlp_bank([as_network(other), as_network(mlp)]) as bank:
        for c in range(3):
            gbar = np.stack([fn[k + "gbar"][c] for k in keys])
            out = hc.step_vjp_bank(table, bank, nets, prev, cur, nxt, tens, _dev(torch, gbar))
            assert (out["status"] == 0).all() and float(out["resid"].max()) <= RESID_MAX
            for b, k in enumerate(keys[:-1]):
                floor = sc.fd_floor(gbar[b], nxt[b].cpu().numpy())
                for name, err, tol, size in sc.block_report(got_vector(out, b), fn[k + "fd_h"][c], fn[k + "fd_2h"][c], n, floor):
                    print(f"{net} rod {b} cot {c} {name:14s} err {err:.3e} tol {tol:.3e} size {size:.3e}")
                    worst = max(worst, err / tol)
                    assert err <= tol, (net, c, b, name, err, tol)
                gw = bc.weight_grad(mlp, out["nn_x"][b, :, :28].cpu().numpy(), out["nn_g"][b, :, :25].cpu().numpy())
                a, b2 = fn[k + "wfd_h"][:, c], fn[k + "wfd_2h"][:, c]
                for lo in range(0, len(gw), 6):
                    err, tol = np.max(np.abs(gw[lo:lo + 6] - a[lo:lo + 6])), sc.block_tol(a[lo:lo + 6], b2[lo:lo + 6], floor)
                    print(f"{net} rod {b} cot {c} weights layer {lo // 6} err {err:.3e} tol {tol:.3e}")
                    assert err <= tol, (net, c, b, lo, err, tol)
            # the last rod is the first rod's state on another network: it must not come out as the first rod
            first = next(i for i, r in enumerate(rods) if r == rods[-1])
            if c == 0: assert not torch.equal(out["g_tensions"][-1], out["g_tensions"][first])
    print(f"{net}: largest error / tolerance {worst:.3f}")


def test_elu512_bank_against_the_handle_calls(torch_cuda, fn):
    """4. One hidden layer of 512 units (eight chunks of the Jacobian kernel), B = 3, K = 2, N = 10, net_of_rod = [0, 1, 0]: the
    bank call against kr_step_vjp_nn_batch on a handle set to each network, under the tolerance the fixture's rule gives each
    block of the rod; whether the two are bit for bit the same is printed."""
    torch = torch_cuda
    n, net = 10, "elu512"
    rods = [("bc", n, "sine30", net, r) for r in range(3)]
    keys, prev, cur, nxt, tens = nn_fixture_batch(torch, fn, rods)
    hidden, act, gain = nc.NETWORKS[net]
    mlps = [nn_fixture_mlp(fn, net), nc.signed_mlp(hidden, act, gain, 12)]
    nets = [0, 1, 0]
    hc = carrier_for(n, net)._native()
    gbar = np.stack([fn[k + "gbar"][0] for k in keys])
    g_next = _dev(torch, gbar)
    robot = make_robot(None, n)
    P = sc.params("bc", n)
    for k in ("Bse", "Bbt", "F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
        setattr(robot, k, np.array(getattr(P, k), dtype=np.float64))
    robot.compute_intermediate_terms()
    hb = robot._native()
    with hc.param_table([robot._params()] * 3) as table, hc.mlp_bank([as_network(m) for m in mlps]) as bank:
        out = hc.step_vjp_bank(table, bank, nets, prev, cur, nxt, tens, g_next)
    assert (out["status"] == 0).all()
    exact = True
    for kk, m in enumerate(mlps):
        hb.set_mlp(*as_network(m))
        ref = hb.step_vjp_nn(prev, cur, nxt, tens, g_next)
        for b in (i for i in range(3) if nets[i] == kk):
            floor = sc.fd_floor(gbar[b], nxt[b].cpu().numpy())
            tols = [tol for _, _, tol, _ in sc.block_report(got_vector(ref, b), fn[keys[b] + "fd_h"][0], fn[keys[b] + "fd_2h"][0], n, floor)]
            g, r = sc.split_grad(got_vector(out, b), n), sc.split_grad(got_vector(ref, b), n)
            for (name, arr, sl), tol in zip(sc.BLOCKS, tols):
                diff = float(np.max(np.abs(g[arr][..., sl] - r[arr][..., sl])))
                print(f"elu512 rod {b} network {kk} {name:14s} |bank - handle| {diff:.3e} tol {tol:.3e}")
                assert diff <= tol, (b, name, diff, tol)
            bits = same_bits(torch, pick(out, slice(b, b + 1)), pick(ref, slice(b, b + 1)))
            print(f"elu512 rod {b} network {kk}: bit for bit the handle's call: {bits}")
            exact = exact and bits
            if kk == 0:  # the fixture's own network: the bank call against the oracle's differences too
                for name, err, tol, size in sc.block_report(got_vector(out, b), fn[keys[b] + "fd_h"][0], fn[keys[b] + "fd_2h"][0], n, floor):
                    assert err <= tol, (b, name, err, tol)
    print("elu512: the bank call is bit for bit the handle calls:", exact)


def test_f32_is_the_f64_call_rounded(torch_cuda, fb):
    """5. The KR_F32 calls are the KR_F64 calls on the upcast inputs, rounded to float: step and rollout."""
    torch = torch_cuda
    s = setup(torch, fb, "tanh17")
    hc, table, bank, ks = s["hc"], s["table"], s["bank"], s["ks"]
    t = bc.STEP_TS[-1]
    g_next = _dev(torch, np.stack([fb[k + f"s{t}_gbar"][0] for k in ks]))
    f32 = [a.float().contiguous() for a in (*step_args(s, t), g_next)]
    lo = hc.step_vjp_bank(table, bank, NETS, *f32)
    hi = hc.step_vjp_bank(table, bank, NETS, *[a.double().contiguous() for a in f32])
    assert (lo["status"] == 0).all() and lo["nn_g"].dtype == torch.float32
    for k in ("g_cur", "g_prev", "g_tensions", "g_bnd", "nn_x", "nn_g"):
        assert torch.equal(lo[k], hi[k].float()), k
    assert torch.equal(lo["resid"], hi["resid"]) and torch.equal(lo["status"], hi["status"])
    ctl32, st32 = s["ctl"].float().contiguous(), s["states"].float().contiguous()
    g0 = _dev(torch, np.stack([fb[k + "gbar"][0] for k in ks], axis=1)).float().contiguous()
    g = g0.clone()
    r32 = hc.simulate_vjp_bank(table, bank, NETS, ctl32, st32, g, bnd_per_step=True)
    ref = composition(torch, hc, table, bank, NETS, ctl32, st32, g0)
    assert r32["g_ctl"].dtype == torch.float32 and torch.equal(g, ref["g_states"])
    assert all(torch.equal(r32[n], ref[n]) for n in ("g_ctl", "g_bnd", "resid", "status", "nn_x", "nn_g"))


def test_failing_rod(torch_cuda, fb):
    """6. One rod's state_next holds a NaN: its status is KR_ST_NONFINITE, its gradients and nn_g rows NaN (its nn_x rows keep
    the inputs); every other rod - those that share its network's Jacobian launch too - is bit for bit the clean call; the
    next call on the handle is clean."""
    torch = torch_cuda
    import krod_native as kn
    s = setup(torch, fb, "softplus33x20")
    hc, table, bank, ks = s["hc"], s["table"], s["bank"], s["ks"]
    t = bc.STEP_TS[-1]
    prev, cur, nxt, tens = step_args(s, t)
    g_next = _dev(torch, np.stack([fb[k + f"s{t}_gbar"][0] for k in ks]))
    clean = hc.step_vjp_bank(table, bank, NETS, prev, cur, nxt, tens, g_next)
    assert (clean["status"] == 0).all()
    bad_next = nxt.clone()
    bad_next[2, 4, 19] = float("nan")  # rod 2: the second of network 1's three rods
    out = hc.step_vjp_bank(table, bank, NETS, prev, cur, bad_next, tens, g_next)
    assert out["status"].tolist() == [0, 0, kn.ST_NONFINITE, 0, 0]
    for k in ("g_tensions", "g_bnd"):
        assert bool(torch.isnan(out[k][2]).all()), k
    assert bool(torch.isnan(out["g_cur"][2, :, :12]).all()) and torch.count_nonzero(out["g_cur"][2, :, 12:]) == 0
    assert bool(torch.isnan(out["nn_g"][2, :, :25]).all()) and torch.count_nonzero(out["nn_g"][2, :, 25:]) == 0
    keep_x = [j for j in range(N - 1) if j != 4]
    assert torch.equal(out["nn_x"][2, keep_x], clean["nn_x"][2, keep_x])
    keep = [0, 1, 3, 4]
    assert same_bits(torch, pick(out, keep), pick(clean, keep))
    assert same_bits(torch, hc.step_vjp_bank(table, bank, NETS, prev, cur, nxt, tens, g_next), clean)
    bad = s["states"].clone()
    bad[2, 1, 3, 20] = float("nan")  # states[2] is state_next of step 1 and state_cur of step 2 (slot 20 is read as next only)
    g0 = _dev(torch, np.stack([fb[k + "gbar"][0] for k in ks], axis=1))
    o_clean = hc.simulate_vjp_bank(table, bank, NETS, s["ctl"], s["states"], g0.clone(), bnd_per_step=True)
    o_bad = hc.simulate_vjp_bank(table, bank, NETS, s["ctl"], bad, g0.clone(), bnd_per_step=True)
    assert o_bad["status"][1].tolist() == [kn.ST_NONFINITE, kn.ST_NONFINITE, 0, 0]
    assert bool(torch.isnan(o_bad["g_bnd"][1, :2]).all()) and torch.equal(o_bad["g_bnd"][1, 2:], o_clean["g_bnd"][1, 2:])
    for b in (0, 2, 3, 4):
        assert all(torch.equal(o_bad[n][b], o_clean[n][b]) for n in ("g_ctl", "g_bnd")) and torch.equal(o_bad["nn_g"][:, b], o_clean["nn_g"][:, b])


def test_refusals_leave_every_output_byte(torch_cuda, fb):
    """7. Each refusal of the header, in the header's order: the (rc, message) pair, the message naming the call, nothing
    launched, and output buffers pre-filled with a pattern come back unchanged.  (An activation on the last layer and a bank
    made for the 53-wide input cannot be built - kr_mlp_bank_create refuses them - so the network's refusals are reached through
    a table of nn_input_history = 1 and a bank of two hidden layers the second of which is wider than 64.)"""
    torch = torch_cuda
    import krod_native as kn
    s = setup(torch, fb, "tanh17")
    hc, table, bank = s["hc"], s["table"], s["bank"]
    lib = hc.lib
    prev, cur, nxt, tens = step_args(s, 0)
    g_next = torch.ones_like(nxt)
    full = lambda *shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=DEV)
    outs = [full(B, N, 28), full(B, N, 28), full(B, 4), full(B, 19), full(B), full(B, dtype=torch.int32), full(B, N - 1, 32), full(B, N - 1, 32)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = (C.c_int32 * B)(*NETS)
    high, low = (C.c_int32 * B)(1, 0, 3, 1, 0), (C.c_int32 * B)(1, 0, 1, -1, 0)
    h33 = tc.carrier_for(33)._native()               # another N
    other_dt = make_robot("youngs", N)
    other_dt.del_t = 0.025
    other_dt.compute_intermediate_terms()
    hdt = other_dt._native()                          # another del_t
    hist = make_robot("youngs", N)
    hist.nn_input_history = True
    hh = hist._native()
    rows_h = []
    for r in s["robots"]:
        q = r._params()
        q.nn_input_history = 1
        rows_h.append(q)
    table_h = hh.param_table(rows_h)                  # a table for the 53-wide input
    wide = nc.signed_mlp((20, 100), "tanh", 0.3, 5)   # a bank the forward call serves and the input Jacobian does not
    bank_w = hc.mlp_bank([as_network(wide)] * K)
    api = b"kr_step_vjp_bank_batch"

    def step(h=hc._h, t=table._t, bk=bank._b, nets=ok, scheme=kn.KR_EULER, g=g_next, dtype=kn.KR_F64, cur_=cur, tens_=tens):
        return lib.kr_step_vjp_bank_batch(h, t, bk, nets, scheme, p(prev), p(cur_), p(nxt), p(tens_), p(g), *[p(o) for o in outs], dtype, None)
    step_cases = ((dict(h=None), kn.KR_E_ARG, b"null handle"), (dict(t=None), kn.KR_E_ARG, api + b": null parameter table"),
                  (dict(bk=None), kn.KR_E_ARG, api + b": null network bank"), (dict(dtype=5), kn.KR_E_ARG, b"dtype"),
                  (dict(g=None), kn.KR_E_ARG, api + b": null pointer"), (dict(cur_=None), kn.KR_E_ARG, api + b": null pointer"),
                  (dict(tens_=None), kn.KR_E_ARG, api + b": null pointer"), (dict(nets=None), kn.KR_E_ARG, api + b": null pointer argument: net_of_rod_host"),
                  (dict(h=h33._h), kn.KR_E_ARG, api + b": parameter table: N of the table differs"),
                  (dict(h=hdt._h), kn.KR_E_ARG, api + b": parameter table: del_t of the table differs"),
                  (dict(nets=high), kn.KR_E_ARG, api + b": network bank: rod 2 asks for network 3, the bank holds 3"),
                  (dict(nets=low), kn.KR_E_ARG, api + b": network bank: rod 3 asks for network -1"),
                  (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, api + b": the adjoint of the RK4 sweep is not served"),
                  (dict(t=table_h._t), kn.KR_E_UNSUPPORTED, api + b": nn_input_history = 1"),
                  (dict(bk=bank_w._b), kn.KR_E_UNSUPPORTED, api + b": two hidden layers of more than 64 units are not served"),
                  # the order: dtype, null pointers, the table, the indices, then what is not served
                  (dict(dtype=5, g=None), kn.KR_E_ARG, b"dtype"), (dict(g=None, nets=high), kn.KR_E_ARG, b"null pointer"),
                  (dict(nets=None, h=h33._h), kn.KR_E_ARG, b"net_of_rod_host"), (dict(h=h33._h, nets=high), kn.KR_E_ARG, b"N of the table differs"),
                  (dict(nets=high, scheme=kn.KR_RK4), kn.KR_E_ARG, b"asks for network 3"),
                  (dict(scheme=kn.KR_RK4, bk=bank_w._b), kn.KR_E_UNSUPPORTED, b"RK4"))
    for kw, want, word in step_cases:
        rc = step(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    Ts = 2
    states = torch.zeros((Ts + 1, B, N, 28), dtype=torch.float64, device=DEV)
    ctl = torch.zeros((B, Ts, 4), dtype=torch.float64, device=DEV)
    g_states = full(Ts + 1, B, N, 28)
    souts = [full(B, N, 28), full(B, Ts, 4), full(B, Ts, 19)]
    stail = [full(B, Ts), full(B, Ts, dtype=torch.int32), full(Ts, B, N - 1, 32), full(Ts, B, N - 1, 32)]
    sapi = b"kr_simulate_vjp_bank_batch"

    def sim(h=hc._h, t=table._t, bk=bank._b, nets=ok, T_=Ts, scheme=kn.KR_EULER, st=states, dtype=kn.KR_F64, per_step=1):
        return lib.kr_simulate_vjp_bank_batch(h, t, bk, nets, T_, scheme, p(ctl), p(st), None, p(g_states), *[p(o) for o in souts], per_step,
                                              *[p(o) for o in stail], dtype, None)
    sim_cases = ((dict(h=None), kn.KR_E_ARG, b"null handle"), (dict(t=None), kn.KR_E_ARG, sapi + b": null parameter table"),
                 (dict(bk=None), kn.KR_E_ARG, sapi + b": null network bank"), (dict(per_step=2), kn.KR_E_ARG, sapi + b": bnd_per_step"),
                 (dict(dtype=-1), kn.KR_E_ARG, b"dtype"), (dict(T_=0), kn.KR_E_ARG, sapi + b": T < 1"), (dict(st=None), kn.KR_E_ARG, sapi + b": null pointer"),
                 (dict(nets=None), kn.KR_E_ARG, sapi + b": null pointer argument: net_of_rod_host"),
                 (dict(h=h33._h), kn.KR_E_ARG, sapi + b": parameter table: N of the table differs"),
                 (dict(h=hdt._h), kn.KR_E_ARG, b"del_t of the table differs"), (dict(nets=high), kn.KR_E_ARG, sapi + b": network bank: rod 2 asks for network 3"),
                 (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, sapi + b": the adjoint of the RK4"),
                 (dict(t=table_h._t), kn.KR_E_UNSUPPORTED, sapi + b": nn_input_history = 1"),
                 (dict(bk=bank_w._b), kn.KR_E_UNSUPPORTED, sapi + b": two hidden layers"), (dict(T_=0, st=None), kn.KR_E_ARG, b"T < 1"))
    for kw, want, word in sim_cases:
        rc = sim(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    torch.cuda.synchronize()
    for o in outs + souts + stail + [g_states]:
        assert bool((o == 7).all())
    with pytest.raises(kn.KrError, match="the states hold 3 rods, the parameter table 5"):
        hc.step_vjp_bank(table, bank, NETS[:3], prev[:3], cur[:3], nxt[:3], tens[:3], g_next[:3])
    with pytest.raises(kn.KrError, match="net_of_rod 4"):
        hc.step_vjp_bank(table, bank, NETS[:4], prev, cur, nxt, tens, g_next)
    with pytest.raises(kn.KrError, match="must be a ParamTable"):
        hc.step_vjp_bank(None, bank, NETS, prev, cur, nxt, tens, g_next)
    with pytest.raises(kn.KrError, match="must be an MlpBank"):
        hc.simulate_vjp_bank(table, None, NETS, ctl, states, g_states)
    bank_w.close()
    table_h.close()


def test_simulate_tips_bank_backward_is_the_direct_call(torch_cuda, fb):
    """8. simulate_tips_bank(...): the forward is the bank call with per-step boundary data and reproduces the oracle's tips;
    backward() fills ctl.grad, every params[k][i].grad, base_motion.grad and tip_loads.grad with what the direct call and
    weight_grads over its gathered rows give, bit for bit; the network without rods gets zeros; the carrier robot keeps its own
    weights (the handle's network is neither read nor replaced)."""
    torch = torch_cuda
    import krod_grad as kg
    fam = "tanh17"
    s = setup(torch, fb, fam)
    hc, ks, nets, carrier = s["hc"], s["ks"], s["nets"], s["carrier"]
    own = [np.array(a, copy=True) for a in carrier.param_ls]
    carrier._native()  # (the robot's own weights are the handle's)
    key_before = carrier._mlp_key
    assert key_before is not None
    probe = _dev(torch, np.linspace(-1.0, 1.0, 3 * 28).reshape(3, 28))
    before = hc.mlp_eval(probe)
    params = [[p.requires_grad_(True) for p in as_params(torch, m)] for m in nets]
    leaf = s["ctl"].clone().requires_grad_(True)
    base = s["bnd"][:, :, :13].clone().requires_grad_(True)
    loads = s["bnd"][:, :, 13:].clone().requires_grad_(True)
    w = _dev(torch, np.stack([fb[k + "gbar"][0][1:, N - 1, 12:15] for k in ks]))  # [B, T, 3]: the tip cotangent of every step
    tips = kg.simulate_tips_bank(carrier, s["robots"], leaf, params, NETS, base_motion=base, tip_loads=loads)
    oracle_tips = s["states"][1:, :, N - 1, 12:15].permute(1, 0, 2)
    miss = float((tips.detach() - oracle_tips).abs().max())
    print(f"simulate_tips_bank forward against the oracle's tips: {miss:.2e}")
    assert tuple(tips.shape) == (B, T, 3) and miss < 1e-9
    (tips * w).sum().backward()
    # the direct call on the states of THAT forward run
    states = hc.new_state(B, torch.float64, n_slots=T + 1)
    hc.init_straight(states[0], table=s["table"])
    G = torch.zeros((B, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((B, T), dtype=torch.int32, device=DEV)
    hc.simulate(s["ctl"], states, G, ring=False, status=status, tol=1e-12, table=s["table"], bank=s["bank"], net_of_rod=NETS, bnd=s["bnd"])
    assert (status == 0).all() and torch.equal(states[1:, :, N - 1, 12:15].permute(1, 0, 2), tips.detach())
    g = torch.zeros_like(states)
    g[1:, :, N - 1, 12:15] = w.permute(1, 0, 2)
    direct = hc.simulate_vjp_bank(s["table"], s["bank"], NETS, s["ctl"], states, g, bnd_per_step=True)
    assert torch.equal(leaf.grad, direct["g_ctl"])
    assert torch.equal(base.grad, direct["g_bnd"][:, :, :13]) and torch.equal(loads.grad, direct["g_bnd"][:, :, 13:])
    acts = [int(a) for a in nets[0].acts]
    for kk in range(K):
        rods = bc.rods_of(kk)
        if not rods:
            assert all(p.grad is not None and torch.count_nonzero(p.grad) == 0 for p in params[kk])
            continue
        p32 = [p.detach().to(DEV) for p in params[kk]]
        want = kg.weight_grads(hc, p32, acts, direct["nn_x"][:, rods].contiguous(), direct["nn_g"][:, rods].contiguous())
        assert all(torch.equal(p.grad, wv.cpu()) for p, wv in zip(params[kk], want)), kk
    # and against the fixture: the tip cotangent is cotangent 0 of the rollout
    for b, k in enumerate(ks):
        got = bc.x_got(leaf.grad[b].cpu().numpy(), torch.cat([base.grad[b], loads.grad[b]], dim=1).cpu().numpy(), np.zeros((N, 28)))
        bl = [(nm, idx, tol) for (nm, idx), tol in zip(bc.x_blocks(T, False), fb[k + "x_tol"][0]) if nm.startswith(("g_ctl", "g_bnd"))]
        bc.assert_blocks(f"{k} autograd", [nm for nm, _, _ in bl], [got[i] for _, i, _ in bl], [fb[k + "x_fd_h"][0][i] for _, i, _ in bl],
                         [tol for _, _, tol in bl])
    assert carrier._mlp_key == key_before and all(np.array_equal(a, b) for a, b in zip(own, carrier.param_ls))
    assert torch.equal(carrier._native().mlp_eval(probe), before)  # (the handle still evaluates the robot's own network)
