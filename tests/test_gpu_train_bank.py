"""GPU tests of the bank of trainings (``kr_train_bank_*``, ``KnodeBankTrainer``): training k of a bank against the SAME
training run alone through ``kr_train_epochs`` / ``KnodeTrainer`` on copies of the same buffers.  The bank deals a
network's row blocks out over the workgroups the one-network call would launch for it, so the arithmetic and its order
are the same: every comparison here is ``torch.equal``, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE, TANH, SOFTPLUS, RELU, ELU = range(5)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, threshold=1e-4, min_lr=0.0)
K = 4
DENOM = 29.0
LOG = 16
STATE = ("params", "grads", "exp_avg", "exp_avg_sq", "sched", "loss_log")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import krod_native as kn
    p = kn.KrParams()
    kn.check(kn.load().kr_default_params(C.byref(p)))
    p.N = 10
    return torch, kn, kn.Handle(p)


def make_training(torch, seed, S, dims, lr=1e-2, clamp=True, converged=False):
    """Seeded buffers of one training: rows, nn.Linear-style parameters, zero moments, a fresh schedule."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    Q = S * K
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    x = torch.zeros(Q, 32)
    x[:, :28] = 0.5 * rnd(Q, 28)
    base = 0.3 * rnd(Q, 25)
    base[:, 3:7] = torch.nn.functional.normalize(rnd(Q, 4) + torch.tensor([2.0, 0, 0, 0]), dim=1)
    target = base + 0.05 * rnd(Q, 25)
    params, lower = [], []
    for k in range(len(dims) - 1):
        bound = 1.0 / np.sqrt(dims[k])
        W = (torch.rand(dims[k + 1], dims[k], generator=g) * 2 - 1) * bound
        b = (torch.rand(dims[k + 1], generator=g) * 2 - 1) * bound
        if converged and k == len(dims) - 2:  # MLP output 0 and target = base: the loss is 0 and stays there
            W, b = torch.zeros_like(W), torch.zeros_like(b)
        params += [W.reshape(-1), b]
        lower += [torch.zeros(W.numel()), torch.full((b.numel(),), float("-inf"))]
    if converged:
        target = base.clone()
    p = torch.cat(params)
    n = p.numel()
    t = dict(S=S, x=x, base=base, target_rows=target, params=p, grads=torch.zeros(n + 1), exp_avg=torch.zeros(n),
             exp_avg_sq=torch.zeros(n), lower=torch.cat(lower) if clamp else None,
             sched=torch.tensor([lr, lr, float("inf"), 0.0, 0.0, 0.0], dtype=torch.float64), loss_log=torch.zeros(LOG))
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in t.items()}


def clone_training(torch, t):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}


def run_solo(env, t, dims, acts, n_epochs, step=1, patience=80, factor=0.5):
    torch, kn, h = env
    n = len(dims) - 1
    dims_c, acts_c = (C.c_int32 * (n + 1))(*dims), (C.c_int32 * n)(*acts)
    Q = t["S"] * K
    ws = torch.empty(h.lib.kr_mlp_ws_bytes(n, dims_c, Q), dtype=torch.uint8, device=DEV)
    dout = torch.zeros(Q, 32, device=DEV)
    kn.check(h.lib.kr_train_epochs(
        h._h, n_epochs, t["S"], K, n, dims_c, acts_c, kn._ptr(t["params"]), kn._ptr(t["grads"]), kn._ptr(t["exp_avg"]),
        kn._ptr(t["exp_avg_sq"]), kn._ptr(t["lower"]), kn._ptr(t["sched"]), kn._ptr(t["x"]), 32, kn._ptr(t["base"]),
        kn._ptr(t["target_rows"]), DENOM, kn._ptr(dout), kn._ptr(ws), ADAM["beta1"], ADAM["beta2"], ADAM["eps"],
        ADAM["weight_decay"], step, factor, patience, ADAM["threshold"], ADAM["min_lr"],
        t["loss_log"].data_ptr() + 4 * (step - 1), 1, kn._stream()))
    torch.cuda.synchronize()


def bank_nets(env, ts):
    torch, kn, h = env
    ds = float(h.derived().ds)
    nets = (kn.KrTrainBankNet * len(ts))()
    for k, t in enumerate(ts):
        nets[k].S, nets[k].ds = t["S"], ds
        for f in ("params", "grads", "exp_avg", "exp_avg_sq", "lower", "sched", "x", "base", "target_rows", "loss_log"):
            setattr(nets[k], f, None if t[f] is None else t[f].data_ptr())
    return nets


def bank_create(env, ts, dims, acts):
    torch, kn, h = env
    n = len(dims) - 1
    out = C.c_void_p()
    rc = h.lib.kr_train_bank_create(h._h, len(ts), bank_nets(env, ts), K, n, (C.c_int32 * (n + 1))(*dims),
                                    (C.c_int32 * n)(*acts), 32, DENOM, C.byref(out))
    return rc, out


def bank_epochs(env, bank, n_epochs, step=1, patience=80, factor=0.5, repack=0):
    torch, kn, h = env
    rc = h.lib.kr_train_bank_epochs(h._h, bank, n_epochs, step, ADAM["beta1"], ADAM["beta2"], ADAM["eps"],
                                    ADAM["weight_decay"], factor, patience, ADAM["threshold"], ADAM["min_lr"], step - 1,
                                    repack, kn._stream())
    torch.cuda.synchronize()
    return rc


def assert_same(torch, got, ref, what):
    for f in STATE:
        assert torch.equal(got[f], ref[f]), (what, f, (got[f].double() - ref[f].double()).abs().max().item())
    assert float(got["grads"].abs().max()) == 0.0, what


def bank_against_solo(env, S, dims, acts, n_epochs, seeds, **sched):
    torch, kn, h = env
    solo = [make_training(torch, seed, s, dims, clamp=(i % 2 == 0)) for i, (seed, s) in enumerate(zip(seeds, S))]
    inb = [clone_training(torch, t) for t in solo]
    rc, bank = bank_create(env, inb, dims, acts)
    assert rc == 0, kn.load().kr_last_error()
    try:
        assert bank_epochs(env, bank, n_epochs, **sched) == 0, kn.load().kr_last_error()
    finally:
        h.lib.kr_train_bank_destroy(bank)
    for k, t in enumerate(solo):
        run_solo(env, t, dims, acts, n_epochs, **sched)
        assert_same(torch, inb[k], t, f"network {k} (S = {S[k]})")
        assert torch.isfinite(t["loss_log"][:n_epochs]).all() and float(t["loss_log"][:n_epochs].min()) > 0.0
        assert not torch.equal(t["params"], make_training(torch, seeds[k], S[k], dims)["params"])  # (it did train)


def test_ragged_rows_and_mixed_sizes(env):
    """28 -> 512 -> 25: Q = 116, 232, 4, 348 - every one with a ragged last row block of 32, one smaller than a row block,
    one with more backward groups (3 x 8 workgroups) than the others (1 / 2 x 8: their surplus workgroups return early);
    5 epochs from step 1: both parities of the rate slot."""
    bank_against_solo(env, (29, 58, 1, 87), [28, 512, 25], [TANH, NONE], 5, seeds=(11, 12, 13, 14))


@pytest.mark.parametrize("dims,acts", [
    ([28, 64, 64, 25], [SOFTPLUS, SOFTPLUS, NONE]),
    ([28, 40, 24, 25], [RELU, RELU, NONE]),   # three-layer kernels at ragged widths
    ([28, 96, 25], [SOFTPLUS, NONE]),         # two hidden chunks, the second one ragged
    ([28, 96, 25], [RELU, NONE]),
])
def test_other_kernels(env, dims, acts):
    bank_against_solo(env, (29, 3), dims, acts, 4, seeds=(21, 22))


def test_schedules_are_per_network(env):
    """patience 0: every epoch that does not improve halves the rate of ITS training only."""
    torch, kn, h = env
    dims, acts = [28, 512, 25], [TANH, NONE]
    solo = [make_training(torch, 31, 29, dims, lr=1e-3, clamp=False), make_training(torch, 32, 58, dims, lr=0.2),
            make_training(torch, 33, 29, dims, converged=True)]
    inb = [clone_training(torch, t) for t in solo]
    rc, bank = bank_create(env, inb, dims, acts)
    assert rc == 0, kn.load().kr_last_error()
    try:
        assert bank_epochs(env, bank, 8, patience=0) == 0, kn.load().kr_last_error()
    finally:
        h.lib.kr_train_bank_destroy(bank)
    for k, t in enumerate(solo):
        run_solo(env, t, dims, acts, 8, patience=0)
        assert_same(torch, inb[k], t, f"network {k}")
    rates = [float(t["sched"][8 & 1]) for t in inb]
    print("final learning rates:", rates, "reductions:", [float(t["sched"][5]) for t in inb])
    assert len(set(rates)) >= 2, rates
    assert float(inb[2]["sched"][5]) == 7.0  # the converged training: one reduction per epoch after the first


def make_robot(torch, seed, mod, H=512):
    from cosserat_ode_torch import CosseratRodTorch
    from knode import setup_robot
    torch.manual_seed(seed)
    rob = CosseratRodTorch(DEV, H)
    setup_robot(rob, mod)
    rob.N = 10
    rob.compute_intermediate_terms()
    return rob


def robot_copy(torch, rob, mod):
    cp = make_robot(torch, 0, mod, H=rob.nn_models[0].out_features)
    with torch.no_grad():
        for a, b in zip(rob.nn_models.parameters(), cp.nn_models.parameters()):
            b.copy_(a)
    return cp


@pytest.fixture(scope="module")
def rod_data(env):
    """Per training: one or two trajectories [M, 30, 25, 10] with their controls (the golden trajectory and a perturbed
    copy of it - to the trainer they are data)."""
    torch = env[0]
    g = load_golden("train_step")
    traj, ctl = torch.tensor(g["traj"], device=DEV), torch.tensor(g["controls"], device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(5)
    traj2 = traj * (1.0 + 1e-2 * torch.randn(traj.shape, generator=gen).to(DEV))
    two = (torch.stack([traj, traj2]), torch.stack([ctl, 1.1 * ctl]))
    one = (traj[None], ctl[None])
    return one, two


MODS = ("nsw", "short", "youngs", "lengthstiff")


def test_bank_trainer_per_network_ds_and_parameters(env, rod_data):
    torch, kn, _ = env
    from krod_train import KnodeBankTrainer, KnodeTrainer
    one, two = rod_data
    data = [one, two, one, two]
    robots = [make_robot(torch, 40 + k, mod) for k, mod in enumerate(MODS)]
    assert len({float(r._native().derived().ds) for r in robots}) >= 2  # (short / lengthstiff change L, hence ds)
    alone = [robot_copy(torch, r, mod) for r, mod in zip(robots, MODS)]
    bank = KnodeBankTrainer(robots, [d[0] for d in data], [d[1] for d in data], [3, 5, 7, 9])
    bank.run(4)
    l5 = bank.step()
    l6 = bank.step()
    losses = bank.losses()
    assert [l[4] for l in losses] == l5 and [l[5] for l in losses] == l6
    for k, (rob, (tr, ct)) in enumerate(zip(alone, data)):
        solo = KnodeTrainer(rob, tr, ct, [3, 5, 7, 9])
        solo.run(4)
        solo.step()
        solo.step()
        assert solo.losses() == losses[k], (k, solo.losses(), losses[k])
        assert torch.equal(solo.flat_p, bank.flat_p[k]), k
        assert torch.equal(solo.exp_avg, bank.exp_avg[k]) and torch.equal(solo.exp_avg_sq, bank.exp_avg_sq[k]), k
        assert solo.scheduler.get_last_lr()[0] == bank.get_last_lr()[k]
        for a, b in zip(rob.nn_models.parameters(), robots[k].nn_models.parameters()):
            assert torch.equal(a, b), k  # robots[k].nn_models holds the trained weights
        sd, sd_solo = bank.optimizer_state_dict(k), solo.optimizer_state_dict()
        assert sorted(sd["state"]) == sorted(sd_solo["state"]) and sd["param_groups"][0].keys() == sd_solo["param_groups"][0].keys()
        assert torch.equal(sd["state"][0]["exp_avg"], sd_solo["state"][0]["exp_avg"])
    assert float(bank.grads.abs().max()) == 0.0
    bank.close()


def test_bank_trainer_continuation_and_repack(env, rod_data):
    torch, kn, _ = env
    from krod_train import KnodeBankTrainer, KnodeTrainer
    one, two = rod_data
    data = [one, two, one]
    mods = ("nsw", "short", "youngs")
    robots = [make_robot(torch, 50 + k, mod, H=64) for k, mod in enumerate(mods)]
    alone = [robot_copy(torch, r, mod) for r, mod in zip(robots, mods)]
    bank = KnodeBankTrainer(robots, [d[0] for d in data], [d[1] for d in data], [3, 5, 7, 9])
    solos = [KnodeTrainer(rob, tr, ct, [3, 5, 7, 9]) for rob, (tr, ct) in zip(alone, data)]
    bank.run(3)
    for s in solos:
        s.run(3)
    with torch.no_grad():  # "a checkpoint" lands in the parameters of training 1, in the bank and in its solo twin
        gen = torch.Generator(device="cpu").manual_seed(6)
        for a, b in zip(robots[1].nn_models.parameters(), alone[1].nn_models.parameters()):
            new = (0.02 * torch.rand(a.shape, generator=gen)).to(DEV)
            a.copy_(new)
            b.copy_(new)
    bank.weights_changed()
    solos[1].weights_changed()
    bank.run(3)
    for s in solos:
        s.run(3)
    losses = bank.losses()
    for k, s in enumerate(solos):
        assert s.losses() == losses[k], k
        assert torch.equal(s.flat_p, bank.flat_p[k]) and torch.equal(s.exp_avg_sq, bank.exp_avg_sq[k]), k
    bank.close()


def test_bank_trainer_refuses_differing_structures(env, rod_data):
    torch, kn, _ = env
    from krod_train import KnodeBankTrainer
    one, _ = rod_data
    robots = [make_robot(torch, 60, "nsw", H=64), make_robot(torch, 61, "short", H=32)]
    with pytest.raises(kn.KrError, match="share one MLP structure"):
        KnodeBankTrainer(robots, [one[0]] * 2, [one[1]] * 2, [3, 5, 7, 9])


def test_refusals_launch_nothing(env):
    torch, kn, h = env
    dims, acts = [28, 512, 25], [TANH, NONE]
    ts = [make_training(torch, 70 + k, s, dims) for k, s in enumerate((29, 3))]
    before = [clone_training(torch, t) for t in ts]
    four = [make_training(torch, 75, 29, [28, 32, 32, 32, 25])]
    four_before = clone_training(torch, four[0])
    rc, out = bank_create(env, four, [28, 32, 32, 32, 25], [TANH, TANH, TANH, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and not out.value and b"4 layers" in kn.load().kr_last_error()
    rc, bank = bank_create(env, ts, dims, acts)
    assert rc == 0, kn.load().kr_last_error()
    try:
        assert bank_epochs(env, bank, 2, step=0) == kn.KR_E_ARG and b"step" in kn.load().kr_last_error()
        assert bank_epochs(env, bank, 2, factor=1.0) == kn.KR_E_ARG and b"factor" in kn.load().kr_last_error()
        assert bank_epochs(env, bank, -1) == kn.KR_E_ARG and b"n_epochs" in kn.load().kr_last_error()
    finally:
        h.lib.kr_train_bank_destroy(bank)
    for got, ref in zip(ts + four, before + [four_before]):
        for f in ("params", "grads", "sched", "exp_avg", "exp_avg_sq", "loss_log"):
            assert torch.equal(got[f], ref[f]), f
