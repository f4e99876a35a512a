#!/usr/bin/env python3
"""Generate tests/golden/bank_motion.npz by IMPORTING THE REFERENCE (like make_golden_base_motion.py: runs only where the
reference is; the fixture is data only - inputs and the reference's outputs on them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bank_motion.py

Rods with their OWN network on a moving base under a tip wrench that varies in time: what the evaluation half of the
reference's experiment would see with the six boundary attributes assigned between two solves.  The network is injected
as physics_train.py:142-144 does (nn_model, param_ls, nn_path = 'whatever'); p0 / h0 / q0 / w0 / F_tip / M_tip are plain
attributes that getResidualEuler reads at every solve, and knode.simulate iterates over its controls (knode.py:70): an
iterable that assigns the six while it yields control t gives the reference's answer, with no reference code changed.
fsolve is wrapped to record ier, which the reference discards (knode.py:89); nothing is written unless ier == 1 on every
step of every rod.  (Rows 1, 2, 3 and 5 of tests/bank_keypoints_cases.py: all four converge, none had to be replaced.)

The reference drops its last solve (knode.py:102): T controls give states 0 .. T-1.

Arrays (N = 10, T = 12, four rods in the order of ``mods``): ``mods``, ``base_cases``, ``load_cases`` (names), ``nets``
int[4] (network of each rod), ``ctl`` [T, 4], ``bnd`` [4, T, 19] (p0 h0 q0 w0 F_tip M_tip), the bank's weights as
``net{k}_W{l}`` / ``net{k}_b{l}`` / ``net{k}_acts`` / ``net{k}_history``, ``ier`` [4, T], ``traj`` [4, T, 25, N],
``tips`` [4, T, 3]."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference/knode_cosserat"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))
sys.path.insert(2, os.path.join(HERE, "..", "..", "oracle"))

import numpy as np
import torch
import torch.nn as nn

import cosserat_ode as ref_ode  # noqa: E402  (reference)
import knode as ref_knode  # noqa: E402

import cosserat_oracle as orc  # noqa: E402  (only for the networks' weights: input generators)
import bank_keypoints_cases as cases  # noqa: E402  (the rods: one definition for generator and tests)
from mlp_bank_cases import controls  # noqa: E402

torch.set_num_threads(1)
ACT_MODULE = {orc.ACT_TANH: nn.Tanh, orc.ACT_SOFTPLUS: nn.Softplus, orc.ACT_RELU: nn.ReLU, orc.ACT_ELU: nn.ELU}


class FsolveSpy:
    def __init__(self):
        from scipy.optimize import fsolve
        self._f = fsolve
        self.ier = []

    def __call__(self, fun, x0, args=()):
        x, info, ier, _ = self._f(fun, x0, args=args, full_output=True)
        self.ier.append(ier)
        return x


def inject_nn(robot, mlp):
    """physics_train.py:142-144 with an nn.ModuleList in the layer order the reference walks by str()"""
    mods = []
    for W, b, act in zip(mlp.weights, mlp.biases, mlp.acts):
        lin = nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(W))
            lin.bias.copy_(torch.tensor(b))
        mods.append(lin)
        if act != orc.ACT_NONE:
            mods.append(ACT_MODULE[act]())
    ml = nn.ModuleList(mods)
    robot.nn_model = ml
    robot.param_ls = [t.detach().cpu().numpy() for _, t in ml.state_dict().items()]
    robot.nn_path = "whatever"
    robot.nn_input_history = mlp.history


def moved_controls(r, ctl, bnd):
    """yields control t with the boundary of step t assigned first"""
    for t, c in enumerate(ctl):
        r.p0, r.h0 = np.array(bnd[t, 0:3], dtype=np.float64), np.array(bnd[t, 3:7], dtype=np.float64)
        r.q0, r.w0 = np.array(bnd[t, 7:10], dtype=np.float64), np.array(bnd[t, 10:13], dtype=np.float64)
        r.F_tip, r.M_tip = np.array(bnd[t, 13:16], dtype=np.float64), np.array(bnd[t, 16:19], dtype=np.float64)
        yield c


def run(N, mod, ctl, bnd, mlp):
    r = ref_ode.CosseratRod(use_fsolve=True)
    ref_knode.setup_robot(r, mod)
    r.N = N
    r.compute_intermediate_terms()
    inject_nn(r, mlp)
    spy = FsolveSpy()
    old = ref_knode.fsolve
    ref_knode.fsolve = spy
    try:
        with np.errstate(all="ignore"):
            traj = ref_knode.simulate(r, moved_controls(r, ctl, bnd))
    finally:
        ref_knode.fsolve = old
    return traj[:, :25], np.array(spy.ier)


def main():
    case = cases.FIXTURE
    N, T, which = case["N"], case["T"], case["bank"]
    ctl = np.array(controls(T), dtype=np.float64)
    bnd = cases.bnd_of(case)
    nets = cases.nets_of(case, which)
    bank = cases.bank(which)
    trajs, iers = zip(*(run(N, r[0], ctl, bnd[b], bank[nets[b]]) for b, r in enumerate(case["rows"])))
    trajs, iers = np.stack(trajs), np.stack(iers)
    print(f"  N = {N}, T = {T}: ier all 1: {bool((iers == 1).all())}")
    if not (iers == 1).all():
        sys.exit("fsolve did not converge on every step: nothing written")
    out = {"mods": np.array([str(r[0]) for r in case["rows"]]), "base_cases": np.array([r[1] for r in case["rows"]]),
           "load_cases": np.array([r[2] for r in case["rows"]]), "nets": np.array(nets, dtype=np.int32), "ctl": ctl, "bnd": bnd,
           "ier": iers, "traj": trajs, "tips": trajs[:, :, :3, -1]}
    for k, mlp in enumerate(bank):
        for l, (W, b) in enumerate(zip(mlp.weights, mlp.biases)):
            out[f"net{k}_W{l}"], out[f"net{k}_b{l}"] = W, b
        out[f"net{k}_acts"] = np.array(mlp.acts, dtype=np.int32)
        out[f"net{k}_history"] = np.array(int(mlp.history))
    path = os.path.join(HERE, "bank_motion.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote bank_motion.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
