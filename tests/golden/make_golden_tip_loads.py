#!/usr/bin/env python3
"""Generate tests/golden/tip_loads.npz by IMPORTING THE REFERENCE (like make_golden.py: runs only where the reference
is; the fixture is data only - inputs and the reference's outputs on them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tip_loads.py

A tip wrench that varies in time.  In the reference F_tip / M_tip are plain attributes that getResidualEuler reads at
every solve (cosserat_ode.py:28-29, :206-207) and knode.simulate iterates over its controls (knode.py:70): an iterable
that assigns robot.F_tip / robot.M_tip while it yields control t gives the reference's answer for a wrench history, with
no reference code changed.  fsolve is wrapped to record ier, which the reference discards (knode.py:89).

The reference drops its last solve (knode.py:102): T controls give states 0 .. T-1, and the load of step T-1 is consumed
but its state not returned.

Arrays, per (N, T) in ((10, 12), (23, 13)) with key suffix ``_n{N}``: ``ctl`` [T, 4]; ``loads`` [4, T, 6] and
``tips`` [4, T, 3], ``last`` [4, 25, N], ``ier`` [4, T] in the order of ``cases``; ``tips_zero`` [T, 3], ``ier_zero``: the
same run with no load; N = 10 only: ``traj`` [4, T, 25, N]."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference/knode_cosserat"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import numpy as np

import cosserat_ode as ref_ode  # noqa: E402  (reference)
import knode as ref_knode  # noqa: E402
import physics_controls as ref_ctl  # noqa: E402

CASES = ("const", "jump", "alt", "sine")
SHAPES = ((10, 12), (23, 13))


def load_history(case, T):
    """[T, 6] = F_tip (3), M_tip (3) of step t = 0 .. T-1"""
    t = np.arange(T, dtype=np.float64)
    L = np.zeros((T, 6))
    if case == "const":  # the wrench of the `bc` fixture
        L[:] = [0.05, -0.02, 0.1, 1e-3, 2e-3, -1e-3]
    elif case == "jump":
        L[T // 2:, 0] = 0.1
        L[T // 2:, 4] = 2e-3
    elif case == "alt":
        sgn = (-1.0) ** t
        L[:, 0] = 0.05 * sgn
        L[:, 1] = -0.02 * sgn
        L[:, 5] = 1e-3 * sgn
    elif case == "sine":
        L[:, 0] = 0.05 * np.sin(2 * np.pi * t / 8)
        L[:, 2] = 0.05 * np.cos(2 * np.pi * t / 8)
        L[:, 3] = 1e-3 * np.sin(2 * np.pi * t / 5)
    else:
        raise ValueError(case)
    return L


class FsolveSpy:
    def __init__(self):
        from scipy.optimize import fsolve
        self._f = fsolve
        self.ier = []

    def __call__(self, fun, x0, args=()):
        x, info, ier, _ = self._f(fun, x0, args=args, full_output=True)
        self.ier.append(ier)
        return x


def loaded_controls(r, ctl, loads):
    """yields control t with the wrench of step t assigned first"""
    for c, w in zip(ctl, loads):
        r.F_tip = np.array(w[:3], dtype=np.float64)
        r.M_tip = np.array(w[3:], dtype=np.float64)
        yield c


def run(N, ctl, loads):
    r = ref_ode.CosseratRod(use_fsolve=True)
    ref_knode.setup_robot(r, None)
    r.N = N
    r.compute_intermediate_terms()
    spy = FsolveSpy()
    old = ref_knode.fsolve
    ref_knode.fsolve = spy
    try:
        with np.errstate(all="ignore"):
            traj = ref_knode.simulate(r, loaded_controls(r, ctl, loads))
    finally:
        ref_knode.fsolve = old
    return traj[:, :25], np.array(spy.ier)


def main():
    out = {"cases": np.array(CASES)}
    for N, T in SHAPES:
        ctl = np.array(ref_ctl.calc_controls("sine", 1.0, 0.05, T), dtype=np.float64)
        loads = np.stack([load_history(c, T) for c in CASES])
        trajs, iers = zip(*(run(N, ctl, loads[k]) for k in range(len(CASES))))
        trajs, iers = np.stack(trajs), np.stack(iers)
        zero, ier0 = run(N, ctl, np.zeros((T, 6)))
        k = f"_n{N}"
        out.update({"ctl" + k: ctl, "loads" + k: loads, "tips" + k: trajs[:, :, :3, -1], "last" + k: trajs[:, -1],
                    "ier" + k: iers, "tips_zero" + k: zero[:, :3, -1], "ier_zero" + k: ier0})
        if N == 10:
            out["traj" + k] = trajs
        print(f"  N = {N}, T = {T}: ier all 1: {bool((iers == 1).all() and (ier0 == 1).all())}")
    path = os.path.join(HERE, "tip_loads.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote tip_loads.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
