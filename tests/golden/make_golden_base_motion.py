#!/usr/bin/env python3
"""Generate tests/golden/base_motion.npz by IMPORTING THE REFERENCE (like make_golden_tip_loads.py: runs only where the
reference is; the fixture is data only - inputs and the reference's outputs on them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_base_motion.py

A base that moves in time.  In the reference p0 / h0 / q0 / w0 are plain attributes that getResidualEuler reads at every
solve (cosserat_ode.py:44-47, :194) and knode.simulate iterates over its controls (knode.py:70): an iterable that assigns
the four while it yields control t gives the reference's answer for a base history, with no reference code changed.
fsolve is wrapped to record ier, which the reference discards (knode.py:89); nothing is written unless ier == 1 on every
step of every run.

The reference drops its last solve (knode.py:102): T controls give states 0 .. T-1, and the base of step T-1 is consumed
but its state not returned.

Arrays, per (N, T) in ((10, 12), (23, 13)) with key suffix ``_n{N}``: ``ctl`` [T, 4]; ``base`` [5, T, 13] and
``tips`` [5, T, 3], ``last`` [5, 25, N], ``ier`` [5, T] in the order of ``cases``; ``tips_unmoved`` [T, 3],
``last_unmoved`` [25, N], ``ier_unmoved``: the same run with the base left alone; N = 10 only: ``traj`` [5, T, 25, N]."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference/knode_cosserat"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.dirname(HERE))

import numpy as np

import cosserat_ode as ref_ode  # noqa: E402  (reference)
import knode as ref_knode  # noqa: E402
import physics_controls as ref_ctl  # noqa: E402
from base_motion_cases import CASES, SHAPES, base_history  # noqa: E402  (the histories: one definition for generator and tests)


class FsolveSpy:
    def __init__(self):
        from scipy.optimize import fsolve
        self._f = fsolve
        self.ier = []

    def __call__(self, fun, x0, args=()):
        x, info, ier, _ = self._f(fun, x0, args=args, full_output=True)
        self.ier.append(ier)
        return x


def moved_controls(r, ctl, base):
    """yields control t with the base of step t assigned first (None: the base is left alone)"""
    for t, c in enumerate(ctl):
        if base is not None:
            r.p0 = np.array(base[t, 0:3], dtype=np.float64)
            r.h0 = np.array(base[t, 3:7], dtype=np.float64)
            r.q0 = np.array(base[t, 7:10], dtype=np.float64)
            r.w0 = np.array(base[t, 10:13], dtype=np.float64)
        yield c


def run(N, ctl, base):
    r = ref_ode.CosseratRod(use_fsolve=True)
    ref_knode.setup_robot(r, None)
    r.N = N
    r.compute_intermediate_terms()
    spy = FsolveSpy()
    old = ref_knode.fsolve
    ref_knode.fsolve = spy
    try:
        with np.errstate(all="ignore"):
            traj = ref_knode.simulate(r, moved_controls(r, ctl, base))
    finally:
        ref_knode.fsolve = old
    return traj[:, :25], np.array(spy.ier)


def main():
    out = {"cases": np.array(CASES)}
    converged = True
    for N, T in SHAPES:
        ctl = np.array(ref_ctl.calc_controls("sine", 1.0, 0.05, T), dtype=np.float64)
        base = np.stack([base_history(c, T) for c in CASES])
        trajs, iers = zip(*(run(N, ctl, base[k]) for k in range(len(CASES))))
        trajs, iers = np.stack(trajs), np.stack(iers)
        still, ier0 = run(N, ctl, None)
        k = f"_n{N}"
        out.update({"ctl" + k: ctl, "base" + k: base, "tips" + k: trajs[:, :, :3, -1], "last" + k: trajs[:, -1],
                    "ier" + k: iers, "tips_unmoved" + k: still[:, :3, -1], "last_unmoved" + k: still[-1], "ier_unmoved" + k: ier0})
        if N == 10:
            out["traj" + k] = trajs
        ok = bool((iers == 1).all() and (ier0 == 1).all())
        converged = converged and ok
        print(f"  N = {N}, T = {T}: ier all 1: {ok}")
    if not converged:
        sys.exit("fsolve did not converge on every step: nothing written")
    path = os.path.join(HERE, "base_motion.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote base_motion.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
