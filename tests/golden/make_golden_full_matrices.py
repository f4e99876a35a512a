#!/usr/bin/env python3
"""Generate tests/golden/full_matrices.npz by IMPORTING THE REFERENCE (like make_golden_tip_loads.py: runs only where the
reference is; the fixture is data only - inputs and the reference's outputs on them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_full_matrices.py

Full, asymmetric material matrices.  ``Bse`` and ``Bbt`` are plain attributes of the reference's rod
(cosserat_ode.py:22-23) that compute_intermediate_terms folds into the inverses of ``Kse + c0 Bse`` / ``Kbt + c0 Bbt``
(cosserat_ode.py:71-72) and that ODE multiplies the histories by (cosserat_ode.py:150-151): assigning the "full-asym"
matrices of tests/full_matrix_cases.py to the None preset's rod and deriving again gives the reference's answer with no
reference code changed.  fsolve is wrapped to record ier, which the reference discards (knode.py:89).

The reference drops its last solve (knode.py:102): T controls give entries 0 .. T-1.

Arrays, per run (N, T, kind) of ``full_matrix_cases.FIXTURE_RUNS`` with key prefix ``n{N}_{kind}_``: ``ctl`` [T, 4],
``tips`` [T, 3], ``ier`` [T], ``entries`` [k] (every fourth entry and the last) and ``states`` [k, 25, N] at them; and the
matrices themselves, ``Bse`` and ``Bbt``."""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference/knode_cosserat"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)

import numpy as np

import cosserat_ode as ref_ode  # noqa: E402  (reference)
import knode as ref_knode  # noqa: E402
import physics_controls as ref_ctl  # noqa: E402

# the project's own case module: the matrices, the runs and the entries stored.  Its imports (the oracle, the other case
# modules) must not shadow the reference's modules of the same names above, so they come last on the path.
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.append(_p)
import full_matrix_cases as fm  # noqa: E402


class FsolveSpy:
    def __init__(self):
        from scipy.optimize import fsolve
        self._f = fsolve
        self.ier = []

    def __call__(self, fun, x0, args=()):
        x, info, ier, _ = self._f(fun, x0, args=args, full_output=True)
        self.ier.append(ier)
        return x


def run(N, ctl):
    r = ref_ode.CosseratRod(use_fsolve=True)
    ref_knode.setup_robot(r, None)
    r.N = N
    fm.apply_to_rod(r, "full-asym")
    spy = FsolveSpy()
    old = ref_knode.fsolve
    ref_knode.fsolve = spy
    try:
        with np.errstate(all="ignore"):
            traj = ref_knode.simulate(r, ctl)
    finally:
        ref_knode.fsolve = old
    return traj[:, :25], np.array(spy.ier)


def main():
    Bse, Bbt = fm.matrices("full-asym")
    out = {"Bse": Bse, "Bbt": Bbt}
    for N, T, kind in fm.FIXTURE_RUNS:
        ctl = np.array(ref_ctl.calc_controls("sine", 1.0, fm.DEL_T, T), dtype=np.float64)
        if kind == "jump":
            ctl[T // 2:, 0] += 0.5
        assert np.array_equal(ctl, fm.controls(T, kind))
        traj, ier = run(N, ctl)
        assert traj.shape == (T, 25, N) and ier.shape == (T,)
        entries = fm.fixture_entries(T)
        k = fm.fixture_key(N, kind) + "_"
        out.update({k + "ctl": ctl, k + "tips": traj[:, :3, -1], k + "ier": ier, k + "entries": np.array(entries),
                    k + "states": traj[entries]})
        print(f"  N = {N}, T = {T}, {kind}: ier all 1: {bool((ier == 1).all())}")
        assert (ier == 1).all()
    path = os.path.join(HERE, "full_matrices.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote full_matrices.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
