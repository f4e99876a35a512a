#!/usr/bin/env python3
"""Generate tests/golden/rk4_sweeps.npz by IMPORTING THE REFERENCE (like make_golden_full_matrices.py: runs only where the
reference is; the fixture is data only - inputs and the reference's outputs on them).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rk4_sweeps.py

RK4 sweeps over time steps.  knode.simulate hard-codes the Euler residual (knode.py:89), so the rod's ``getResidualEuler``
is pointed at its own ``getResidualRK4`` for the duration of a run, as make_golden.py does; no reference code is changed.
The parameter sets are "full-asym" and its diagonal twin of tests/full_matrix_cases.py, assigned to the None preset's rod
(``Bse`` and ``Bbt`` are plain attributes, cosserat_ode.py:22-23).  fsolve is wrapped to record ier, which the reference
discards.  Every run of ``rk4_cases.FIXTURE_RUNS`` must be solved (``ier == 1`` at every step: asserted here).

One more run is kept for what it does NOT do: the None preset itself at N = 9, which the reference does not solve under
RK4 (``ier = 5`` from step 2 on) - the reason why no RK4 test uses the preset on a coarse grid.  Tips and ``ier`` only.

The reference drops its last solve (knode.py:102): T controls give entries 0 .. T-1.

Arrays, per run (variant, N, T, kind) with key prefix ``{full|twin}_n{N}_{kind}_``: ``ctl`` [T, 4], ``tips`` [T, 3],
``ier`` [T], ``entries`` [k] (every fourth entry and the last) and ``states`` [k, 25, N] at them; ``preset_n9_sine_ctl`` /
``_tips`` / ``_ier``; and the matrices of "full-asym", ``Bse`` and ``Bbt``."""
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

# the project's own case modules come last on the path: they must not shadow the reference's modules of the same names
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.append(_p)
import full_matrix_cases as fm  # noqa: E402
import rk4_cases as rk  # noqa: E402


class FsolveSpy:
    def __init__(self):
        from scipy.optimize import fsolve
        self._f = fsolve
        self.ier = []

    def __call__(self, fun, x0, args=()):
        x, info, ier, _ = self._f(fun, x0, args=args, full_output=True)
        self.ier.append(ier)
        return x


def run(N, ctl, variant):
    """``variant`` None: the preset as it is."""
    r = ref_ode.CosseratRod(use_fsolve=True)
    ref_knode.setup_robot(r, None)
    r.N = N
    if variant is None:
        r.compute_intermediate_terms()
    else:
        fm.apply_to_rod(r, variant)
    spy = FsolveSpy()
    old = ref_knode.fsolve
    ref_knode.fsolve = spy
    r.getResidualEuler = r.getResidualRK4  # (an attribute of this one rod, dropped with it)
    try:
        with np.errstate(all="ignore"):
            traj = ref_knode.simulate(r, ctl)
    finally:
        ref_knode.fsolve = old
    return traj[:, :25], np.array(spy.ier)


def controls(T, kind):
    ctl = np.array(ref_ctl.calc_controls("sine", 1.0, fm.DEL_T, T), dtype=np.float64)
    if kind == "jump":
        ctl[T // 2:, 0] += 0.5
    assert np.array_equal(ctl, fm.controls(T, kind))
    return ctl


def main():
    Bse, Bbt = fm.matrices("full-asym")
    out = {"Bse": Bse, "Bbt": Bbt}
    for variant, N, T, kind in rk.FIXTURE_RUNS:
        ctl = controls(T, kind)
        traj, ier = run(N, ctl, variant)
        assert traj.shape == (T, 25, N) and ier.shape == (T,)
        entries = fm.fixture_entries(T)
        k = rk.fixture_key(variant, N, kind) + "_"
        out.update({k + "ctl": ctl, k + "tips": traj[:, :3, -1], k + "ier": ier, k + "entries": np.array(entries),
                    k + "states": traj[entries]})
        print(f"  {variant}, N = {N}, T = {T}, {kind}: ier all 1: {bool((ier == 1).all())}")
        assert (ier == 1).all()
    N, T, kind = rk.PRESET_RUN
    ctl = controls(T, kind)
    traj, ier = run(N, ctl, None)
    print(f"  None preset, N = {N}, T = {T}: ier {ier.tolist()}")
    assert (ier != 1).any()
    out.update({"preset_n9_sine_ctl": ctl, "preset_n9_sine_tips": traj[:, :3, -1], "preset_n9_sine_ier": ier})
    path = os.path.join(HERE, "rk4_sweeps.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote rk4_sweeps.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
