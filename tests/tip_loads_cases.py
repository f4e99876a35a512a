"""Shared by tests/test_tip_loads_cpu.py and tests/test_gpu_tip_loads.py: the four load histories of
tests/golden/tip_loads.npz (written by tests/golden/make_golden_tip_loads.py from the unmodified reference) and the
oracle's time loop with a tip wrench per step."""
import copy

import numpy as np

CASES = ("const", "jump", "alt", "sine")
SHAPES = ((10, 12), (23, 13))  # (N, T) of the fixture


def load_history(case, T):
    """[T, 6] = F_tip (3), M_tip (3) of step t = 0 .. T-1 (the formulas of the fixture's generator)"""
    t = np.arange(T, dtype=np.float64)
    L = np.zeros((T, 6))
    if case == "const":
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


def oracle_loop(P, ctl, loads, tol=1e-12):
    """knode.simulate's loop from the oracle's own pieces (straight_state, residual_euler, newton_shoot) with
    ``D.P.F_tip`` / ``D.P.M_tip`` assigned before the solve of step t.  ALL T steps are solved: returns
    ``(states[T + 1, 25, N], ok[T], iterations[T])``, entry 0 the straight rod, entry t + 1 the state after step t."""
    import cosserat_oracle as orc
    D = copy.deepcopy(P).derived()
    y, z = orc.straight_state(D)
    y_prev, z_prev = y.copy(), z.copy()
    G = np.zeros(6)
    out, oks, its = [np.vstack([y, z])], [], []
    for tensions, w in zip(np.asarray(ctl, float), np.asarray(loads, float)):
        D.P.F_tip, D.P.M_tip = w[:3].copy(), w[3:].copy()
        yh = D.c1 * y + D.c2 * y_prev
        zh = D.c1 * z + D.c2 * z_prev
        y_prev, z_prev = y.copy(), z.copy()
        G, ok, it = orc.newton_shoot(lambda g: orc.residual_euler(D, g, y, z, yh, zh, tensions), G, tol=tol)
        oks.append(ok)
        its.append(it)
        out.append(np.vstack([y, z]))
    return np.array(out), np.array(oks), np.array(its)
