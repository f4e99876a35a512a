"""Shared by tests/test_base_motion_cpu.py and tests/test_gpu_base_motion.py: the five base histories of
tests/golden/base_motion.npz (written by tests/golden/make_golden_base_motion.py from the unmodified reference) and the
oracle's time loop with a base state - and, optionally, a tip wrench - per step."""
import copy

import numpy as np

CASES = ("still", "slide", "tilt", "jump", "alt")
SHAPES = ((10, 12), (23, 13))  # (N, T) of the fixture
DT = 0.05                      # del_t of the presets
UNMOVED = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)  # p0 h0 q0 w0 of the presets


def base_history(case, T):
    """[T, 13] = p0 (3), h0 (4), q0 (3), w0 (3) of step t = 0 .. T-1 (the formulas of the fixture's generator)"""
    t = np.arange(T, dtype=np.float64)
    M = np.tile(UNMOVED, (T, 1))
    if case == "still":  # a constant base that is none of the presets'
        M[:] = [0.01, -0.02, 0.03, 0.98, 0.05, -0.1, 0.02, 0.01, 0.0, -0.02, 0.05, -0.03, 0.02]
    elif case == "slide":  # a carriage: p0.x and its velocity
        om = 2 * np.pi / (8 * DT)
        M[:, 0] = 0.02 * np.sin(om * t * DT)
        M[:, 7] = 0.02 * om * np.cos(om * t * DT)
    elif case == "tilt":  # a platform that rocks about y
        om = 2 * np.pi / (10 * DT)
        th = 0.2 * np.sin(om * t * DT)
        M[:, 3] = np.cos(th / 2)
        M[:, 5] = np.sin(th / 2)
        M[:, 11] = 0.2 * om * np.cos(om * t * DT)
    elif case == "jump":  # from T // 2 on, with a quaternion that is not a unit one
        M[T // 2:, 0] = 0.01
        M[T // 2:, 3:7] = [1.05, 0.0, 0.08, 0.0]
    elif case == "alt":  # another base on every step: tells the two sets of the overlapped kernel apart
        s = (-1.0) ** t
        M[:, 0] = 0.005 * s
        M[:, 1] = -0.002 * s
        M[:, 3] = 1.0
        M[:, 4] = 0.02 * s
        M[:, 12] = 0.1 * s
    else:
        raise ValueError(case)
    return M


def oracle_loop(P, ctl, base, loads=None, tol=1e-12):
    """tip_loads_cases.oracle_loop with ``D.y0_head`` / ``D.y0_tail`` (and, with ``loads``, ``D.P.F_tip`` / ``D.P.M_tip``)
    assigned before the solve of step t.  ALL T steps are solved: returns ``(states[T + 1, 25, N], ok[T], iterations[T])``,
    entry 0 the straight rod of the UNMOVED parameters, entry t + 1 the state after step t."""
    import cosserat_oracle as orc
    D = copy.deepcopy(P).derived()
    y, z = orc.straight_state(D)
    y_prev, z_prev = y.copy(), z.copy()
    G = np.zeros(6)
    out, oks, its = [np.vstack([y, z])], [], []
    base = np.asarray(base, float)
    for t, tensions in enumerate(np.asarray(ctl, float)):
        D.y0_head, D.y0_tail = base[t, :7].copy(), base[t, 7:].copy()
        if loads is not None:
            D.P.F_tip, D.P.M_tip = np.array(loads[t][:3], float), np.array(loads[t][3:], float)
        yh = D.c1 * y + D.c2 * y_prev
        zh = D.c1 * z + D.c2 * z_prev
        y_prev, z_prev = y.copy(), z.copy()
        G, ok, it = orc.newton_shoot(lambda g: orc.residual_euler(D, g, y, z, yh, zh, tensions), G, tol=tol)
        oks.append(ok)
        its.append(it)
        out.append(np.vstack([y, z]))
    return np.array(out), np.array(oks), np.array(its)
