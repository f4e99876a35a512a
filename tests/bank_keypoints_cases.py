"""Shared by tests/test_bank_keypoints_cpu.py and tests/test_gpu_bank_keypoints.py (not a test module): the rods of the
bank key-point tests - a model variant, a base history (tests/base_motion_cases.py), a load history
(tests/tip_loads_cases.py) and a network of a bank (tests/mlp_bank_cases.py) each - and the oracle's time loop with a
network, a base state and a tip wrench per step.  Every reference is computed once per process by the oracle's tightly
converged Newton solver, asserts that every step converged and is handed out read-only."""
import copy
import functools

import numpy as np

import mlp_bank_cases as banks
from base_motion_cases import base_history
from tip_loads_cases import load_history

# (mod, base history, load history, network; -1 = the bank's last).  Every combination converges at every step on the CPU
# oracle (newton_shoot, tol 1e-12) in 4 to 5 iterations with the controls of bc.npz and both banks of mlp_bank_cases.
ROWS = ((None, "slide", "sine", 0), ("damping", "tilt", "alt", 1), ("short", "alt", "jump", 2), ("youngs", "jump", "const", -1),
        ("noair", "still", "sine", 1), ("nsw", "alt", "alt", 0))
# N = 20: the sixteen points of the MLP-on key-point tests (both ends and their neighbours, ragged gaps); N = 100: both
# words of the mask and both sides of their boundary
POINTS = {20: [0, 1, 2, 3, 5, 6, 8, 9, 10, 12, 13, 15, 16, 17, 18, 19], 100: [0, 63, 64, 99], 10: list(range(10))}
CASE_SMALL = dict(N=20, T=13, rows=ROWS)
CASE_N100 = dict(N=100, T=8, rows=ROWS[:2])
# the rods of tests/golden/bank_motion.npz (tests/golden/make_golden_bank_motion.py): rows 1, 2, 3 and 5 at N = 10, T = 12
FIXTURE = dict(N=10, T=12, rows=(ROWS[0], ROWS[1], ROWS[2], ROWS[4]), bank=2)


def bank(which):
    return banks.bank_three() if which == 3 else banks.bank_two()


def net_index(which, k):
    return k % len(bank(which))


def nets_of(case, which):
    return [net_index(which, r[3]) for r in case["rows"]]


def bnd_of(case):
    """bnd[B, T, 19] of a case: base history, then load history, per rod"""
    T = case["T"]
    return np.stack([np.hstack([base_history(r[1], T), load_history(r[2], T)]) for r in case["rows"]])


def oracle_loop(P, ctl, base, loads=None, mlp=None, tol=1e-12):
    """base_motion_cases.oracle_loop with ``mlp=`` passed to ``residual_euler``: ``D.y0_head`` / ``D.y0_tail`` (and, with
    ``loads``, ``D.P.F_tip`` / ``D.P.M_tip``) assigned before the solve of step t, the network inside every sweep.  ALL T
    steps are solved: returns ``(states[T + 1, 25, N], ok[T], iterations[T])``, entry 0 the straight rod."""
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
        G, ok, it = orc.newton_shoot(lambda g: orc.residual_euler(D, g, y, z, yh, zh, tensions, mlp=mlp), G, tol=tol)
        oks.append(ok)
        its.append(it)
        out.append(np.vstack([y, z]))
    return np.array(out), np.array(oks), np.array(its)


@functools.lru_cache(maxsize=None)
def oracle_rod(N, T, mod, base, load, which, k):
    """float64[T + 1, 25, N] of one rod; ``which`` = 3 / 2 names the bank, k the network in it (None: no network)"""
    import cosserat_oracle as orc
    mlp = None if k is None else bank(which)[k]
    ref, ok, it = oracle_loop(orc.setup_params(mod, N), banks.controls(T), base_history(base, T), load_history(load, T), mlp=mlp)
    assert np.all(ok), (N, T, mod, base, load, which, k, ok)
    ref = np.ascontiguousarray(ref[:, :25])
    ref.setflags(write=False)
    return ref


def oracle_case(case, which):
    return [oracle_rod(case["N"], case["T"], r[0], r[1], r[2], which, net_index(which, r[3])) for r in case["rows"]]
