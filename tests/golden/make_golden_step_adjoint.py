"""Writes tests/golden/step_adjoint.npz: finite-difference gradients of the oracle's own step and rollout
(tests/step_adjoint_cases.py: cosserat_oracle.residual_euler + newton_shoot, solved to step_adjoint_cases.ORACLE_TOL), each at two step sizes.

    python tests/golden/make_golden_step_adjoint.py [processes] [only]

`only` (e.g. "_N33_"): compute just the cases whose key holds that text and merge them into the existing file - every case
is deterministic on its own, so the merged file is the one a full run writes.

Step cases: key <set>_N<N>_<state>_r<rod>_: prev, cur, next [N, 28], tens [4], gbar [3, N, 28], fd_h / fd_2h
[3, 24 N + 23] = d <gbar_c, next> / d x, x = [cur[N, 12], prev[N, 12], tensions[4], bnd[19]].
Rollout cases: key roll_<set>_N<N>_T<T>_: ctl [T, 4], gbar [2, T + 1, N, 28], fd_h / fd_2h [2, 4 T + 19 + 36] =
d sum_t <gbar_c[t], states[t]> / d [ctl, bnd, chosen entries of states[0]].
About 90 CPU-minutes (N = 100 and 130 carry most of it)."""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import step_adjoint_cases as sc  # noqa: E402

_W = {}


def _step_base(case):
    ps, N, rod, state = case
    P = sc.params(ps, N)
    prev, cur, tens = sc.step_inputs(ps, N, rod, state)
    x = sc.x_of(cur, prev, tens, sc.bnd_of(P))
    nxt, G = sc.oracle_step(P, x, np.zeros(6))
    return P, x, nxt, G, prev, cur, tens


def _step_task(arg):
    case, idx = arg
    if case not in _W:
        _W[case] = _step_base(case)
    P, x, nxt, G = _W[case][:4]
    N = int(P.N)
    gb = sc.cotangents(N, 100 + N).reshape(3, -1)
    fn = lambda xx: gb @ sc.oracle_step(P, xx, G)[0].ravel()
    return case, idx, sc.fd_columns(fn, x, idx, sc.H), sc.fd_columns(fn, x, idx, 2 * sc.H)


def _roll_setup(case):
    ps, N, T = case
    P = sc.params(ps, N)
    ctl = sc.orc.batch_sine_controls(1, T, P.del_t, 11)[0]
    s0 = sc.straight_state(P)
    ent = sc.rollout_state0_entries(N)
    x = np.concatenate([ctl.ravel(), sc.bnd_of(P), [s0[j, s] for j, s in ent]])
    gb = sc.rollout_cotangents(T, N, 200 + N + T).reshape(2, -1)

    def fn(xx):
        st = s0.copy()
        for (j, s), v in zip(ent, xx[4 * T + 19:]):
            st[j, s] = v
        return gb @ sc.oracle_rollout(P, xx[:4 * T].reshape(T, 4), st, bnd=xx[4 * T:4 * T + 19]).ravel()
    return x, fn, ctl


def _roll_task(arg):
    case, idx = arg
    if case not in _W:
        _W[case] = _roll_setup(case)
    x, fn, _ = _W[case]
    return case, idx, sc.fd_columns(fn, x, idx, sc.H), sc.fd_columns(fn, x, idx, 2 * sc.H)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else os.cpu_count()
    only = sys.argv[2] if len(sys.argv) > 2 else None
    path = os.path.join(HERE, "step_adjoint.npz")
    out = {"H": np.array(sc.H)}
    step_cases = [(ps, N, rod, state) for ps, N, rods, state in sc.STEP_CASES for rod in range(rods)]
    roll_cases = list(sc.ROLLOUT_CASES)
    if only is not None:
        with np.load(path) as old:
            out = {k: old[k] for k in old.files}
        assert float(out["H"]) == sc.H
        step_cases = [c for c in step_cases if only in sc.case_key(c[0], c[1], c[3]) + f"_r{c[2]}_"]
        roll_cases = [c for c in roll_cases if only in f"roll_{c[0]}_N{c[1]}_T{c[2]}_"]
    tasks = []
    for case in step_cases:
        n = 24 * case[1] + 23
        tasks += [(case, list(range(i, min(i + 16, n)))) for i in range(0, n, 16)]
    rtasks = []
    for case in roll_cases:
        n = 4 * case[2] + 19 + len(sc.rollout_state0_entries(case[1]))
        rtasks += [(case, list(range(i, min(i + 4, n)))) for i in range(0, n, 4)]
    tasks.sort(key=lambda t: -t[0][1])  # the long rods first
    with mp.get_context("fork").Pool(procs) as pool:
        got = {}
        for case, idx, a, b in pool.imap_unordered(_step_task, tasks):
            got.setdefault(case, {})[idx[0]] = (a, b)
        rgot = {}
        for case, idx, a, b in pool.imap_unordered(_roll_task, rtasks):
            rgot.setdefault(case, {})[idx[0]] = (a, b)
    for case in step_cases:
        ps, N, rod, state = case
        P, x, nxt, G, prev, cur, tens = _step_base(case)
        k = sc.case_key(ps, N, state) + f"_r{rod}_"
        parts = [got[case][i] for i in sorted(got[case])]
        out[k + "prev"], out[k + "cur"], out[k + "next"], out[k + "tens"] = prev, cur, nxt, tens
        out[k + "gbar"] = sc.cotangents(N, 100 + N)
        out[k + "fd_h"] = np.concatenate([p[0] for p in parts]).T
        out[k + "fd_2h"] = np.concatenate([p[1] for p in parts]).T
    for case in roll_cases:
        ps, N, T = case
        k = f"roll_{ps}_N{N}_T{T}_"
        parts = [rgot[case][i] for i in sorted(rgot[case])]
        out[k + "ctl"] = _roll_setup(case)[2]
        out[k + "gbar"] = sc.rollout_cotangents(T, N, 200 + N + T)
        out[k + "fd_h"] = np.concatenate([p[0] for p in parts]).T
        out[k + "fd_2h"] = np.concatenate([p[1] for p in parts]).T
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main()
