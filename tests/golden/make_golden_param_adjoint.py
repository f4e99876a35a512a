"""Writes tests/golden/param_adjoint.npz: finite-difference gradients of the oracle's own step and rollout with respect to
the 43 material parameters (tests/param_adjoint_cases.py), each block at the rung of the step ladder that resolves it best,
at H and 2 H.

    python tests/golden/make_golden_param_adjoint.py [processes]

Step cases (key <set>_N<N>_<state>_r<rod>_; inputs prev, cur, next, tens are those of step_adjoint.npz) and the slack-tendon
case (key zeroT_<...>: tens and next stored here): fd_h / fd_2h [2, 43] = d <gbar_c, next> / d theta for the first two
cotangents, rung [2, 10] = the relative step kept per block, floor [2, 10] = what the quotient cannot resolve at that step
(its rounding, step_adjoint_cases.fd_floor, plus what the oracle's solve leaves, param_adjoint_cases.solve_floor_step).
Rollout cases (key roll_<set>_N<N>_T<T>_, controls and cotangents those of step_adjoint.npz): the same for
sum_t <gbar_c[t], states[t]>, the straight initial state rebuilt from the perturbed parameters.
The generator does not write the fixture while a block's tolerance exceeds MAX_REL_TOL of its largest entry (such a case is
replaced by another input, or the block's ladder is extended, in param_adjoint_cases.py).  About 35 CPU-minutes."""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import param_adjoint_cases as pc  # noqa: E402
import step_adjoint_cases as sc  # noqa: E402

_G = {}


def _golden():
    if "g" not in _G:
        with np.load(os.path.join(HERE, "step_adjoint.npz")) as g:
            _G["g"] = {k: g[k] for k in g.files}
    return _G["g"]


def _step_task(case):
    kind, ps, N, rod, state = case
    g = _golden()
    k = pc.step_key(ps, N, rod, state)
    P = sc.params(ps, N)
    prev, cur, tens = g[k + "prev"], g[k + "cur"], g[k + "tens"].copy()
    if kind == "zeroT":
        tens[2] = 0.0
    x = sc.x_of(cur, prev, tens, sc.bnd_of(P))
    nxt, G = sc.oracle_step(P, x, np.zeros(6))
    if kind == "step":
        assert np.max(np.abs(nxt - g[k + "next"])) < 1e-12, k
    gb = sc.cotangents(N, 100 + N)[:pc.N_COT]
    fn = lambda Pt: gb.reshape(pc.N_COT, -1) @ sc.oracle_step(Pt, x, G)[0].ravel()
    solve = pc.solve_floor_step(P, x, G, gb.reshape(pc.N_COT, -1))
    floors1 = [pc.unit_floor(gb[c], nxt) + solve[c] for c in range(pc.N_COT)]
    fd_h, fd_2h, rung, floor = pc.fd_ladder(fn, P, floors1)
    key = ("zeroT_" if kind == "zeroT" else "") + k
    out = {key + "fd_h": fd_h, key + "fd_2h": fd_2h, key + "rung": rung, key + "floor": floor}
    if kind == "zeroT":
        out[key + "tens"], out[key + "next"] = tens, nxt
    return key, out


def _roll_task(case):
    ps, N, T = case
    P, ctl, gbar = pc.roll_inputs(ps, N, T)
    states = pc.rollout_of(P, ctl)
    gb = gbar.reshape(2, -1)
    fn = lambda Pt: gb @ pc.rollout_of(Pt, ctl).ravel()
    solve = pc.solve_floor_rollout(P, ctl, gb)
    floors1 = [pc.unit_floor(gbar[c], states) + solve[c] for c in range(2)]
    fd_h, fd_2h, rung, floor = pc.fd_ladder(fn, P, floors1)
    key = pc.roll_key(ps, N, T)
    return key, {key + "fd_h": fd_h, key + "fd_2h": fd_2h, key + "rung": rung, key + "floor": floor}


def _task(t):
    return _step_task(t[1:]) if t[0] == "s" else _roll_task(t[1:])


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else os.cpu_count()
    tasks = [("s", "step", ps, N, rod, state) for ps, N, rods, state in pc.STEP_CASES for rod in range(rods)]
    tasks.append(("s", "zeroT") + pc.ZERO_T_CASE)
    tasks += [("r",) + c for c in pc.ROLLOUT_CASES + [pc.CPU_ROLLOUT_CASE]]
    cost = lambda t: t[3] if t[0] == "s" else t[2] * t[3]
    tasks.sort(key=lambda t: -cost(t))  # the long ones first
    out = {}
    with mp.get_context("fork").Pool(procs) as pool:
        for key, part in pool.imap_unordered(_task, tasks):
            out.update(part)
            print("done", key, flush=True)
    bad = 0
    for k in sorted(out):
        if not k.endswith("fd_h"):
            continue
        base = k[:-4]
        for c in range(out[k].shape[0]):
            for name, err, tol, size, zero in pc.block_report(out[k][c], out[k][c], out[base + "fd_2h"][c], out[base + "floor"][c]):
                if not zero and not tol <= pc.MAX_REL_TOL * size:
                    print(f"UNRESOLVED {base} cot {c} {name}: tol {tol:.2e} size {size:.2e}")
                    bad += 1
    if bad:  # (kept beside the fixture's name for inspection; git ignores nothing here, so it is removed by hand)
        np.savez_compressed(os.path.join(HERE, "param_adjoint_unresolved.npz"), **out)
        sys.exit(f"{bad} blocks are not resolved to {pc.MAX_REL_TOL:g} of their size: the fixture is not written "
                 "(param_adjoint_unresolved.npz holds what was computed)")
    np.savez_compressed(os.path.join(HERE, "param_adjoint.npz"), **out)


if __name__ == "__main__":
    main()
