"""Writes tests/golden/table_adjoint.npz: finite-difference gradients of the oracle's own rollouts of a heterogeneous batch
(tests/table_adjoint_cases.py) - three rods, `plain`, `bc`, `noair`, at N = 9, each with its own controls and its own boundary
history bnd[t] - computed on the CPU from the oracle alone.

    python tests/golden/make_golden_table_adjoint.py [processes]

Per rod and case (key <set>_<case>_; cases T1, T3, and T3p = T = 3 continued from two steps with a prev_init): the inputs ctl,
bnd, state0, prev_init, the cotangents gbar [2, T + 1, N, 28] and the oracle's states; x_fd_h / x_fd_2h [2, len(x)] = the
central differences of sum_t <gbar_c[t], states[t]> at H and 2 H in x = [ctl, bnd, entries of states[0], entries of prev_init]
(table_adjoint_cases.x_of; the state entries at H_STATE) with x_floor [2, 2] (cotangent; ctl and bnd, state entries);
par_fd_h / par_fd_2h [2, 43], par_rung, par_floor [2, 10] = the same in the 43 material parameters at the rung of param_adjoint_cases' ladder that resolves each block best, states[0] and prev_init held
fixed.  N = 9 resolved every block; no case fell back to N = 10.
The generator does not write the fixture if a block's tolerance (ten times the H / 2 H disagreement plus the quotient's floor)
exceeds MAX_REL_TOL = 1e-2 of the block, and an oracle solve that misses 1e-15 raises.  About two minutes on 8 cores."""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import param_adjoint_cases as pc  # noqa: E402
import step_adjoint_cases as sc  # noqa: E402
import table_adjoint_cases as tc  # noqa: E402


def _x_task(arg):
    b, case, idx = arg
    rc = tc.rod_case(b, case)
    x = tc.x_of(rc)
    fn = lambda xx: tc.loss_of_x(rc, xx)
    h = tc.x_step(idx[0], rc["T"])  # (a chunk never straddles the two kinds of entries)
    assert h == tc.x_step(idx[-1], rc["T"])
    return ("x", b, case, idx[0]), (sc.fd_columns(fn, x, idx, h), sc.fd_columns(fn, x, idx, 2 * h))


def _par_task(arg):
    b, case, name = arg
    rc = tc.rod_case(b, case)
    x, P = tc.x_of(rc), rc["P"]
    fn = lambda Pt: tc.loss_of_x(rc, x, P=Pt)
    off, n = next((o, c) for nm, o, c, _ in pc.PAR_BLOCKS if nm == name)
    s = pc.scales_of(P)
    est = {}
    for H in pc.ladder_of(name):
        est[H] = (pc.fd_theta(fn, P, range(off, off + n), H).T, pc.fd_theta(fn, P, range(off, off + n), 2 * H).T, float(s[off]))
    return ("p", b, case, name), est


def _floor_task(arg):
    b, case = arg
    rc = tc.rod_case(b, case)
    return ("f", b, case, 0), tc.solve_floor(rc, rc["gbar"].reshape(2, -1))


def _task(t):
    return {"x": _x_task, "p": _par_task, "f": _floor_task}[t[0]](t[1:])


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else os.cpu_count()
    tasks = []
    for b in range(3):
        for case, (T, with_prev) in tc.CASES.items():
            n = 23 * T + len(tc.entries()) * (2 if with_prev else 1)
            tasks += [("p", b, case, name) for name in ("Bse", "tendon_dirs", "Bbt", "C")]
            tasks += [("x", b, case, list(range(i, min(i + 12, e)))) for s, e in ((0, 23 * T), (23 * T, n)) for i in range(s, e, 12)]
            tasks += [("p", b, case, name) for name in pc.BLOCK_NAMES if name not in ("Bse", "tendon_dirs", "Bbt", "C")]
            tasks.append(("f", b, case))
    tasks.sort(key=lambda t: -tc.CASES[t[2]][0])  # the long cases first
    got = {}
    with mp.get_context("fork").Pool(procs) as pool:
        for k, v in pool.imap_unordered(_task, tasks):
            got[k] = v
    out, bad = {"H": np.array(sc.H)}, []
    for b in range(3):
        for case, (T, with_prev) in tc.CASES.items():
            rc, k = tc.rod_case(b, case), tc.key(b, case)
            parts = [got[key] for key in sorted(kk for kk in got if kk[:3] == ("x", b, case))]
            fd_h, fd_2h = np.concatenate([p[0] for p in parts]).T, np.concatenate([p[1] for p in parts]).T
            solve1 = got[("f", b, case, 0)]
            xfl = np.array([tc.x_floor(rc, c, solve1) for c in range(2)])
            floors1 = [pc.unit_floor(rc["gbar"][c], rc["states"]) + solve1[c] for c in range(2)]
            est = {name: got[("p", b, case, name)] for name in pc.BLOCK_NAMES}
            p_h, p_2h, rung, pfl = pc.choose_rungs(est, floors1)
            for c in range(2):
                for name, idx in tc.x_blocks(T, with_prev):
                    a, bb = fd_h[c][idx], fd_2h[c][idx]
                    if not np.any(a) and not np.any(bb): continue
                    tol, size = sc.block_tol(a, bb, tc._floor_of(name, xfl[c])), float(np.max(np.abs(a)))
                    print(f"{k} cot {c} {name:18s} tol {tol:.2e} size {size:.2e} rel {tol / size:.1e}")
                    if tol > tc.MAX_REL_TOL * size: bad.append((k, c, name, tol, size))
                for name, err, tol, size, zero in pc.block_report(p_h[c], p_h[c], p_2h[c], pfl[c]):
                    print(f"{k} cot {c} {name:18s} tol {tol:.2e} size {size:.2e} rel {tol / max(size, 1e-300):.1e} rung {rung[c][pc.BLOCK_NAMES.index(name)]:g}")
                    if not zero and tol > tc.MAX_REL_TOL * size: bad.append((k, c, name, tol, size))
            out.update({k + "ctl": rc["ctl"], k + "bnd": rc["bnd"], k + "state0": rc["state0"], k + "gbar": rc["gbar"], k + "states": rc["states"],
                        k + "x_fd_h": fd_h, k + "x_fd_2h": fd_2h, k + "x_floor": xfl, k + "par_fd_h": p_h, k + "par_fd_2h": p_2h,
                        k + "par_rung": rung, k + "par_floor": pfl})
            if with_prev: out[k + "prev_init"] = rc["prev_init"]
    if bad:
        for row in bad: print("UNRESOLVED", row)
        sys.exit("blocks above MAX_REL_TOL: the fixture is not written")
    path = os.path.join(HERE, "table_adjoint.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
