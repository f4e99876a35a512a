"""Writes tests/golden/sweep_counts.npz: the oracle's Newton iterations per step, with the MLP off, for every cell of
tests/sweep_count_cases.py - the exact Jacobian and start rule and every mutant of either.  Nothing here needs the
reference or a GPU: the counts are those of ``mlp_shape_cases.newton_steps`` (``cosserat_oracle.newton_shoot``).

    python tests/golden/make_golden_sweep_counts.py [processes]

Per Jacobian cell ``jac_<scheme>_<pset>_n<N>_<dtype>``: ``_iters`` int16 [1 + mutants][B][T_JAC] (row 0 exact, then
JAC_MUTANTS[scheme]) and ``_dev`` float64 [1 + mutants][B], the largest relative distance of a stored state from the exact
run's (inf: a step of the mutant did not converge within 50 iterations, which then counts 50).  Per start cell
``start_<scheme>_<pset>_n<N>``: the same with the rows START_ROWS, T_START steps.  The script refuses to write unless
every exact run converged at every step and every converged mutant kept the root (``ROOT_TOL``)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the oracle on the path)
import sweep_count_cases as cc  # noqa: E402


def jac_cell(cell):
    scheme, pset, N, dtype = cell
    names = (None,) + cc.JAC_MUTANTS[scheme]
    iters = np.zeros((len(names), cc.B, cc.T_JAC), np.int16)
    dev = np.zeros((len(names), cc.B))
    for b in range(cc.B):
        with np.errstate(all="ignore"):
            runs = [cc.run(pset, scheme, N, b, dtype, "jac", m) for m in names]
        assert all(runs[0]["ok"]), (cell, b)
        for k, r in enumerate(runs):
            iters[k, b] = r["iters"]
            dev[k, b] = cc.root_deviation(r, runs[0])
    return cc.jac_key(*cell), iters, dev


def start_cell(cell):
    scheme, pset, N = cell
    iters = np.zeros((len(cc.START_ROWS), cc.B, cc.T_START), np.int16)
    dev = np.zeros((len(cc.START_ROWS), cc.B))
    spec = {"rule0": (0, None), "rule1": (1, None), "rule2": (2, None), "sign1": (1, "sign"), "sign2": (2, "sign"),
            "zero": (2, "zero")}
    for b in range(cc.B):
        with np.errstate(all="ignore"):
            runs = [cc.run(pset, scheme, N, b, "f64", "start", spec[r][1], spec[r][0]) for r in cc.START_ROWS]
        assert all(all(r["ok"]) for r in runs[:3]), (cell, b)
        for k, r in enumerate(runs):
            iters[k, b] = r["iters"]
            dev[k, b] = cc.root_deviation(r, runs[0])
    return cc.start_key(*cell), iters, dev


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    out = {}
    with multiprocessing.Pool(procs) as pool:
        jobs = [pool.apply_async(jac_cell, (c,)) for c in cc.jac_cells()] + [pool.apply_async(start_cell, (c,)) for c in cc.start_cells()]
        for j in jobs:
            key, iters, dev = j.get()
            tol = cc.ROOT_TOL["f32" if key.endswith("f32") else "f64"]
            ok = np.isfinite(dev)
            assert np.all(dev[ok] <= tol), (key, dev)
            print(f"{key}: sums {iters.sum(axis=2).tolist()} worst deviation {dev[ok].max():.1e}"
                  f"{'' if ok.all() else ' (not converged: ' + str(np.argwhere(~ok).tolist()) + ')'}", flush=True)
            out[key + "_iters"], out[key + "_dev"] = iters, dev
    np.savez_compressed(os.path.join(HERE, "sweep_counts.npz"), **out)


if __name__ == "__main__":
    main()
