"""Writes tests/golden/bank_adjoint.npz: finite-difference gradients of the oracle's own rollout of a heterogeneous batch with
the residual MLP on and a network per rod (tests/bank_adjoint_cases.py) - B = 5 rods at N = 9 over T = 4 steps, three parameter
rows, each rod its own controls and boundary history, K = 3 networks with net_of_rod = [1, 0, 1, 1, 0] - once per kernel family
of the input Jacobian (tanh17, softplus33x20), computed on the CPU from the oracle alone.

    python tests/golden/make_golden_bank_adjoint.py [processes]

Networks: net_<family>_<k>_W<l> / _b<l> (fp32) and net_<family>_acts - the fixture carries the weights it was computed with.
Per family and rod (key <family>_r<b>_): ctl, bnd, state0, gbar [2, T + 1, N, 28], the oracle's states [T + 1, N, 28];
x_fd_h / x_fd_2h [2, len(x)] = the central differences of sum_t <gbar_c[t], states[t]> at H and 2 H in x = [ctl, bnd, entries of
states[0]] (the state entries at H_STATE) and x_tol [2, blocks] = the tolerance of every block of
table_adjoint_cases.x_blocks (0: the block is exactly zero); per step t of STEP_TS: s<t>_gbar [3, N, 28], s<t>_fd_h / _fd_2h
[3, 24 N + 23] = d <gbar_c, states[t + 1]> / d [cur, prev (at H_STATE), tensions, bnd[t]] and s<t>_tol [3, blocks of step_adjoint_cases.BLOCKS].
Per family and network with rods (key <family>_net<k>_): wfd_h / wfd_2h [2, dirs] = the same rollout differences along
nn_adjoint_cases.weight_directions, the loss summed over the network's rods, w_tol [2, layers]; s<t>_wfd_h / _wfd_2h [3, dirs],
s<t>_w_tol [3, layers] for the single steps.
The generator does not write the fixture if a block's tolerance (ten times the H / 2 H disagreement plus
step_adjoint_cases.fd_floor) exceeds MAX_REL_TOL = 1e-2 of the block, and an oracle solve that misses 1e-15 raises."""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bank_adjoint_cases as bc  # noqa: E402
import nn_adjoint_cases as nc  # noqa: E402
import step_adjoint_cases as sc  # noqa: E402

CHUNK = 12


def _step_fn(fam, b, t, m=None):
    rc = bc.rod_case(fam, b)
    x, _, G = bc.step_inputs(rc, t)
    gb = rc["gstep"].reshape(3, -1)
    return x, (lambda xx, mm=None: gb @ nc.oracle_step_nn(rc["P"], mm if mm is not None else rc["mlp"], xx, G)[0].ravel())


def _task(arg):
    kind = arg[0]
    if kind == "x":
        _, fam, b, idx = arg
        rc = bc.rod_case(fam, b)
        x, fn = bc.x_of(rc), (lambda xx: bc.loss_of_x(rc, xx))
        h = bc.x_step(idx[0], rc["T"])
        assert h == bc.x_step(idx[-1], rc["T"])  # (a chunk never straddles the two kinds of entries)
        return arg[:3] + (idx[0],), (idx, sc.fd_columns(fn, x, idx, h), sc.fd_columns(fn, x, idx, 2 * h))
    if kind == "w":
        _, fam, k, idx = arg
        mlp = bc.networks(fam)[k]
        fn = lambda m: bc.weight_loss(fam, k, m)
        dirs = nc.weight_directions(mlp)[idx]
        return arg[:3] + (idx[0],), (idx, nc.weight_fd(fn, mlp, dirs, sc.H), nc.weight_fd(fn, mlp, dirs, 2 * sc.H))
    if kind == "sx":
        _, fam, b, t, idx = arg
        x, fn = _step_fn(fam, b, t)
        h = bc.step_h(idx[0])
        assert h == bc.step_h(idx[-1])
        return arg[:4] + (idx[0],), (idx, sc.fd_columns(fn, x, idx, h), sc.fd_columns(fn, x, idx, 2 * h))
    _, fam, k, t, idx = arg  # "sw"
    mlp = bc.networks(fam)[k]
    fns = [_step_fn(fam, b, t) for b in bc.rods_of(k)]
    fn = lambda m: sum(f(x, m) for x, f in fns)
    dirs = nc.weight_directions(mlp)[idx]
    return arg[:4] + (idx[0],), (idx, nc.weight_fd(fn, mlp, dirs, sc.H), nc.weight_fd(fn, mlp, dirs, 2 * sc.H))


def _chunks(lo, hi):
    return [list(range(i, min(i + CHUNK, hi))) for i in range(lo, hi, CHUNK)]


def _gather(got, prefix, n, width):
    a, b = np.zeros((n, width)), np.zeros((n, width))
    for k in got:
        if k[:len(prefix)] == prefix:
            idx, u, v = got[k]
            a[idx], b[idx] = u, v
    return a.T, b.T


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else os.cpu_count()
    T, N, nx = bc.T_FIX, bc.N_FIX, 23 * bc.T_FIX + len(bc.entries())
    nets_with_rods = [k for k in range(bc.K_FIX) if bc.rods_of(k)]
    tasks = []
    for fam in bc.FAMILIES:
        nd = 6 * (len(nc.NETWORKS[fam][0]) + 1)
        for b in range(bc.B_FIX):
            tasks += [("x", fam, b, idx) for lo, hi in ((0, 23 * T), (23 * T, nx)) for idx in _chunks(lo, hi)]
            tasks += [("sx", fam, b, t, idx) for t in bc.STEP_TS for idx in _chunks(0, 24 * N + 23)]
        for k in nets_with_rods:
            tasks += [("w", fam, k, idx) for idx in _chunks(0, nd)]
            tasks += [("sw", fam, k, t, idx) for t in bc.STEP_TS for idx in _chunks(0, nd)]
    tasks.sort(key=lambda t: 0 if t[0] in ("x", "w") else 1)  # the rollouts first
    got = {}
    with mp.get_context("fork").Pool(procs) as pool:
        for k, v in pool.imap_unordered(_task, tasks):
            got[k] = v
    out, bad = {"H": np.array(sc.H), "H_STATE": np.array(bc.H_STATE), "net_of_rod": np.array(bc.NET_OF_ROD, np.int32),
                "row_of_rod": np.array(bc.ROW_OF_ROD, np.int32)}, []

    def report(tag, names, fd, tols):
        for name, a, tol in zip(names, fd, tols):
            size = float(np.max(np.abs(a)))
            print(f"{tag} {name:18s} tol {tol:.2e} size {size:.2e} rel {tol / size if size else 0.0:.1e}" + ("" if tol else " (exactly zero)"))
            if tol > bc.MAX_REL_TOL * size: bad.append((tag, name, tol, size))

    for fam in bc.FAMILIES:
        mlps = bc.networks(fam)
        for k, mlp in enumerate(mlps):
            for l, (W, b) in enumerate(zip(mlp.weights, mlp.biases)):
                out[f"net_{fam}_{k}_W{l}"], out[f"net_{fam}_{k}_b{l}"] = W, b
        out[f"net_{fam}_acts"] = np.array(mlps[0].acts, dtype=np.int32)
        nd, nl = 6 * len(mlps[0].weights), len(mlps[0].weights)
        xb = bc.x_blocks(T, False)
        for b in range(bc.B_FIX):
            rc, kb = bc.rod_case(fam, b), bc.key(fam, b)
            fd_h, fd_2h = _gather(got, ("x", fam, b), nx, 2)
            tol = np.array([bc.x_tols(fd_h[c], fd_2h[c], bc.x_floor(rc, c)) for c in range(2)])
            for c in range(2):
                report(f"{kb} cot {c}", [n for n, _ in xb], [fd_h[c][i] for _, i in xb], tol[c])
            out.update({kb + "ctl": rc["ctl"], kb + "bnd": rc["bnd"], kb + "state0": rc["state0"], kb + "gbar": rc["gbar"],
                        kb + "states": rc["states"], kb + "x_fd_h": fd_h, kb + "x_fd_2h": fd_2h, kb + "x_tol": tol})
            for t in bc.STEP_TS:
                s_h, s_2h = _gather(got, ("sx", fam, b, t), 24 * N + 23, 3)
                stol = np.array([bc.step_tols(s_h[c], s_2h[c], bc.step_floor(rc["gstep"][c], rc["states"][t + 1])) for c in range(3)])
                for c in range(3):
                    a = sc.split_grad(s_h[c], N)
                    report(f"{kb} step {t} cot {c}", [n for n, _, _ in sc.BLOCKS], [a[arr][..., sl] for _, arr, sl in sc.BLOCKS], stol[c])
                out.update({kb + f"s{t}_gbar": rc["gstep"], kb + f"s{t}_fd_h": s_h, kb + f"s{t}_fd_2h": s_2h, kb + f"s{t}_tol": stol})
        for k in nets_with_rods:
            kk = f"{fam}_net{k}_"
            w_h, w_2h = _gather(got, ("w", fam, k), nd, 2)
            wtol = np.array([bc.w_tols(w_h[c], w_2h[c], bc.w_floor(fam, k, c)) for c in range(2)])
            for c in range(2):
                report(f"{kk} cot {c}", [f"weights layer {l}" for l in range(nl)], [w_h[c][6 * l:6 * l + 6] for l in range(nl)], wtol[c])
            out.update({kk + "wfd_h": w_h, kk + "wfd_2h": w_2h, kk + "w_tol": wtol})
            for t in bc.STEP_TS:
                s_h, s_2h = _gather(got, ("sw", fam, k, t), nd, 3)
                fl = [sum(sc.fd_floor(bc.rod_case(fam, b)["gstep"][c], bc.rod_case(fam, b)["states"][t + 1]) for b in bc.rods_of(k)) for c in range(3)]
                stol = np.array([bc.w_tols(s_h[c], s_2h[c], fl[c]) for c in range(3)])
                for c in range(3):
                    zero = not np.any(s_h[c]) and not np.any(s_2h[c])  # (the pass-through cotangent reaches no network output)
                    if zero: stol[c] = 0.0
                    report(f"{kk} step {t} cot {c}", [f"weights layer {l}" for l in range(nl)], [s_h[c][6 * l:6 * l + 6] for l in range(nl)], stol[c])
                out.update({kk + f"s{t}_wfd_h": s_h, kk + f"s{t}_wfd_2h": s_2h, kk + f"s{t}_w_tol": stol})
    if bad:
        for row in bad: print("UNRESOLVED", row)
        sys.exit("blocks above MAX_REL_TOL: the fixture is not written")
    path = os.path.join(HERE, "bank_adjoint.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
