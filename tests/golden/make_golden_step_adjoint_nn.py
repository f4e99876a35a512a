"""Writes tests/golden/step_adjoint_nn.npz: finite-difference gradients of the oracle's own step and rollout WITH the
residual MLP in the sweep (tests/nn_adjoint_cases.py: cosserat_oracle.residual_euler(..., mlp) + newton_shoot, solved to
step_adjoint_cases.ORACLE_TOL), each at two step sizes H and 2 H, exactly as make_golden_step_adjoint.py does for the physics.

    python tests/golden/make_golden_step_adjoint_nn.py [processes]

Networks: net_<name>_W<k> / _b<k> (fp32) and net_<name>_acts - the fixture carries the weights it was computed with.
Step cases: key <set>_N<N>_<state>_<net>_r<rod>_: prev, cur, next [N, 28], tens [4], gbar [3, N, 28], fd_h / fd_2h
[3, 24 N + 23] = d <gbar_c, next> / d x, x = [cur[N, 12], prev[N, 12], tensions[4], bnd[19]]; wfd_h / wfd_2h [n_dirs, 3] =
d <gbar_c, next> / d theta along nn_adjoint_cases.weight_directions (per layer two dense directions and the four corners of W).
Rollout cases: key roll_<set>_N<N>_T<T>_<net>_: ctl [T, 4], gbar [2, T + 1, N, 28], fd_h / fd_2h [2, 4 T + 19 + 36] =
d sum_t <gbar_c[t], states[t]> / d [ctl, bnd, chosen entries of states[0]]; wfd_h / wfd_2h [n_dirs, 2].
About 15 CPU-minutes."""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nn_adjoint_cases as nc  # noqa: E402
import step_adjoint_cases as sc  # noqa: E402

_W = {}
CHUNK = 24


def _step_base(case):
    ps, N, rod, state, net = case
    P, mlp = sc.params(ps, N), nc.network(net)
    prev, cur, tens = nc.step_inputs_nn(ps, N, rod, state, mlp)
    x = sc.x_of(cur, prev, tens, sc.bnd_of(P))
    nxt, G = nc.oracle_step_nn(P, mlp, x, np.zeros(6))
    return P, mlp, x, nxt, G, prev, cur, tens


def _step_task(arg):
    case, kind, idx = arg
    if case not in _W:
        _W[case] = _step_base(case)
    P, mlp, x, nxt, G = _W[case][:5]
    N = int(P.N)
    gb = sc.cotangents(N, 100 + N).reshape(3, -1)
    if kind == "x":
        fn = lambda xx: gb @ nc.oracle_step_nn(P, mlp, xx, G)[0].ravel()
        return case, kind, idx, sc.fd_columns(fn, x, idx, sc.H), sc.fd_columns(fn, x, idx, 2 * sc.H)
    dirs = nc.weight_directions(mlp)[idx]
    fn = lambda m: gb @ nc.oracle_step_nn(P, m, x, G)[0].ravel()
    return case, kind, idx, nc.weight_fd(fn, mlp, dirs, sc.H), nc.weight_fd(fn, mlp, dirs, 2 * sc.H)


def _roll_setup(case):
    ps, N, T, net = case
    P, mlp = sc.params(ps, N), nc.network(net)
    ctl = sc.orc.batch_sine_controls(1, T, P.del_t, 11)[0]
    s0 = sc.straight_state(P)
    ent = sc.rollout_state0_entries(N)
    x = np.concatenate([ctl.ravel(), sc.bnd_of(P), [s0[j, s] for j, s in ent]])
    gb = sc.rollout_cotangents(T, N, 200 + N + T).reshape(2, -1)

    def fn(xx, m=mlp):
        st = s0.copy()
        for (j, s), v in zip(ent, xx[4 * T + 19:]):
            st[j, s] = v
        return gb @ nc.oracle_rollout_nn(P, m, xx[:4 * T].reshape(T, 4), st, bnd=xx[4 * T:4 * T + 19]).ravel()
    return x, fn, ctl, mlp


def _roll_task(arg):
    case, kind, idx = arg
    if case not in _W:
        _W[case] = _roll_setup(case)
    x, fn, _, mlp = _W[case]
    if kind == "x":
        return case, kind, idx, sc.fd_columns(fn, x, idx, sc.H), sc.fd_columns(fn, x, idx, 2 * sc.H)
    dirs = nc.weight_directions(mlp)[idx]
    f = lambda m: fn(x, m)
    return case, kind, idx, nc.weight_fd(f, mlp, dirs, sc.H), nc.weight_fd(f, mlp, dirs, 2 * sc.H)


def _chunks(n):
    return [list(range(i, min(i + CHUNK, n))) for i in range(0, n, CHUNK)]


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else os.cpu_count()
    out = {"H": np.array(sc.H)}
    for net in nc.FIXTURE_NETS:
        mlp = nc.network(net)
        for k, (W, b) in enumerate(zip(mlp.weights, mlp.biases)):
            out[f"net_{net}_W{k}"], out[f"net_{net}_b{k}"] = W, b
        out[f"net_{net}_acts"] = np.array(mlp.acts, dtype=np.int32)
    step_cases = [(ps, N, rod, state, net) for ps, N, rods, state, net in nc.NN_STEP_CASES for rod in range(rods)]
    roll_cases = list(nc.NN_ROLLOUT_CASES)
    ndirs = lambda net: 6 * (len(nc.NETWORKS[net][0]) + 1)
    tasks = [(c, "x", idx) for c in step_cases for idx in _chunks(24 * c[1] + 23)] + \
            [(c, "w", idx) for c in step_cases for idx in _chunks(ndirs(c[4]))]
    rtasks = [(c, "x", idx) for c in roll_cases for idx in _chunks(4 * c[2] + 19 + 36)] + \
             [(c, "w", idx) for c in roll_cases for idx in _chunks(ndirs(c[3]))]
    tasks.sort(key=lambda t: -t[0][1])  # (long rods first)
    res = {}
    with mp.Pool(procs) as pool:
        for fn, tk in ((_step_task, tasks), (_roll_task, rtasks)):
            for case, kind, idx, a, b in pool.imap_unordered(fn, tk):
                res.setdefault((case, kind), []).append((idx, a, b))
    for case in step_cases:
        ps, N, rod, state, net = case
        P, mlp, x, nxt, G, prev, cur, tens = _step_base(case)
        k = nc.nn_case_key(ps, N, state, net) + f"_r{rod}_"
        out[k + "prev"], out[k + "cur"], out[k + "next"], out[k + "tens"] = prev, cur, nxt, tens
        out[k + "gbar"] = sc.cotangents(N, 100 + N)
        fd_h, fd_2h = np.zeros((3, 24 * N + 23)), np.zeros((3, 24 * N + 23))
        for idx, a, b in res[(case, "x")]:
            fd_h[:, idx], fd_2h[:, idx] = a.T, b.T
        out[k + "fd_h"], out[k + "fd_2h"] = fd_h, fd_2h
        nd = ndirs(net)
        wh, w2h = np.zeros((nd, 3)), np.zeros((nd, 3))
        for idx, a, b in res[(case, "w")]:
            wh[idx], w2h[idx] = a, b
        out[k + "wfd_h"], out[k + "wfd_2h"] = wh, w2h
    for case in roll_cases:
        ps, N, T, net = case
        x, fn, ctl, mlp = _roll_setup(case)
        k = f"roll_{ps}_N{N}_T{T}_{net}_"
        out[k + "ctl"] = ctl
        out[k + "gbar"] = sc.rollout_cotangents(T, N, 200 + N + T)
        fd_h, fd_2h = np.zeros((2, x.size)), np.zeros((2, x.size))
        for idx, a, b in res[(case, "x")]:
            fd_h[:, idx], fd_2h[:, idx] = a.T, b.T
        out[k + "fd_h"], out[k + "fd_2h"] = fd_h, fd_2h
        nd = ndirs(net)
        wh, w2h = np.zeros((nd, 2)), np.zeros((nd, 2))
        for idx, a, b in res[(case, "w")]:
            wh[idx], w2h[idx] = a, b
        out[k + "wfd_h"], out[k + "wfd_2h"] = wh, w2h
    path = os.path.join(HERE, "step_adjoint_nn.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
