"""Cases and finite-difference machinery of the parameter-adjoint tests (kr_step_vjp_par_batch, kr_simulate_vjp_par_batch).

Expected values are central finite differences of the ORACLE's own step and rollout (step_adjoint_cases.oracle_step /
oracle_rollout, solved to ORACLE_TOL = 1e-15) of the scalar <gbar, next> in each of the 43 material parameters

    theta = [E, r, rho, L, vstar[3], g[3], Bse[9], Bbt[9], C[3], tendon_dirs[12]]      (KR_PAR order, row-major)

with the step's inputs (cur, prev, tensions, boundary) held fixed.  The sensitivities span twenty orders of magnitude
(E ~1e-10, r ~1e3, Bse ~1e-7), so every comparison is per parameter BLOCK, and the step of a difference is relative to a
scale per block (SCALES).  One relative step does not serve every block - the drag q|q| has a kink that C needs a large step
to average over (and where q is small its whole effect is tiny), Bse is a 1e-5 perturbation of Kse and drowns in rounding
below H = 1e-2 - so the fixture's generator
(tests/golden/make_golden_param_adjoint.py) takes H per block from a ladder: for every rung the difference is formed at H and
2 H, the block's tolerance is the project's rule (step_adjoint_cases.block_tol: ten times their disagreement plus what the
quotient cannot resolve), and the rung with the smallest tolerance relative to the block's largest entry is kept and
recorded.  Every block of every case must come out with a tolerance of at most MAX_REL_TOL of its largest entry.

A rollout's differences rebuild the straight initial state from the perturbed parameters (its p scales with L), as a user's
87 forward rollouts would: the device adds no initial-state term, and none is needed - no step reads p of an earlier state.

numpy_param_adjoint restates the recursion of the header in NumPy, with the parameter tangents of the point map taken by
differences of cosserat_oracle.ode through RodParams.derived()."""
import copy

import numpy as np

import step_adjoint_cases as sc

orc = sc.orc

KR_PAR = 43
# name, offset, count, shape
PAR_BLOCKS = (("E", 0, 1, ()), ("r", 1, 1, ()), ("rho", 2, 1, ()), ("L", 3, 1, ()), ("vstar", 4, 3, (3,)), ("g", 7, 3, (3,)),
              ("Bse", 10, 9, (3, 3)), ("Bbt", 19, 9, (3, 3)), ("C", 28, 3, (3,)), ("tendon_dirs", 31, 12, (4, 3)))
BLOCK_NAMES = tuple(b[0] for b in PAR_BLOCKS)
LADDER = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
# The ladder's extension upward.  Bse: c0 Bse stays a 3e-4 part of Kse even at H = 10.  C: the step depends on C through
# the drag C q|q| alone, linearly at fixed inputs (a second-order response comes through the solve only), and where q is
# small - one interval from a base at rest, the tip cotangent alone - its whole effect is 1e-9 of the loss: only a large
# step lifts it above the rounding of the quotient.  Either way the H / 2 H rule measures what truncation is left.
LADDER_UP = {"Bse": (1e1, 1e0, 1e-1), "C": (1e3, 1e2, 1e1, 1e0, 1e-1)}
MAX_REL_TOL = 1e-2
# relative steps of numpy_param_adjoint's differences of the point map (default 1e-4).  C: the map is exactly linear in it, and
# its tangent R (q|q|) is ~1e-9 beside values of order one - only a step of 100 in C itself lifts it over their rounding
INNER_H = {"Bse": 1e-1, "Bbt": 1e-1, "C": 1e6}


def ladder_of(name):
    return LADDER_UP.get(name, ()) + LADDER


def theta_of(P):
    return np.concatenate([[P.E, P.r, P.rho, P.L], np.asarray(P.vstar, float), np.asarray(P.g, float), np.asarray(P.Bse, float).ravel(),
                           np.asarray(P.Bbt, float).ravel(), np.asarray(P.C, float), np.asarray(P.tendon_dirs, float).ravel()])


def with_theta(P, th):
    P = copy.deepcopy(P)
    th = np.asarray(th, float)
    P.E, P.r, P.rho, P.L = (float(v) for v in th[:4])
    for name, off, n, shape in PAR_BLOCKS[4:]:
        setattr(P, name, th[off:off + n].reshape(shape).copy())
    return P


def scales_of(P):
    """The scale a difference's relative step multiplies, per parameter: |value| for E, r, rho, L; 1 for vstar; 9.81 for g;
    3e-2 for Bse / Bbt; 1e-4 for C; 1 for tendon_dirs."""
    s = np.ones(KR_PAR)
    s[0:4] = np.abs(theta_of(P)[0:4])
    s[7:10] = 9.81
    s[10:28] = 3e-2
    s[28:31] = 1e-4
    return s


def fd_theta(fn, P, idx, H):
    """Central differences of fn(parameter set) in the parameters idx, step H * scale -> [len(idx), *fn(P).shape]"""
    th, s = theta_of(P), scales_of(P)
    out = []
    for i in idx:
        tp, tm = th.copy(), th.copy()
        tp[i] += H * s[i]
        tm[i] -= H * s[i]
        out.append((fn(with_theta(P, tp)) - fn(with_theta(P, tm))) / (2 * H * s[i]))
    return np.array(out)


def choose_rungs(est, floors1):
    """est[name][rung] = (a, b): the block's estimates at H and 2 H, [C cotangents, count]; floors1[c] = fd_floor at a unit
    step.  -> per cotangent and block the kept rung: fd_h, fd_2h [C, KR_PAR], rung [C, blocks], floor [C, blocks]."""
    C = len(floors1)
    fd_h, fd_2h = np.zeros((C, KR_PAR)), np.zeros((C, KR_PAR))
    rung, floor = np.zeros((C, len(PAR_BLOCKS))), np.zeros((C, len(PAR_BLOCKS)))
    for bi, (name, off, n, _) in enumerate(PAR_BLOCKS):
        for c in range(C):
            best = None
            for H, (a, b, scale) in est[name].items():
                fl = floors1[c] / (H * scale)
                size = float(np.max(np.abs(a[c])))
                tol = sc.block_tol(a[c], b[c], fl)
                rel = tol / size if size > 0 else (0.0 if tol == 0 else np.inf)
                if best is None or rel < best[0]:
                    best = (rel, H, a[c], b[c], fl)
            fd_h[c, off:off + n], fd_2h[c, off:off + n] = best[2], best[3]
            rung[c, bi], floor[c, bi] = best[1], best[4]
    return fd_h, fd_2h, rung, floor


def fd_ladder(fn, P, floors1):
    """fn(parameter set) -> [C] (one scalar per cotangent).  The whole ladder for all 43 parameters, then choose_rungs."""
    s = scales_of(P)
    est = {}
    for name, off, n, _ in PAR_BLOCKS:
        est[name] = {}
        for H in ladder_of(name):
            a = fd_theta(fn, P, range(off, off + n), H).T
            b = fd_theta(fn, P, range(off, off + n), 2 * H).T
            est[name][H] = (a, b, float(s[off]))
    return choose_rungs(est, floors1)


def unit_floor(gbar, out):
    """step_adjoint_cases.fd_floor at a step of one: divide by the absolute step of the block"""
    return sc.fd_floor(gbar, out, h=1.0)


# What the oracle's SOLVE leaves in a quotient.  newton_shoot stops before applying an update d with |d|_inf <= ORACLE_TOL
# max(1, |G|_inf): each evaluation's base wrench is off its root by up to that, which moves the loss by up to |dL/dG|_1 times
# it (dL/dG: the sweep's derivative at fixed inputs, `a` of the recursion) - in either direction, whatever the step, so H and
# 2 H can agree on it.  A difference of two evaluations over 2 h carries twice that over 2 h.  Against the rounding floor it
# matters where the absolute step is tiny (r: 3e-8 .. 3e-11), and nowhere else.
def sweep_at(P, x, G):
    """the oracle's sweep of one step at a GIVEN base wrench (no solve) -> next [N, 28]"""
    N = int(P.N)
    cur, prev, tens, bnd = sc.split_x(np.asarray(x, float), N)
    D = sc.with_bnd(P, bnd).derived()
    hist = D.c1 * cur + D.c2 * prev
    yh = np.zeros((19, N))
    yh[13:19] = hist[:, 0:6].T
    zh = hist[:, 6:12].T.copy()
    y, z = np.zeros((19, N)), np.zeros((6, N))
    z[:, N - 1] = cur[N - 1, 6:12]
    orc.residual_euler(D, G, y, z, yh, zh, tens)
    return sc.pack(y, z)


def _g_steps(G):
    return 1e-6 * np.maximum(np.abs(G), 1.0)


def solve_floor_step(P, x, G, gb):
    """unit-step floor of the solve for a step case, per cotangent: |dL/dG|_1 ORACLE_TOL max(1, |G|_inf)"""
    e = _g_steps(G)
    a = np.array([(gb @ sweep_at(P, x, G + e[c] * np.eye(6)[c]).ravel() - gb @ sweep_at(P, x, G - e[c] * np.eye(6)[c]).ravel()) / (2 * e[c])
                  for c in range(6)])  # [6, C]
    return np.sum(np.abs(a), axis=0) * sc.ORACLE_TOL * max(1.0, float(np.max(np.abs(G))))


def solve_floor_rollout(P, ctl, gb):
    """the same for a rollout: the sum over its steps, dL/dG_t taken through the later steps' own solves"""
    s0 = sc.straight_state(P)
    bnd = sc.bnd_of(P)
    states, Gs, prev, G = [s0], [], s0, np.zeros(6)
    for tens in ctl:
        nxt, G = sc.oracle_step(P, sc.x_of(states[-1], prev, tens, bnd), G)
        prev = states[-1]
        states.append(nxt)
        Gs.append(G)

    def loss_from(t, Gt):
        st = list(states[:t + 1])
        st.append(sweep_at(P, sc.x_of(st[t], st[t - 1] if t > 0 else st[0], ctl[t], bnd), Gt))
        for u in range(t + 1, len(ctl)):
            st.append(sc.oracle_step(P, sc.x_of(st[u], st[u - 1], ctl[u], bnd), Gs[u])[0])
        return gb @ np.array(st).ravel()
    total = np.zeros(gb.shape[0])
    for t, G in enumerate(Gs):
        e = _g_steps(G)
        a = np.array([(loss_from(t, G + e[c] * np.eye(6)[c]) - loss_from(t, G - e[c] * np.eye(6)[c])) / (2 * e[c]) for c in range(6)])
        total += np.sum(np.abs(a), axis=0) * sc.ORACLE_TOL * max(1.0, float(np.max(np.abs(G))))
    return total


def block_report(got, fd_h, fd_2h, floor):
    """Per block: (name, max-abs error of `got` against the kept estimate, tolerance, the block's largest entry, exact zero?)"""
    rows = []
    for bi, (name, off, n, _) in enumerate(PAR_BLOCKS):
        a, b = fd_h[off:off + n], fd_2h[off:off + n]
        zero = not np.any(a) and not np.any(b)
        rows.append((name, float(np.max(np.abs(got[off:off + n] - a))), sc.block_tol(a, b, float(floor[bi])), float(np.max(np.abs(a))), zero))
    return rows


def assert_blocks(got, fd_h, fd_2h, floor, label, worst=None):
    """Every block of `got` [KR_PAR] within its tolerance, which is at most MAX_REL_TOL of the block's largest entry; a block
    (or a tendon_dirs row) whose expected value is exactly zero must be exactly zero.  Prints each figure first."""
    for name, err, tol, size, zero in block_report(got, fd_h, fd_2h, floor):
        print(f"{label} {name:12s} err {err:.2e} tol {tol:.2e} size {size:.2e}" + (" (exactly zero)" if zero else ""))
        if worst is not None and not zero:
            worst[name] = max(worst.get(name, 0.0), err / tol)
        if zero:
            assert err == 0.0, (label, name, err)
        else:
            assert tol <= MAX_REL_TOL * size, (label, name, tol, size)
            assert err <= tol, (label, name, err, tol)
    for i in range(4):
        sl = slice(31 + 3 * i, 34 + 3 * i)
        if not np.any(fd_h[sl]) and not np.any(fd_2h[sl]):
            assert not np.any(got[sl]), (label, "tendon_dirs row", i, got[sl])


# ---- the NumPy restatement of the recursion ------------------------------------------------------------------------------
def point_param_tangents(P, y, yh, zh, tens, h_scale=1.0):
    """[25, KR_PAR]: d [ds y_s; z] / d theta at one grid point, the inputs held fixed, by central differences of
    cosserat_oracle.ode through RodParams.derived() (relative step INNER_H[block] * h_scale, default 1e-4 * h_scale);
    with it the value [ds y_s; z] itself and the absolute steps [KR_PAR]."""
    th, s = theta_of(P), scales_of(P)

    def F(t):
        D = with_theta(P, t).derived()
        ys, z = orc.ode(D, y, yh, zh, orc.tendon_force(D, tens))
        return np.concatenate([D.ds * ys, z])
    cols, habs = np.zeros((25, KR_PAR)), np.zeros(KR_PAR)
    for name, off, n, _ in PAR_BLOCKS:
        h = INNER_H.get(name, 1e-4) * h_scale
        for i in range(off, off + n):
            tp, tm = th.copy(), th.copy()
            tp[i] += h * s[i]
            tm[i] -= h * s[i]
            cols[:, i] = (F(tp) - F(tm)) / (2 * h * s[i])
            habs[i] = h * s[i]
    return cols, F(th), habs


def numpy_param_adjoint(P, x, nxt, gbar, h_scales=(1.0,), jac=sc.jacobian_exact):
    """The recursion of kr_step_vjp_par_batch in NumPy -> (g_par [KR_PAR] per inner step scale, gradient with respect to x in
    the layout of step_adjoint_cases.numpy_step_adjoint).  lambda is the total adjoint: the sweep seeded with g plus nu on
    the tip's (n, m); g_par = sum_j [lambda_{j+1}; g_z[j]] . d [ds y_s; z]_j / d theta.  The point Jacobians in (y, history,
    tf) are the 50-digit oracle's by default, so that what is left is the resolution of the parameter differences alone."""
    N = int(P.N)
    cur, prev, tens, bnd = sc.split_x(np.asarray(x, float), N)
    Pb = sc.with_bnd(P, bnd)
    D = Pb.derived()
    hist = D.c1 * cur + D.c2 * prev
    tf = orc.tendon_force(D, tens)
    y, _ = sc.unpack(nxt)
    gy = gbar[:, sc.ROW_TO_SLOT[:19]]
    gz = gbar[:, sc.ROW_TO_SLOT[19:]]
    Js, yhs = [], []
    for j in range(N - 1):
        yh = np.zeros(19)
        yh[13:19] = hist[j, 0:6]
        yhs.append(yh)
        Js.append(jac(D, y[:, j], yh, hist[j, 6:12], tf))

    def sweep(seed_tip, with_g):
        lam, lams = seed_tip.copy(), {}
        ghist, gtf = np.zeros((N, 12)), np.zeros(3)
        for j in range(N - 2, -1, -1):
            lams[j] = lam.copy()  # lambda_{j+1}
            jt = Js[j].T @ np.concatenate([D.ds * lam, gz[j] if with_g else np.zeros(6)])
            lam = (gy[j] if with_g else 0.0) + lam + jt[:19]
            ghist[j] = jt[19:31]
            gtf += jt[31:34]
        return lam, lams, ghist, gtf
    a = sweep(gy[N - 1], True)[0][7:13]
    M = np.array([sweep(np.eye(19)[7 + k], False)[0][7:13] for k in range(6)])
    nu = np.linalg.solve(M.T, -a)
    seed = gy[N - 1].copy()
    seed[7:13] += nu
    lam, lams, ghist, gtf = sweep(seed, True)
    g_pars = []
    for hs in h_scales:
        # .round: what these quotients cannot resolve - each is a difference of two values of c . F rounded at 2^-53 of
        # their terms, over twice the step (step_adjoint_cases.fd_floor, point by point)
        g_par, rnd = np.zeros(KR_PAR), np.zeros(KR_PAR)
        for j in range(N - 1):
            c = np.concatenate([lams[j], gz[j]])
            cols, F0, habs = point_param_tangents(Pb, y[:, j], yhs[j], hist[j, 6:12], tens, hs)
            g_par += c @ cols
            rnd += np.array([sc.fd_floor(c, F0, h) for h in habs])
        g_pars.append(g_par)
        numpy_param_adjoint.round = rnd if hs == h_scales[0] else numpy_param_adjoint.round
    g_cur = D.c1 * ghist
    g_cur[N - 1, 6:12] += gbar[N - 1, 6:12]
    gx = np.concatenate([g_cur.ravel(), (D.c2 * ghist).ravel(), np.asarray(P.tendon_dirs, float) @ gtf,
                         np.concatenate([lam[0:7], lam[13:19], -nu])])
    return g_pars, gx


def numpy_rollout_param_adjoint(P, ctl, states, gbar, h_scales=(1.0,)):
    """The composition that defines kr_simulate_vjp_par_batch, in NumPy: step adjoints for t = T - 1 .. 0, g_states[t] +=
    g_cur, g_states[t - 1] += g_prev, g_par summed over the steps (per inner step scale).  No term for the initial state."""
    T, N = len(ctl), int(P.N)
    g = np.array(gbar, float)
    bnd = sc.bnd_of(P)
    g_pars = [np.zeros(KR_PAR) for _ in h_scales]
    numpy_rollout_param_adjoint.round = np.zeros(KR_PAR)
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else states[0]
        gp, gx = numpy_param_adjoint(P, sc.x_of(states[t], prev, ctl[t], bnd), states[t + 1], g[t + 1], h_scales)
        gx = sc.split_grad(gx, N)
        g[t, :, :12] += gx["cur"]
        g[max(t - 1, 0), :, :12] += gx["prev"]
        for acc, v in zip(g_pars, gp):
            acc += v
        numpy_rollout_param_adjoint.round += numpy_param_adjoint.round
    return g_pars


# ---- the fixture's cases -------------------------------------------------------------------------------------------------
# the step cases of step_adjoint_cases without N = 130 (prev, cur, next, tensions are read from step_adjoint.npz), the first
# two cotangents of cotangents(); one more with a slack tendon (tension 2 = 0: its tendon_dirs row is exactly zero)
STEP_CASES = [c for c in sc.STEP_CASES if c[1] != 130]
N_COT = 2
ZERO_T_CASE = ("plain", 10, 0, "sine30")  # key zeroT_...: tensions[2] = 0, next re-solved by the oracle and stored
ROLLOUT_CASES = list(sc.ROLLOUT_CASES)
CPU_ROLLOUT_CASE = ("plain", 6, 3)  # held against numpy_rollout_param_adjoint in the CPU test


def step_key(ps, N, rod, state):
    return sc.case_key(ps, N, state) + f"_r{rod}_"


def roll_key(ps, N, T):
    return f"roll_{ps}_N{N}_T{T}_"


def roll_inputs(ps, N, T):
    """ctl [T, 4], gbar [2, T + 1, N, 28] of a rollout case (those of step_adjoint_cases' fixture)"""
    P = sc.params(ps, N)
    return P, orc.batch_sine_controls(1, T, P.del_t, 11)[0], sc.rollout_cotangents(T, N, 200 + N + T)


def rollout_of(P, ctl):
    """the oracle's rollout from the straight rod OF THESE PARAMETERS"""
    return sc.oracle_rollout(P, ctl, sc.straight_state(P))
