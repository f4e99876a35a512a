"""Cases and finite-difference machinery of the step-adjoint tests (kr_step_vjp_batch, kr_simulate_vjp_batch).

Expected values are central finite differences of the ORACLE's own step: ``cosserat_oracle.residual_euler`` solved by
``cosserat_oracle.newton_shoot`` to ORACLE_TOL = 1e-15, with everything a step reads packed into one input vector

    x = [cur[N, 12], prev[N, 12], tensions[4], bnd[19]]        (leading slots q w v u; bnd in KR_BND order)

and its output ``next[N, 25]`` in packed slot order.  Every difference is taken at two step sizes, H and 2 H; a compared
block's tolerance is ten times the disagreement of the two estimates (truncation falls by four between them), never a
number chosen in advance.  The solve is tighter than 1e-13 on purpose: newton_shoot stops BEFORE applying its last update, and
with a forward-difference Jacobian that update is proportional to the distance from the start - a perturbed solve warm-started
at the base solution keeps an error proportional to the perturbation, which a difference quotient turns into a bias that
does not depend on the step size (measured at 1e-13: 2e-9 relative at N = 2, five times the H / 2 H disagreement; at 1e-15
it is below 1e-10).  tests/golden/make_golden_step_adjoint.py writes the fixture ``step_adjoint.npz`` from here;
the CPU test re-derives a small case at test time."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "knode-cosserat_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import cosserat_oracle as orc  # noqa: E402

H = 1e-5
ORACLE_TOL = 1e-15
SLOTS = 28
# reference row (0..24 of [y; z]) -> packed slot (knode_rod.h)
ROW_TO_SLOT = np.array([12 + r for r in range(13)] + [r - 13 for r in range(13, 19)] + [6 + (r - 19) for r in range(19, 25)])
BND_KEYS = (("p0", 3), ("h0", 4), ("q0", 3), ("w0", 3), ("F_tip", 3), ("M_tip", 3))
PARAM_SETS = ("plain", "fullB", "bc", "noair")
# the compared blocks: name -> (array, slice of its last axis)
BLOCKS = [(f"g_{a}.{n}", a, slice(s, s + 3)) for a in ("cur", "prev") for n, s in (("q", 0), ("w", 3), ("v", 6), ("u", 9))] + \
         [("g_tensions", "tens", slice(0, 4))] + \
         [(f"g_bnd.{n}", "bnd", slice(s, e)) for n, s, e in (("p0", 0, 3), ("h0", 3, 7), ("q0", 7, 10), ("w0", 10, 13), ("F_tip", 13, 16), ("M_tip", 16, 19))]


def params(name, N):
    """The four parameter sets of the tests: the plain preset, one with non-diagonal Bse / Bbt, the boundary surface of
    bc.npz (tilted non-unit h0, tip wrench, q0 / w0 != 0, tendon directions with a z part) and `noair`."""
    P = orc.setup_params("noair" if name == "noair" else None, N)
    if name == "fullB":
        P.Bse = np.array([[2e-2, 4e-3, -2e-3], [4e-3, 3e-2, 5e-3], [-2e-3, 5e-3, 1e-2]])
        P.Bbt = np.array([[3e-2, 6e-3, -3e-3], [6e-3, 2e-2, 4e-3], [-3e-3, 4e-3, 4e-2]])
    elif name == "bc":
        g = np.load(os.path.join(ROOT, "tests", "golden", "bc.npz"))
        for k in ("F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
            setattr(P, k, np.array(g[f"par_{k}"], dtype=np.float64))
    elif name not in ("plain", "noair"):
        raise ValueError(name)
    return P


def bnd_of(P):
    return np.concatenate([np.asarray(getattr(P, k), float).ravel() for k, _ in BND_KEYS])


def with_bnd(P, bnd):
    P = copy.deepcopy(P)
    o = 0
    for k, n in BND_KEYS:
        setattr(P, k, np.array(bnd[o:o + n], float))
        o += n
    return P


def pack(y, z):
    """[19, N], [6, N] -> record array [N, 28]"""
    rec = np.zeros((y.shape[1], SLOTS))
    rec[:, ROW_TO_SLOT] = np.vstack([y, z]).T
    return rec


def unpack(rec):
    rows = rec[:, ROW_TO_SLOT].T
    return rows[:19].copy(), rows[19:].copy()


def x_of(cur, prev, tens, bnd):
    return np.concatenate([cur[:, :12].ravel(), prev[:, :12].ravel(), np.asarray(tens, float), np.asarray(bnd, float)])


def split_x(x, N):
    n = 12 * N
    return x[:n].reshape(N, 12), x[n:2 * n].reshape(N, 12), x[2 * n:2 * n + 4], x[2 * n + 4:]


def oracle_step(P, x, G0, tol=ORACLE_TOL):
    """One implicit step of the oracle from the packed inputs x -> (next[N, 25 used of 28], G).  History
    c1 cur + c2 prev on the twelve leading slots (the only ones the equations read, cosserat_ode.py:146-148); column N-1
    of z is never written by the sweep (cosserat_ode.py:196-198) and so stays the current state's."""
    N = int(P.N)
    cur, prev, tens, bnd = split_x(np.asarray(x, float), N)
    D = with_bnd(P, bnd).derived()
    hist = D.c1 * cur + D.c2 * prev
    yh = np.zeros((19, N))
    yh[13:19] = hist[:, 0:6].T
    zh = hist[:, 6:12].T.copy()
    y = np.zeros((19, N))
    z = np.zeros((6, N))
    z[:, N - 1] = cur[N - 1, 6:12]
    G, ok, it = orc.newton_shoot(lambda g: orc.residual_euler(D, g, y, z, yh, zh, tens), G0, tol=tol)
    if not ok:
        raise RuntimeError("oracle step did not converge")
    return pack(y, z), G


def oracle_rollout(P, ctl, state0, bnd=None, tol=ORACLE_TOL, G0=None):
    """T oracle steps from state0 [N, 28] with y_prev = y before the first (knode.py:65-66) -> states [T + 1, N, 28]"""
    bnd = bnd_of(P) if bnd is None else bnd
    states = [np.array(state0, float)]
    prev = states[0]
    G = np.zeros(6) if G0 is None else G0
    for tens in np.asarray(ctl, float):
        nxt, G = oracle_step(P, x_of(states[-1], prev, tens, bnd), G, tol)
        prev = states[-1]
        states.append(nxt)
    return np.array(states)


def straight_state(P):
    y, z = orc.straight_state(P.derived())
    return pack(y, z)


def fd_columns(fn, x, idx, h):
    """Central differences (fn(x + h e_i) - fn(x - h e_i)) / 2h for i in idx -> [len(idx), *fn(x).shape]"""
    out = []
    for i in idx:
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        out.append((fn(xp) - fn(xm)) / (2 * h))
    return np.array(out)


def cotangents(N, seed):
    """The three cotangents of the step tests, [3, N, 28]: random on all 25 slots of all points; tip position only;
    v, u of the last point only (the pass-through)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((3, N, SLOTS))
    g[0, :, :25] = rng.normal(size=(N, 25))
    g[1, N - 1, 12:15] = rng.normal(size=3)
    g[2, N - 1, 6:12] = rng.normal(size=6)
    return g


def split_grad(gx, N):
    """gradient with respect to x -> dict cur [N, 12], prev [N, 12], tens [4], bnd [19]"""
    cur, prev, tens, bnd = split_x(gx, N)
    return dict(cur=cur, prev=prev, tens=tens, bnd=bnd)


def fd_floor(gbar, out, h=H):
    """What a difference quotient of L = <gbar, out> cannot resolve: L is a sum of products each rounded to 2^-53
    relative, so L(x + h) - L(x - h) carries up to 2^-52 sum |gbar_i out_i|, divided by 2 h - whatever the two step
    sizes happen to agree on (a block that depends on x linearly, such as the pass-through of v, u of the last point,
    gives two estimates that agree to the last bit and are both one such rounding off)."""
    return 2.0 ** -52 * float(np.sum(np.abs(np.asarray(gbar) * np.asarray(out)))) / (2 * h)


def block_tol(a, b, floor):
    """Tolerance of a compared block from its two estimates (H and 2 H): ten times their disagreement (truncation falls
    by four between them), plus the resolution of the quotient itself (fd_floor)."""
    return 10.0 * float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) + floor


def block_report(got, fd_h, fd_2h, N, floor=0.0):
    """Per block: (name, max-abs error of `got` against the H estimate, tolerance, size of the block's largest entry)."""
    g, a, b = split_grad(got, N), split_grad(fd_h, N), split_grad(fd_2h, N)
    rows = []
    for name, arr, sl in BLOCKS:
        err = float(np.max(np.abs(g[arr][..., sl] - a[arr][..., sl])))
        rows.append((name, err, block_tol(a[arr][..., sl], b[arr][..., sl], floor), float(np.max(np.abs(a[arr][..., sl])))))
    return rows


def jacobian_exact(D, y, yh, zh, tf):
    """point_jacobian's layout from the 50-digit derivative oracle (oracle/ode_derivative.py)"""
    import ode_derivative as od
    J = od.jacobian_mp(D, y, yh, zh, tf)
    return np.concatenate([J[:, 0:19], J[:, 32:38], J[:, 38:44], J[:, 44:47]], axis=1)


# ---- a NumPy restatement of the adjoint recursion (second oracle; held to oracle/ode_derivative.py in the CPU test) ----
def point_jacobian(D, y, yh, zh, tf, h=1e-6):
    """[25, 19 + 12 + 3] Jacobian of (y_s, z) in (y, history q w v u, tf) by central differences of cosserat_oracle.ode"""
    x0 = np.concatenate([y, yh[13:19], zh, tf])

    def f(x):
        yh_ = np.zeros(19)
        yh_[13:19] = x[19:25]
        ys, z = orc.ode(D, x[:19], yh_, x[25:31], x[31:34])
        return np.concatenate([ys, z])
    return fd_columns(f, x0, range(34), h).T


def numpy_step_adjoint(P, x, nxt, gbar, jac=point_jacobian):
    """The recursion of kr_step_vjp_batch in NumPy: -> (gradient with respect to x, resid)."""
    N = int(P.N)
    cur, prev, tens, bnd = split_x(np.asarray(x, float), N)
    D = with_bnd(P, bnd).derived()
    hist = D.c1 * cur + D.c2 * prev
    tf = orc.tendon_force(D, tens)
    y, _ = unpack(nxt)
    gy = gbar[:, ROW_TO_SLOT[:19]]
    gz = gbar[:, ROW_TO_SLOT[19:]]
    Js = []
    for j in range(N - 1):
        yh = np.zeros(19)
        yh[13:19] = hist[j, 0:6]
        Js.append(jac(D, y[:, j], yh, hist[j, 6:12], tf))

    def sweep(seed_tip, with_g):
        lam = seed_tip.copy()
        ghist = np.zeros((N, 12))
        gtf = np.zeros(3)
        for j in range(N - 2, -1, -1):
            v = np.concatenate([D.ds * lam, gz[j] if with_g else np.zeros(6)])
            jt = Js[j].T @ v
            lam = (gy[j] if with_g else 0.0) + lam + jt[:19]
            ghist[j] = jt[19:31]
            gtf += jt[31:34]
        return lam, ghist, gtf
    lam0, _, _ = sweep(gy[N - 1], True)
    a = lam0[7:13]
    M = np.array([sweep(np.eye(19)[7 + k], False)[0][7:13] for k in range(6)])
    nu = np.linalg.solve(M.T, -a)
    seed = gy[N - 1].copy()
    seed[7:13] += nu
    lam, ghist, gtf = sweep(seed, True)
    g_cur = D.c1 * ghist
    g_cur[N - 1, 6:12] += gbar[N - 1, 6:12]
    g_bnd = np.concatenate([lam[0:7], lam[13:19], -nu])
    gx = np.concatenate([g_cur.ravel(), (D.c2 * ghist).ravel(), np.asarray(P.tendon_dirs, float) @ gtf, g_bnd])
    an = np.max(np.abs(a))
    return gx, (np.max(np.abs(lam[7:13])) / an if an > 0 else 0.0)


# ---- the fixture's cases -------------------------------------------------------------------------------------------------
# (parameter set, N, rods, state): "sine30" = prev / cur are steps 29 / 30 of a sine run, "straight" = the first step from
# the straight rod (q = 0, the kink of q|q|; prev is cur)
STEP_CASES = [(ps, 10, 3, "sine30") for ps in PARAM_SETS] + [("plain", 10, 3, "straight")] + \
             [("plain", 2, 3, "sine30"), ("bc", 2, 3, "sine30"), ("plain", 3, 3, "sine30"), ("bc", 3, 3, "sine30"),
              ("plain", 33, 3, "sine30"), ("bc", 33, 3, "sine30"), ("plain", 100, 1, "sine30"), ("plain", 130, 1, "sine30")]
ROLLOUT_CASES = [(ps, N, T) for N, ps in ((10, "bc"), (33, "plain")) for T in (1, 2, 3, 8)]


def case_key(ps, N, state):
    return f"{ps}_N{N}_{state}"


def step_inputs(ps, N, rod, state):
    """prev, cur [N, 28], tensions [4] of one rod of a step case (deterministic)."""
    P = params(ps, N)
    ctl = orc.batch_sine_controls(3, 31, P.del_t, 7)[rod]
    s0 = straight_state(P)
    if state == "straight":
        return s0, s0, ctl[0]
    states = oracle_rollout(P, ctl[:30], s0)
    return states[29], states[30], ctl[30]


def rollout_cotangents(T, N, seed):
    """[2, T + 1, N, 28]: a tip cotangent on every solved state; every slot of ONE interior state."""
    rng = np.random.default_rng(seed)
    g = np.zeros((2, T + 1, N, SLOTS))
    g[0, 1:, N - 1, 12:15] = rng.normal(size=(T, 3))
    g[1, max(1, T // 2), :, :25] = rng.normal(size=(N, 25))
    return g


def rollout_state0_entries(N):
    """the entries of the initial state whose gradient is compared: (point, slot)"""
    return [(j, s) for j in sorted({0, N // 2, N - 1}) for s in range(12)]
