"""Cases and finite-difference machinery of the table-adjoint tests (kr_step_vjp_table_batch, kr_simulate_vjp_table_batch):
a heterogeneous batch - every rod its own parameter set, controls and BOUNDARY HISTORY - differentiated rod by rod.

The fixture's rods are the three parameter sets a table row can hold (step_adjoint_cases.params: `plain`, `bc`, `noair`;
`fullB` is not diagonal) at N = 9, the lower edge of a table call.  Rod b runs under its own sine controls and its own smooth
boundary history bnd[t] (KR_BND order): p0 slides along a direction of its own, q0 carries the matching body-frame velocity
R(h0)^T dp0/dt, and F_tip varies - on top of the set's own boundary values.  The sets `plain` and `noair` differ in the drag C
alone, which a rod at rest hardly feels: the bases slide at up to 0.6 m/s so that a rod computed with another rod's row is told
apart (the CPU test's first mutant).

Expected values are central differences of the ORACLE's own rollout with bnd[t] per step (oracle_step with another bnd each
step), solved to ORACLE_TOL = 1e-15, of sum_t <gbar[t], states[t]> with respect to
    ctl[T][4], bnd[T][19], the rollout_state0_entries of states[0] (and of prev_init where a case has one)    at H and 2 H,
    the 43 material parameters                                                   on the ladder of param_adjoint_cases,
every block under the project's rule (ten times the H / 2 H disagreement plus the quotient's floor), which
tests/golden/make_golden_table_adjoint.py requires to stay within MAX_REL_TOL of the block.  Differences in the parameters
hold states[0] (and prev_init) FIXED: the table adjoint adds no initial-state term, and the fixture's initial states are
inputs like any other (the CPU test of param_adjoint_cases shows that a rebuilt straight state changes nothing)."""
import numpy as np

import param_adjoint_cases as pc
import step_adjoint_cases as sc

orc = sc.orc

SETS = ("plain", "bc", "noair")
N_FIX = 9
# case name -> (T, with a prev_init)
CASES = {"T1": (1, False), "T3": (3, False), "T3p": (3, True)}
MAX_REL_TOL = pc.MAX_REL_TOL
SLIDE = ((0.02, 6.0, (1.0, 0.3, 0.1)), (0.03, 9.0, (-0.4, 1.0, 0.2)), (0.05, 12.0, (0.6, -0.7, 0.4)))  # amplitude m, rad/s, direction
# The step of a difference in an entry of states[0] / prev_init.  Under the tip cotangent the gradient with respect to the
# angular-velocity history of a state three steps back is ~1e-8 of a loss of order one: at H = 1e-5 the quotient's rounding
# floor alone was 2 % of that block (measured, T3p), at 1e-4 it is a tenth of that and the truncation still far below it.
H_STATE = 1e-4
WRENCH = ((0.02, 5.0), (0.03, 8.0), (0.025, 11.0))  # amplitude N, rad/s of the F_tip variation


def key(b, case):
    return f"{SETS[b]}_{case}_"


def boundary_history(P, b, T, t0=0):
    """bnd[T][19] of rod b: step t is solved at time (t0 + t + 1) del_t"""
    base = sc.bnd_of(P)
    amp, om, d = SLIDE[b]
    d = np.asarray(d) / np.linalg.norm(d)
    fa, fo = WRENCH[b]
    R = orc.quat_rotation(np.asarray(P.h0, float))
    out = np.tile(base, (T, 1))
    for t in range(T):
        tau = (t0 + t + 1) * P.del_t
        out[t, 0:3] += amp * np.sin(om * tau) * d
        out[t, 7:10] += R.T @ (amp * om * np.cos(om * tau) * d)
        out[t, 13:16] += fa * np.array([np.sin(fo * tau), np.cos(fo * tau), 0.5 * np.sin(2 * fo * tau)])
    return out


def rollout(P, ctl, bnd, state0, prev_init=None, G0=None, tol=sc.ORACLE_TOL):
    """T oracle steps, step t with the boundary values bnd[t] -> (states [T + 1, N, 28], the base wrenches [T, 6]).
    prev_init None: y_prev = y before the first step (knode.py:65-66).  G0 None: every solve starts from the wrench before
    it (the first from zero); G0 [T, 6]: step t starts from G0[t] (a perturbed rollout from the base rollout's wrenches)."""
    states, Gs = [np.array(state0, float)], []
    prev = states[0] if prev_init is None else np.array(prev_init, float)
    G = np.zeros(6)
    for t, tens in enumerate(np.asarray(ctl, float)):
        nxt, G = sc.oracle_step(P, sc.x_of(states[-1], prev, tens, bnd[t]), G if G0 is None else np.asarray(G0[t], float), tol)
        prev = states[-1]
        states.append(nxt)
        Gs.append(G)
    return np.array(states), np.array(Gs)


_cache = {}


def rod_case(b, case):
    """Everything of rod b in `case`: dict P, T, ctl [T, 4], bnd [T, 19], state0, prev_init (or None), gbar [2, T + 1, N, 28],
    states [T + 1, N, 28], Gs [T, 6] (deterministic)."""
    if (b, case) in _cache:
        return _cache[(b, case)]
    T, with_prev = CASES[case]
    P = sc.params(SETS[b], N_FIX)
    ctl_all = orc.batch_sine_controls(3, T + 2, P.del_t, 21)[b]
    s0 = sc.straight_state(P)
    if with_prev:  # two steps of the same rod first: states[0] and prev_init are its states 2 and 1
        warm, _ = rollout(P, ctl_all[:2], boundary_history(P, b, 2), s0)
        prev_init, state0, ctl, bnd = warm[1], warm[2], ctl_all[2:], boundary_history(P, b, T, t0=2)
    else:
        prev_init, state0, ctl, bnd = None, s0, ctl_all[:T], boundary_history(P, b, T)
    states, Gs = rollout(P, ctl, bnd, state0, prev_init)
    gbar = sc.rollout_cotangents(T, N_FIX, 300 + 10 * b + T + int(with_prev))
    _cache[(b, case)] = dict(P=P, T=T, ctl=ctl, bnd=bnd, state0=state0, prev_init=prev_init, gbar=gbar, states=states, Gs=Gs)
    return _cache[(b, case)]


# ---- the inputs a difference moves, as one vector: [ctl (4 T), bnd (19 T), entries of states[0], entries of prev_init] ----
def entries():
    return sc.rollout_state0_entries(N_FIX)


def x_of(rc):
    ent = entries()
    parts = [rc["ctl"].ravel(), rc["bnd"].ravel(), [rc["state0"][j, s] for j, s in ent]]
    if rc["prev_init"] is not None:
        parts.append([rc["prev_init"][j, s] for j, s in ent])
    return np.concatenate(parts)


def loss_of_x(rc, x, P=None):
    """[2]: sum_t <gbar_c[t], states[t]> of the oracle's rollout at the inputs x (parameters P, default the rod's)"""
    T, ent = rc["T"], entries()
    s0 = rc["state0"].copy()
    o = 23 * T
    for (j, s), v in zip(ent, x[o:o + len(ent)]):
        s0[j, s] = v
    pi = None
    if rc["prev_init"] is not None:
        pi = rc["prev_init"].copy()
        for (j, s), v in zip(ent, x[o + len(ent):]):
            pi[j, s] = v
    st, _ = rollout(P if P is not None else rc["P"], x[:4 * T].reshape(T, 4), x[4 * T:23 * T].reshape(T, 19), s0, pi, G0=rc["Gs"])
    return rc["gbar"].reshape(2, -1) @ st.ravel()


def x_blocks(T, with_prev):
    """The compared blocks of the input gradient: (name, indices into x)"""
    ent = entries()
    bl = [(f"g_ctl[{t}]", list(range(4 * t, 4 * t + 4))) for t in range(T)]
    for t in range(T):
        bl += [(f"g_bnd[{t}].{n}", list(range(4 * T + 19 * t + s, 4 * T + 19 * t + e)))
               for n, s, e in (("p0", 0, 3), ("h0", 3, 7), ("q0", 7, 10), ("w0", 10, 13), ("F_tip", 13, 16), ("M_tip", 16, 19))]
    o = 23 * T
    bl += [(f"g_states[0].{n}", [o + i for i, (j, s) in enumerate(ent) if s // 3 == q]) for q, n in enumerate("qwvu")]
    if with_prev:
        bl += [(f"g_prev_init.{n}", [o + len(ent) + i for i, (j, s) in enumerate(ent) if s // 3 == q]) for q, n in enumerate("qwvu")]
    return bl


def solve_floor(rc, gb):
    """param_adjoint_cases.solve_floor_rollout with bnd[t] per step and the case's own start: what the oracle's solves leave
    in a quotient at a UNIT step, per cotangent"""
    P, ctl, bnd, states, Gs = rc["P"], rc["ctl"], rc["bnd"], rc["states"], rc["Gs"]
    first_prev = rc["state0"] if rc["prev_init"] is None else rc["prev_init"]

    def loss_from(t, Gt):
        st = list(states[:t + 1])
        st.append(pc.sweep_at(P, sc.x_of(st[t], st[t - 1] if t > 0 else first_prev, ctl[t], bnd[t]), Gt))
        for u in range(t + 1, len(ctl)):
            st.append(sc.oracle_step(P, sc.x_of(st[u], st[u - 1], ctl[u], bnd[u]), Gs[u])[0])
        return gb @ np.array(st).ravel()
    total = np.zeros(gb.shape[0])
    for t, G in enumerate(Gs):
        e = 1e-6 * np.maximum(np.abs(G), 1.0)
        a = np.array([(loss_from(t, G + e[c] * np.eye(6)[c]) - loss_from(t, G - e[c] * np.eye(6)[c])) / (2 * e[c]) for c in range(6)])
        total += np.sum(np.abs(a), axis=0) * sc.ORACLE_TOL * max(1.0, float(np.max(np.abs(G))))
    return total


def x_step(i, T):
    """the step of the difference in entry i of x: H for ctl and bnd, H_STATE for the entries of states[0] / prev_init"""
    return sc.H if i < 23 * T else H_STATE


def x_floor(rc, c, solve1):
    """[2]: the floor of an input block of cotangent c - the quotient's rounding plus what the solves leave - at step H (ctl,
    bnd) and at H_STATE (state entries)"""
    return np.array([sc.fd_floor(rc["gbar"][c], rc["states"], h) + float(solve1[c]) / h for h in (sc.H, H_STATE)])


def _floor_of(name, floor):
    return float(floor[0 if name.startswith(("g_ctl", "g_bnd")) else 1])


def assert_x_blocks(got, fd_h, fd_2h, floor, T, with_prev, label, worst=None, only=("g_",)):
    """Every input block of `got` (a vector laid out like x) within its tolerance, which is at most MAX_REL_TOL of the block;
    a block whose two estimates are exactly zero (steps behind the only state a cotangent touches) must be exactly zero.
    only: the prefixes of the blocks to compare (default all)."""
    for name, idx in x_blocks(T, with_prev):
        if not name.startswith(tuple(only)): continue
        a, b = fd_h[idx], fd_2h[idx]
        err, size = float(np.max(np.abs(got[idx] - a))), float(np.max(np.abs(a)))
        if not np.any(a) and not np.any(b):
            print(f"{label} {name:18s} err {err:.2e} (exactly zero)")
            assert err == 0.0, (label, name, err)
            continue
        tol = sc.block_tol(a, b, _floor_of(name, floor))
        print(f"{label} {name:18s} err {err:.2e} tol {tol:.2e} size {size:.2e} ratio {err / tol:.3f}")
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), err / tol)
        assert tol <= MAX_REL_TOL * size, (label, name, tol, size)
        assert err <= tol, (label, name, err, tol)


def x_misses(got, fd_h, fd_2h, floor, T, with_prev):
    """[(name, err / tol)] of the input blocks with a nonzero expected value (the mutants' measure)"""
    out = []
    for name, idx in x_blocks(T, with_prev):
        a, b = fd_h[idx], fd_2h[idx]
        if np.any(a) or np.any(b):
            out.append((name, float(np.max(np.abs(got[idx] - a))) / sc.block_tol(a, b, _floor_of(name, floor))))
    return out


# ---- the NumPy restatement: the composition of step adjoints with per-rod P and per-step boundary --------------------------
def jac_richardson(D, y, yh, zh, tf, h=1e-4):
    """step_adjoint_cases.point_jacobian at h and 2 h, extrapolated: truncation O(h^4), rounding ~1e-12 - two orders under
    the tightest block tolerance, at a hundredth of the 50-digit oracle's cost"""
    return (4.0 * sc.point_jacobian(D, y, yh, zh, tf, h) - sc.point_jacobian(D, y, yh, zh, tf, 2 * h)) / 3.0


def numpy_rollout_adjoint(P, rc, c, h_scales=(1.0, 2.0)):
    """The composition that defines kr_simulate_vjp_table_batch for ONE rod, in NumPy, with the row P (the rod's own, or - a
    mutant - another rod's): step adjoints for t = T - 1 .. 0 with the boundary values bnd[t], g_states[t] += g_cur,
    g_states[t - 1] += g_prev (step 0's into g_prev_init where the case has one), g_par summed over the steps.
    -> dict gx (laid out like x_of, the per-step boundary gradients in place), g_bnd [T, 19], g_par per inner step scale, round"""
    T, N, ent = rc["T"], N_FIX, entries()
    states, ctl, bnd = rc["states"], rc["ctl"], rc["bnd"]
    g = np.array(rc["gbar"][c], float)
    g_ctl, g_bnd = np.zeros((T, 4)), np.zeros((T, 19))
    g_pars, rnd = [np.zeros(pc.KR_PAR) for _ in h_scales], np.zeros(pc.KR_PAR)
    g_prev_init = None
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else (states[0] if rc["prev_init"] is None else rc["prev_init"])
        gp, gx = pc.numpy_param_adjoint(P, sc.x_of(states[t], prev, ctl[t], bnd[t]), states[t + 1], g[t + 1], h_scales, jac=jac_richardson)
        gx = sc.split_grad(gx, N)
        g[t, :, :12] += gx["cur"]
        if t > 0 or rc["prev_init"] is None:
            g[max(t - 1, 0), :, :12] += gx["prev"]
        else:
            g_prev_init = gx["prev"]
        g_ctl[t], g_bnd[t] = gx["tens"], gx["bnd"]
        for acc, v in zip(g_pars, gp):
            acc += v
        rnd += pc.numpy_param_adjoint.round
    parts = [g_ctl.ravel(), g_bnd.ravel(), [g[0, j, s] for j, s in ent]]
    if g_prev_init is not None:
        parts.append([g_prev_init[j, s] for j, s in ent])
    return dict(gx=np.concatenate(parts), g_bnd=g_bnd, g_par=g_pars, round=rnd)


def with_bnd_grad(gx, g_bnd, T):
    """gx with its per-step boundary part replaced by g_bnd [T, 19] (the second mutant's tool)"""
    out = gx.copy()
    out[4 * T:23 * T] = np.asarray(g_bnd).ravel()
    return out


# ---- heterogeneous batches for the device tests --------------------------------------------------------------------------
_robots = {}


def robot_for(ps, N):
    """A CosseratRod with the parameter set `ps` of step_adjoint_cases (MLP off); one per (set, N), shared by the tests"""
    from gpu_helpers import make_robot
    if (ps, N) not in _robots:
        P = sc.params(ps, N)
        r = make_robot("noair" if ps == "noair" else None, N)
        for k in ("Bse", "Bbt", "F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
            setattr(r, k, np.array(getattr(P, k), dtype=np.float64))
        r.compute_intermediate_terms()
        _robots[(ps, N)] = r
    return _robots[(ps, N)]


def carrier_for(N):
    """The robot whose handle carries a table call: its OWN parameters (the `youngs` preset, E = 10 GPa) belong to no row, so
    a kernel that read the handle's constants instead of the row's would miss every block"""
    from gpu_helpers import make_robot
    if ("carrier", N) not in _robots:
        _robots[("carrier", N)] = make_robot("youngs", N)
    return _robots[("carrier", N)]


def x_got(g_ctl, g_bnd, g_state0, g_prev_init=None):
    """device outputs of one rod (g_ctl [T, 4], g_bnd [T, 19], g_states[0] [N, 28], g_prev_init [N, 28] or None) laid out like x_of"""
    ent = entries()
    parts = [np.asarray(g_ctl).ravel(), np.asarray(g_bnd).ravel(), [g_state0[j, s] for j, s in ent]]
    if g_prev_init is not None:
        parts.append([g_prev_init[j, s] for j, s in ent])
    return np.concatenate(parts)
