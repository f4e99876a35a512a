"""Cases and finite-difference machinery of the bank-adjoint tests (kr_step_vjp_bank_batch, kr_simulate_vjp_bank_batch): a
heterogeneous batch WITH the residual MLP on - every rod its own parameter row, controls, boundary history AND network.

The fixture (tests/golden/bank_adjoint.npz, written by tests/golden/make_golden_bank_adjoint.py from the oracle alone) holds,
once per kernel family of the network's input Jacobian (`tanh17`: one hidden layer, one chunk; `softplus33x20`: two hidden
layers), ONE rollout of B = 5 rods over T = 4 steps at N = 9 and two of its single steps (step 0 from the straight rod, where
prev is cur, and the last step; the entries of cur and prev differenced at H_STATE, see step_h):
    rows      the three parameter sets a table row can hold (table_adjoint_cases.SETS), rod b on row ROW_OF_ROD[b]
    boundary  rod b's own sliding base and varying tip wrench per step (the histories of table_adjoint_cases, two more rods)
    networks  K = 3 of the family's shape, differing by seed (nn_adjoint_cases.signed_mlp), rod b on NET_OF_ROD[b] =
              [1, 0, 1, 1, 0]: the stable permutation by network is not the identity, network 2 has no rod, and network 1
              has 3 x 8 = 24 rows - past one 16-row workgroup tile of the one-hidden-layer kernel and ragged in the second.
Rods of one network sit on DIFFERENT rows, and rods of one row on different networks, so that neither index can stand in
for the other.

Expected values are central differences of the oracle's own rollout / step (cosserat_oracle.residual_euler(..., mlp) +
newton_shoot to ORACLE_TOL = 1e-15, bnd[t] per step) of L = sum_b sum_t <gbar_b[t], states_b[t]> at H and 2 H in
    rod b's ctl[T][4], bnd[T][19] and the rollout_state0_entries of its states[0] (these at H_STATE),
    for each network with rods, its flat weights along nn_adjoint_cases.weight_directions (six per layer: a block per layer),
where the loss of network k's weights runs over ITS rods.  A block's tolerance is the rule of the existing adjoint fixtures -
ten times the H / 2 H disagreement plus step_adjoint_cases.fd_floor - it is RECORDED in the file, and the generator refuses
to write a fixture in which a block's tolerance exceeds MAX_REL_TOL = 1e-2 of the block (table_adjoint.npz's cap)."""
import numpy as np

import nn_adjoint_cases as nc
import step_adjoint_cases as sc
import table_adjoint_cases as tc

orc = sc.orc

FAMILIES = ("tanh17", "softplus33x20")
B_FIX, T_FIX, K_FIX, N_FIX = 5, 4, 3, tc.N_FIX
NET_OF_ROD = (1, 0, 1, 1, 0)
ROW_OF_ROD = (0, 1, 2, 1, 0)  # index into SETS: network 1 runs rows 0, 2, 1; network 0 rows 1, 0
SETS = tc.SETS
NET_SEEDS = (11, 12, 13)
STEP_TS = (0, T_FIX - 1)
MAX_REL_TOL = tc.MAX_REL_TOL
H_STATE = tc.H_STATE
SLIDE = tc.SLIDE + ((0.04, 7.0, (0.2, 0.5, -0.8)), (0.025, 10.0, (-0.7, -0.2, 0.6)))  # amplitude m, rad/s, direction
WRENCH = tc.WRENCH + ((0.015, 6.5), (0.035, 9.5))  # amplitude N, rad/s of the F_tip variation
# gain per family: nn_adjoint_cases.NETWORKS' own (the oracle reached 1e-15 on every solve of the fixture with them)
GAIN = {f: nc.NETWORKS[f][2] for f in FAMILIES}


def networks(family):
    hidden, act, _ = nc.NETWORKS[family]
    return [nc.signed_mlp(hidden, act, GAIN[family], seed) for seed in NET_SEEDS]


def rods_of(k):
    return [b for b in range(B_FIX) if NET_OF_ROD[b] == k]


def key(family, b):
    return f"{family}_r{b}_"


def boundary_history(P, b, T):
    """table_adjoint_cases.boundary_history with this file's five histories"""
    base = sc.bnd_of(P)
    amp, om, d = SLIDE[b]
    d = np.asarray(d) / np.linalg.norm(d)
    fa, fo = WRENCH[b]
    R = orc.quat_rotation(np.asarray(P.h0, float))
    out = np.tile(base, (T, 1))
    for t in range(T):
        tau = (t + 1) * P.del_t
        out[t, 0:3] += amp * np.sin(om * tau) * d
        out[t, 7:10] += R.T @ (amp * om * np.cos(om * tau) * d)
        out[t, 13:16] += fa * np.array([np.sin(fo * tau), np.cos(fo * tau), 0.5 * np.sin(2 * fo * tau)])
    return out


def rollout(P, mlp, ctl, bnd, state0, G0=None, tol=sc.ORACLE_TOL):
    """T oracle steps with the network in the sweep, step t with bnd[t] -> (states [T + 1, N, 28], base wrenches [T, 6]);
    y_prev = y before the first step; G0 [T, 6]: step t starts from G0[t]"""
    states, Gs = [np.array(state0, float)], []
    prev, G = states[0], np.zeros(6)
    for t, tens in enumerate(np.asarray(ctl, float)):
        nxt, G = nc.oracle_step_nn(P, mlp, sc.x_of(states[-1], prev, tens, bnd[t]), G if G0 is None else np.asarray(G0[t], float), tol)
        prev = states[-1]
        states.append(nxt)
        Gs.append(G)
    return np.array(states), np.array(Gs)


_cache = {}


def rod_case(family, b):
    """Everything of rod b: dict P, mlp, T, ctl [T, 4], bnd [T, 19], state0, prev_init (None), gbar [2, T + 1, N, 28], states,
    Gs [T, 6], gstep [3, N, 28] (the cotangents of its single steps)"""
    if (family, b) not in _cache:
        P = sc.params(SETS[ROW_OF_ROD[b]], N_FIX)
        mlp = networks(family)[NET_OF_ROD[b]]
        ctl = orc.batch_sine_controls(B_FIX, T_FIX, P.del_t, 21)[b]
        bnd = boundary_history(P, b, T_FIX)
        s0 = sc.straight_state(P)
        states, Gs = rollout(P, mlp, ctl, bnd, s0)
        _cache[(family, b)] = dict(P=P, mlp=mlp, T=T_FIX, ctl=ctl, bnd=bnd, state0=s0, prev_init=None, states=states, Gs=Gs,
                                   gbar=sc.rollout_cotangents(T_FIX, N_FIX, 400 + 10 * b + T_FIX), gstep=sc.cotangents(N_FIX, 500 + b))
    return _cache[(family, b)]


# ---- the rollout: inputs as one vector x = [ctl (4 T), bnd (19 T), entries of states[0]] (table_adjoint_cases' layout) ----
entries, x_of, x_blocks, x_step, x_got = tc.entries, tc.x_of, tc.x_blocks, tc.x_step, tc.x_got


def loss_of_x(rc, x, mlp=None, P=None):
    """[2]: sum_t <gbar_c[t], states[t]> of the oracle's rollout of one rod at the inputs x (network mlp, row P: default its own)"""
    T, ent = rc["T"], entries()
    s0 = rc["state0"].copy()
    for (j, s), v in zip(ent, x[23 * T:]):
        s0[j, s] = v
    st, _ = rollout(P if P is not None else rc["P"], mlp if mlp is not None else rc["mlp"], x[:4 * T].reshape(T, 4),
                    x[4 * T:23 * T].reshape(T, 19), s0, G0=rc["Gs"])
    return rc["gbar"].reshape(2, -1) @ st.ravel()


def x_floor(rc, c):
    """[2]: the quotient's rounding floor of cotangent c at H (ctl, bnd) and at H_STATE (state entries)"""
    return np.array([sc.fd_floor(rc["gbar"][c], rc["states"], h) for h in (sc.H, H_STATE)])


def x_tols(fd_h, fd_2h, floor):
    """per block of x_blocks: its tolerance (0 for a block whose two estimates are exactly zero: it must be exactly zero)"""
    out = []
    for name, idx in x_blocks(T_FIX, False):
        a, b = fd_h[idx], fd_2h[idx]
        out.append(0.0 if not np.any(a) and not np.any(b) else sc.block_tol(a, b, tc._floor_of(name, floor)))
    return np.array(out)


def weight_loss(family, k, m):
    """[2]: the loss of network k's weights - the rollouts of ITS rods with the network m"""
    return sum(loss_of_x(rod_case(family, b), x_of(rod_case(family, b)), mlp=m) for b in rods_of(k))


def w_floor(family, k, c):
    return sum(sc.fd_floor(rod_case(family, b)["gbar"][c], rod_case(family, b)["states"]) for b in rods_of(k))


def w_tols(wfd_h, wfd_2h, floor):
    """per layer (six directions each): the block's tolerance"""
    return np.array([sc.block_tol(wfd_h[lo:lo + 6], wfd_2h[lo:lo + 6], floor) for lo in range(0, len(wfd_h), 6)])


def assert_blocks(label, names, got_blocks, fd_blocks, tols, worst=None):
    """err <= the RECORDED tolerance, block by block, every figure printed first; a zero tolerance means exactly zero"""
    for name, got, a, tol in zip(names, got_blocks, fd_blocks, tols):
        err, size = float(np.max(np.abs(np.asarray(got) - np.asarray(a)))), float(np.max(np.abs(a)))
        print(f"{label} {name:18s} err {err:.2e} tol {tol:.2e} size {size:.2e} ratio {err / tol if tol else 0.0:.3f}")
        if worst is not None and tol:
            worst[name] = max(worst.get(name, 0.0), err / tol)
        assert tol <= MAX_REL_TOL * size, (label, name, tol, size)
        assert err <= tol, (label, name, err, tol)


def x_check(label, got, fd_h, tols, worst=None):
    bl = x_blocks(T_FIX, False)
    assert_blocks(label, [n for n, _ in bl], [got[i] for _, i in bl], [fd_h[i] for _, i in bl], tols, worst)


def x_misses(got, fd_h, tols):
    """[(name, err / tol)] of the input blocks with a nonzero expected value (the mutants' measure)"""
    return [(name, float(np.max(np.abs(got[idx] - fd_h[idx]))) / tol) for (name, idx), tol in zip(x_blocks(T_FIX, False), tols) if tol]


def w_check(label, gw, wfd_h, tols, worst=None):
    n = len(tols)
    assert_blocks(label, [f"weights layer {l}" for l in range(n)], [gw[6 * l:6 * l + 6] for l in range(n)],
                  [wfd_h[6 * l:6 * l + 6] for l in range(n)], tols, worst)


def w_misses(gw, wfd_h, tols):
    return [(f"layer {l}", float(np.max(np.abs(gw[6 * l:6 * l + 6] - wfd_h[6 * l:6 * l + 6]))) / tols[l]) for l in range(len(tols))]


# ---- a single step of the rollout: x = [cur [N, 12], prev [N, 12], tensions [4], bnd [19]] (step_adjoint_cases' layout) ----
def step_inputs(rc, t):
    """(x, next, G) of step t of the rod's rollout (G: the oracle's base wrench, None for a case read from the fixture)"""
    st = rc["states"]
    return sc.x_of(st[t], st[t - 1] if t > 0 else st[0], rc["ctl"][t], rc["bnd"][t]), st[t + 1], (rc["Gs"][t] if "Gs" in rc else None)


def step_h(i):
    """the step of the difference in entry i of a step's x: H_STATE for the entries of cur and prev, H for tensions and bnd.
    (Under the tip cotangent the gradient with respect to the angular-velocity history is ~1e-8 of a loss of order one: at
    H = 1e-5 the quotient's rounding floor alone was 1.0 - 1.6 % of g_prev.w on seven step cases of softplus33x20 - measured;
    the rule table_adjoint_cases.H_STATE states for the entries of a rollout's initial state.)"""
    return H_STATE if i < 24 * N_FIX else sc.H


def step_floor(gbar, nxt):
    """[2]: the quotient's rounding floor at H_STATE (cur, prev) and at H (tensions, bnd)"""
    return np.array([sc.fd_floor(gbar, nxt, h) for h in (H_STATE, sc.H)])


def step_tols(fd_h, fd_2h, floor):
    """per block of step_adjoint_cases.BLOCKS: its tolerance (0 for a block whose two estimates are exactly zero)"""
    a, b = sc.split_grad(fd_h, N_FIX), sc.split_grad(fd_2h, N_FIX)
    return np.array([0.0 if not np.any(a[arr][..., sl]) and not np.any(b[arr][..., sl])
                     else sc.block_tol(a[arr][..., sl], b[arr][..., sl], float(floor[0 if arr in ("cur", "prev") else 1]))
                     for _, arr, sl in sc.BLOCKS])


def step_check(label, got, fd_h, tols, worst=None):
    g, a = sc.split_grad(got, N_FIX), sc.split_grad(fd_h, N_FIX)
    assert_blocks(label, [name for name, _, _ in sc.BLOCKS], [g[arr][..., sl] for _, arr, sl in sc.BLOCKS], [a[arr][..., sl] for _, arr, sl in sc.BLOCKS],
                  tols, worst)


# ---- the NumPy restatement: the composition of step adjoints with per-rod row and network ---------------------------------
def numpy_rollout_adjoint(P, mlp, rc, c):
    """The composition that defines kr_simulate_vjp_bank_batch for ONE rod in NumPy, with the row P and the network mlp (the
    rod's own, or - a mutant - another's) -> dict gx (laid out like x_of, per-step boundary gradients in place), X [T, N - 1, 28],
    C [T, N - 1, 25] (the rows of the weight gradient, step-major)"""
    T, ent = rc["T"], entries()
    states, ctl, bnd = rc["states"], rc["ctl"], rc["bnd"]
    g = np.array(rc["gbar"][c], float)
    g_ctl, g_bnd = np.zeros((T, 4)), np.zeros((T, 19))
    X, Cc = np.zeros((T, N_FIX - 1, 28)), np.zeros((T, N_FIX - 1, 25))
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else states[0]
        gx, _, X[t], Cc[t] = nc.numpy_step_adjoint_nn(P, mlp, sc.x_of(states[t], prev, ctl[t], bnd[t]), states[t + 1], g[t + 1],
                                                      jac_phys=tc.jac_richardson)
        gx = sc.split_grad(gx, N_FIX)
        g[t, :, :12] += gx["cur"]
        g[max(t - 1, 0), :, :12] += gx["prev"]
        g_ctl[t], g_bnd[t] = gx["tens"], gx["bnd"]
    return dict(gx=np.concatenate([g_ctl.ravel(), g_bnd.ravel(), [g[0, j, s] for j, s in ent]]), X=X, C=Cc)


def weight_grad(mlp, X, Cc):
    """the six directional derivatives per layer of network mlp from rows X [..., 28], C [..., 25] (fp64 NumPy backward)"""
    return nc.weight_directions(mlp) @ nc.mlp_backward_rows(mlp, np.asarray(X).reshape(-1, 28), np.asarray(Cc).reshape(-1, 25))


# ---- the device side ------------------------------------------------------------------------------------------------------
def fixture_networks(fx, family):
    """the K networks of a family from the fixture's own arrays (the weights it was computed with)"""
    n = len(nc.NETWORKS[family][0]) + 1
    return [orc.Mlp([fx[f"net_{family}_{k}_W{l}"] for l in range(n)], [fx[f"net_{family}_{k}_b{l}"] for l in range(n)],
                    [int(a) for a in fx[f"net_{family}_acts"]], False) for k in range(K_FIX)]


def fixture_case(fx, family, b, nets=None):
    """rod b of the fixture as numpy_rollout_adjoint wants it (its inputs and the oracle's states from the file)"""
    k = key(family, b)
    nets = nets if nets is not None else fixture_networks(fx, family)
    return dict(P=sc.params(SETS[ROW_OF_ROD[b]], N_FIX), mlp=nets[NET_OF_ROD[b]], T=T_FIX, ctl=fx[k + "ctl"], bnd=fx[k + "bnd"],
                state0=fx[k + "state0"], prev_init=None, states=fx[k + "states"], gbar=fx[k + "gbar"])
