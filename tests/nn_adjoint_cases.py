"""Networks, closed forms, cases and the NumPy restatement of the tests of the adjoint with the MLP on
(kr_mlp_input_jacobian_batch, kr_step_vjp_nn_batch, kr_simulate_vjp_nn_batch).

The networks have fp32 weights of both signs, ``gain N(0, 1) / sqrt(fan_in)``: with the all-positive 0.01-sized weights of
``cosserat_oracle.make_mlp`` the activation derivatives sit within a percent of act'(0) and a wrong diagonal factor would
hide inside a tolerance.  The Jacobian dNN/dx is the chain rule in matrix form, evaluated here in NumPy fp64 together with
the entrywise bound its rounding obeys."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "knode-cosserat_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import cosserat_oracle as orc  # noqa: E402

# name -> (hidden widths, activation, gain): the four networks of the adjoint's fixture, then relu at a ragged width past
# one 64-unit chunk of the one-hidden-layer kernel and at ragged two-layer widths.  tanh17 has gain 0.3, not the 0.5 of
# the others: at 0.5 (and 0.4) the oracle's Newton iteration does not reach 1e-15 on two rods of the 30-step run at
# (bc, N = 10) - the gain was lowered, not the solve tolerance.
NETWORKS = {
    "tanh17": ((17,), "tanh", 0.3),
    "softplus33x20": ((33, 20), "softplus", 0.5),
    "elu64x64": ((64, 64), "elu", 0.5),
    "elu512": ((512,), "elu", 0.3),
    "relu100": ((100,), "relu", 0.5),
    "relu20x33": ((20, 33), "relu", 0.5),
}
ACT_CODES = {"none": orc.ACT_NONE, "tanh": orc.ACT_TANH, "softplus": orc.ACT_SOFTPLUS, "relu": orc.ACT_RELU, "elu": orc.ACT_ELU}


def signed_mlp(hidden, act, gain, seed):
    """28 -> hidden... -> 25, fp32, signed weights gain N(0, 1) / sqrt(fan_in), biases 0.1 N(0, 1); no activation on the last layer"""
    rng = np.random.default_rng(seed)
    sizes = [28, *hidden, 25]
    Ws = [(gain * rng.normal(size=(sizes[k + 1], sizes[k])) / np.sqrt(sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)]
    bs = [(0.1 * rng.normal(size=(sizes[k + 1],))).astype(np.float32) for k in range(len(sizes) - 1)]
    return orc.Mlp(Ws, bs, [ACT_CODES[act]] * len(hidden) + [orc.ACT_NONE], False)


def network(name, seed=11):
    hidden, act, gain = NETWORKS[name]
    return signed_mlp(hidden, act, gain, seed)


def act_derivative(code, a):
    """d act / d a in fp64, in forms that keep the RELATIVE accuracy (sech^2 = 4 e / (1 + e)^2 with e = exp(-2 |a|), not
    1 - tanh^2)"""
    a = np.asarray(a, np.float64)
    if code == orc.ACT_NONE:
        return np.ones_like(a)
    if code == orc.ACT_TANH:
        e = np.exp(-2.0 * np.abs(a))
        return 4.0 * e / (1.0 + e) ** 2
    if code == orc.ACT_SOFTPLUS:
        e = np.exp(-np.abs(a))
        return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if code == orc.ACT_RELU:
        return (a > 0).astype(np.float64)
    if code == orc.ACT_ELU:
        return np.where(a > 0, 1.0, np.exp(np.minimum(a, 0.0)))
    raise ValueError(code)


def input_jacobian(mlp, x):
    """-> (Jn[25, 28] = dNN/dx at x, B[25, 28] = |W_L| diag|act'| ... |W_1|, the matrix the rounding bound is stated in)"""
    a = np.asarray(x, np.float64)
    J = B = None
    for W, b, code in zip(mlp.weights, mlp.biases, mlp.acts):
        W = W.astype(np.float64)
        pre = W @ a + b.astype(np.float64)
        d = act_derivative(code, pre)
        J = d[:, None] * (W if J is None else W @ J)
        B = np.abs(d)[:, None] * (np.abs(W) if B is None else np.abs(W) @ B)
        a = orc._activate(code, pre)
    return J, B


def jacobian_gamma(mlp):
    """The factor of the entrywise bound |device - NumPy| <= gamma B: one rounding per term of each inner product (the
    hidden widths and the 28 inputs of the pre-activations), and 64 ulps for the distance between the device's and NumPy's
    exp / log1p / expm1 in the activation derivatives."""
    return (sum(W.shape[0] for W in mlp.weights[:-1]) + 28 + 64) * 2.0 ** -53


def integer_mlp(hidden, seed):
    """Small-integer weights, no activation anywhere, NO symmetry in any layer: every product of the chain is exact in
    fp64, so the Jacobian is W_L ... W_1 to the last bit whatever the summation order - and a transposed operand, a
    swapped row / column map or a wrong k order changes integers."""
    rng = np.random.default_rng(seed)
    sizes = [28, *hidden, 25]
    Ws = [rng.integers(-3, 4, size=(sizes[k + 1], sizes[k])).astype(np.float32) for k in range(len(sizes) - 1)]
    for W in Ws:
        W[0, -1] += 5.0  # (square blocks included: no layer equals its transpose)
    bs = [rng.integers(-2, 3, size=(sizes[k + 1],)).astype(np.float32) for k in range(len(sizes) - 1)]
    return orc.Mlp(Ws, bs, [orc.ACT_NONE] * len(Ws), False)


# ---- the step adjoint with the network on: cases, the oracle's step, the NumPy restatement -----------------------------------
import step_adjoint_cases as sc  # noqa: E402

FIXTURE_NETS = ("tanh17", "softplus33x20", "elu64x64", "elu512")
# (parameter set, N, rods, state, network)
NN_STEP_CASES = [("bc", 10, 3, "sine30", net) for net in FIXTURE_NETS] + \
                [(ps, N, rods, "sine30", net) for ps, N, rods in (("plain", 2, 3), ("plain", 3, 3), ("bc", 33, 1))
                 for net in ("elu64x64", "tanh17")] + [("plain", 10, 3, "straight", "elu64x64")]
NN_ROLLOUT_CASES = [("bc", 10, T, "elu64x64") for T in (1, 3, 8)]


def nn_case_key(ps, N, state, net):
    return f"{ps}_N{N}_{state}_{net}"


def oracle_step_nn(P, mlp, x, G0, tol=sc.ORACLE_TOL):
    """step_adjoint_cases.oracle_step with the network in the sweep (cosserat_oracle.residual_euler(..., mlp))"""
    N = int(P.N)
    cur, prev, tens, bnd = sc.split_x(np.asarray(x, float), N)
    D = sc.with_bnd(P, bnd).derived()
    hist = D.c1 * cur + D.c2 * prev
    yh = np.zeros((19, N))
    yh[13:19] = hist[:, 0:6].T
    zh = hist[:, 6:12].T.copy()
    y = np.zeros((19, N))
    z = np.zeros((6, N))
    z[:, N - 1] = cur[N - 1, 6:12]
    G, ok, it = orc.newton_shoot(lambda g: orc.residual_euler(D, g, y, z, yh, zh, tens, mlp), G0, tol=tol)
    if not ok:
        raise RuntimeError("oracle step did not converge")
    return sc.pack(y, z), G


def oracle_rollout_nn(P, mlp, ctl, state0, bnd=None, tol=sc.ORACLE_TOL):
    bnd = sc.bnd_of(P) if bnd is None else bnd
    states = [np.array(state0, float)]
    prev = states[0]
    G = np.zeros(6)
    for tens in np.asarray(ctl, float):
        nxt, G = oracle_step_nn(P, mlp, sc.x_of(states[-1], prev, tens, bnd), G, tol)
        prev = states[-1]
        states.append(nxt)
    return np.array(states)


def step_inputs_nn(ps, N, rod, state, mlp):
    """prev, cur [N, 28], tensions [4] of one rod of a step case: steps 29 / 30 of a sine run OF THE MODEL WITH ITS NETWORK"""
    P = sc.params(ps, N)
    ctl = orc.batch_sine_controls(3, 31, P.del_t, 7)[rod]
    s0 = sc.straight_state(P)
    if state == "straight":
        return s0, s0, ctl[0]
    states = oracle_rollout_nn(P, mlp, ctl[:30], s0)
    return states[29], states[30], ctl[30]


def with_weights(mlp, theta):
    """the network with the flat parameter vector theta (W1, b1, W2, b2, ... in nn.Linear order), fp64"""
    Ws, bs, o = [], [], 0
    for W, b in zip(mlp.weights, mlp.biases):
        Ws.append(theta[o:o + W.size].reshape(W.shape))
        o += W.size
        bs.append(theta[o:o + b.size])
        o += b.size
    return orc.Mlp(Ws, bs, list(mlp.acts), False)


def flat_weights(mlp):
    return np.concatenate([np.concatenate([W.astype(np.float64).ravel(), b.astype(np.float64)]) for W, b in zip(mlp.weights, mlp.biases)])


def weight_directions(mlp):
    """Per layer: two dense unit directions in that layer's (W, b) block (entries sin(i phi + c): no random generator whose
    stream a fixture would depend on), then the four corner entries of its W.  -> [6 layers, n_params]"""
    dirs, o = [], 0
    total = sum(W.size + b.size for W, b in zip(mlp.weights, mlp.biases))
    for k, (W, b) in enumerate(zip(mlp.weights, mlp.biases)):
        n = W.size + b.size
        for c in range(2):
            d = np.zeros(total)
            d[o:o + n] = np.sin(np.arange(n) * (0.7 + 0.37 * c) + 0.3 * k + c)
            dirs.append(d / np.linalg.norm(d))
        rows, cols = W.shape
        for r, cc in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
            d = np.zeros(total)
            d[o + r * cols + cc] = 1.0
            dirs.append(d)
        o += n
    return np.array(dirs)


def mlp_backward_rows(mlp, X, Cc):
    """The ordinary MLP backward pass in fp64 over the rows (x, c): X [Q, 28], Cc [Q, 25] = dL/d(output) -> flat dL/dtheta
    in the order of flat_weights"""
    acts, hs, pres = list(mlp.acts), [np.asarray(X, np.float64)], []
    for W, b, code in zip(mlp.weights, mlp.biases, acts):
        pres.append(hs[-1] @ W.astype(np.float64).T + b.astype(np.float64))
        hs.append(orc._activate(code, pres[-1]))
    delta = np.asarray(Cc, np.float64)
    grads = [None] * len(acts)
    for k in range(len(acts) - 1, -1, -1):
        delta = delta * act_derivative(acts[k], pres[k])
        grads[k] = np.concatenate([(delta.T @ hs[k]).ravel(), delta.sum(axis=0)])
        delta = delta @ mlp.weights[k].astype(np.float64)
    return np.concatenate(grads)


def jacobian_with_network(mlp, jac_phys=sc.jacobian_exact):
    """The point Jacobian of the model with its network, J = Jp + Jn X, in point_jacobian's layout [25, 34]: X is identity
    on the y columns (rows 0..18), rows 19..24 of Jp (the z_phys tangents) and identity on the tf columns (rows 25..27)."""
    def jac(D, y, yh, zh, tf):
        Jp = jac_phys(D, y, yh, zh, tf)
        z_phys = orc.ode(D, y, yh, zh, tf)[1]
        Jn, _ = input_jacobian(mlp, np.concatenate([y, z_phys, tf]))
        X = np.zeros((28, 34))
        X[:19, :19] = np.eye(19)
        X[19:25] = Jp[19:25]
        X[25:28, 31:34] = np.eye(3)
        return Jp + Jn @ X
    return jac


def numpy_step_adjoint_nn(P, mlp, x, nxt, gbar, jac_phys=sc.jacobian_exact):
    """step_adjoint_cases.numpy_step_adjoint with the network's Jacobian in the point map, and the rows of the weight
    gradient: -> (gradient with respect to x, resid, X [N - 1, 28], C [N - 1, 25]), c_j = [ds lambda_{j+1}; g_z[j]]."""
    N = int(P.N)
    cur, prev, tens, bnd = sc.split_x(np.asarray(x, float), N)
    D = sc.with_bnd(P, bnd).derived()
    hist = D.c1 * cur + D.c2 * prev
    tf = orc.tendon_force(D, tens)
    y, _ = sc.unpack(nxt)
    gy = gbar[:, sc.ROW_TO_SLOT[:19]]
    gz = gbar[:, sc.ROW_TO_SLOT[19:]]
    jac = jacobian_with_network(mlp, jac_phys)
    Js, X = [], []
    for j in range(N - 1):
        yh = np.zeros(19)
        yh[13:19] = hist[j, 0:6]
        Js.append(jac(D, y[:, j], yh, hist[j, 6:12], tf))
        X.append(np.concatenate([y[:, j], orc.ode(D, y[:, j], yh, hist[j, 6:12], tf)[1], tf]))

    def sweep(seed_tip, with_g):
        lam = seed_tip.copy()
        ghist, gtf, rows = np.zeros((N, 12)), np.zeros(3), np.zeros((N - 1, 25))
        for j in range(N - 2, -1, -1):
            v = np.concatenate([D.ds * lam, gz[j] if with_g else np.zeros(6)])
            rows[j] = v
            jt = Js[j].T @ v
            lam = (gy[j] if with_g else 0.0) + lam + jt[:19]
            ghist[j] = jt[19:31]
            gtf += jt[31:34]
        return lam, ghist, gtf, rows
    lam0 = sweep(gy[N - 1], True)[0]
    a = lam0[7:13]
    M = np.array([sweep(np.eye(19)[7 + k], False)[0][7:13] for k in range(6)])
    nu = np.linalg.solve(M.T, -a)
    seed = gy[N - 1].copy()
    seed[7:13] += nu
    lam, ghist, gtf, rows = sweep(seed, True)
    g_cur = D.c1 * ghist
    g_cur[N - 1, 6:12] += gbar[N - 1, 6:12]
    g_bnd = np.concatenate([lam[0:7], lam[13:19], -nu])
    gx = np.concatenate([g_cur.ravel(), (D.c2 * ghist).ravel(), np.asarray(P.tendon_dirs, float) @ gtf, g_bnd])
    an = np.max(np.abs(a))
    return gx, (np.max(np.abs(lam[7:13])) / an if an > 0 else 0.0), np.array(X), rows


def weight_fd(fn_of_mlp, mlp, dirs, h):
    """central differences of fn along each direction of the flat weights -> [n_dirs, *fn(...).shape]"""
    th = flat_weights(mlp)
    return np.array([(fn_of_mlp(with_weights(mlp, th + h * d)) - fn_of_mlp(with_weights(mlp, th - h * d))) / (2 * h) for d in dirs])
