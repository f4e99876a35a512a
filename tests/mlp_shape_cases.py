"""Networks, inputs and oracle references shared by tests/test_gpu_mlp_shapes.py and tests/test_mlp_shapes_cpu.py (not a
test module): the in-sweep MLP at widths that are no multiple of the 16-unit tile or the 64-unit chunk, and the number
of Newton sweeps a step needs with and without a working Jacobian of the network.

PARITY networks are ``orc.make_mlp`` networks (the project's weight class) at the smallest shapes of each padding /
chunking rule of ``build_mlp_plan`` (csrc/kr_api.hip) and of the evaluators of mlp_mfma.hpp / mlp_jvp.hpp.  They keep
the input columns of the positions p.  Every reference is computed once per process by the oracle's tightly converged
Newton solver, asserts ``ier == 1`` on every step and is handed out read-only.

COUNT networks have signed weights ``gain * N(0, 1) / sqrt(fan_in)`` (fp32; biases as in ``make_mlp``): a network whose
Jacobian matters to Newton's convergence.  Their first three INPUT COLUMNS of layer 0 ARE ZERO: the one-launch-per-step
multiple-shooting kernel carries no Jacobian columns for the interval-start positions (PCOL is persistent-only,
kr_ms_impl.hpp), which is a known omission of that kernel, not of the evaluator under test; a network that does not read
p cannot have its sweep count moved by it.

Two oracle counts per count case, rod and precision (``sweep_counts``):

* ``full``:   ``orc.newton_shoot`` iterations per step at the sweep precision's stopping rule (fp64: tol 1e-8, forward
              differences 1e-7; fp32: tol 1e-5, 1e-3), from the reference's warm start (the previous step's G);
* ``frozen``: the same Newton, except that the six perturbed sweeps of an iteration reuse, grid point by grid point, the
              network outputs recorded during that iteration's base sweep - what a dead or mispacked Jacobian chain of
              mlp_jvp.hpp amounts to (NN(x_b) + 0 * dx).  Base and line-search sweeps evaluate the network normally, so
              the root is the same.

``count_bound`` is what the GPU may need: S_full + T + (S_frozen - S_full) / 3 summed sweeps per rod (one storing sweep
per step at the accepted unknowns, which newton_shoot performs outside its count, and a third of the reference gap for
what the design knowingly gives up: bf16 operands, act' one-sided at the base point, the interval unknowns of multiple
shooting)."""
import functools

import numpy as np

DEL_T = 0.05          # every preset's time step (knode.py:8)
CTL_SEED = 77
B = 3                 # rods of every batch here
T_PARITY = 10
T_COUNT = 8
NET_SEED = 7
BANK_SEEDS = (7, 8, 9)
BANK_NETS = (2, 0, 1)
BANK_MODS = (None, "damping", "short")

#        id: (layer widths, activation)                 the smallest case of ...
PARITY = {
    "a": ((28, 1, 25), "elu"),             # one real unit in a 64-unit chunk
    "b": ((28, 17, 25), "tanh"),           # width = 16 + 1
    "c": ((28, 130, 25), "elu"),           # third chunk of a two-layer net holds 2 units
    "d": ((28, 17, 33, 25), "elu"),        # tile3 / tile3f with both widths ragged
    "e": ((28, 50, 64, 25), "relu"),       # tile3 / tile3f, first width ragged
    "f": ((28, 64, 65, 25), "elu"),        # one unit spills into a second chunk: mlp_jvp_tile with chunks2 = 2
    "g": ((28, 33, 192, 25), "tanh"),      # chunks2 = 3: last act' slot, largest served shape
    "h": ((28, 64, 191, 25), "elu"),       # the same, last chunk one unit short
    "i": ((28, 40, 25), "softplus"),       # padded units with act(0) = ln 2
}
PARITY_IDS = tuple(PARITY)
PARITY_SCALE = {"i": 1.0}   # (case i converges on the oracle with make_mlp's plain weights: no scaling needed)
W2_IDS = ("d", "f", "g")    # also at N = 40 with two wavefronts per rod
BANK_IDS = ("d", "g")
REFUSED = ((28, 64, 193, 25), (28, 65, 64, 25))

#        id: (layer widths, activation, gain)
COUNT = {
    "c3_64_64": ((28, 64, 64, 25), "elu", 0.5),      # one chunk per layer: mlp_jvp_tile3 (fp64) / tile3f (fp32)
    "c2_130": ((28, 130, 25), "elu", 0.45),          # two layers, three chunks, the last with 2 units
    "c3_17_33": ((28, 17, 33, 25), "elu", 0.6),      # tile3 / tile3f, both widths ragged (in neither count test: below)
    "c3_50_49": ((28, 50, 49, 25), "elu", 0.6),      # tile3 / tile3f, both widths ragged, wide enough to count
    "c3_64_192": ((28, 64, 192, 25), "elu", 0.6),    # mlp_jvp_tile, chunks2 = 3
}
COUNT_IDS = tuple(COUNT)
# The cases each precision's count test runs: those that meet the conditions of tests/test_mlp_shapes_cpu.py on all
# three rods.  Measured with these weights (sums over the 8 steps, exact / frozen, rods 0, 1, 2):
#   c2_130 at gain 0.5 backtracks and has steps of 7 and 13 exact iterations; at 0.45: fp64 38/98 38/97 39/100,
#     fp32 33/63 33/64 35/65 - kept at 0.45.
#   c3_17_33 misses the ratio at every gain tried in [0.4, 0.6]: at 0.6 fp64 33/80 33/79 39/92 (2.4 < 2.5), fp32 31/52 30/51
#     32/59 (1.7 < 1.75); at 0.55 fp64 2.25 / fp32 1.64; at 0.5 2.0 / 1.52; at 0.4 1.8 / 1.36.  So narrow a network does
#     not steer Newton enough.  It is DROPPED from both count tests (its shape stays a parity case, d); c3_50_49, the
#     next ragged shape of the same one-chunk evaluators that does meet every condition (fp64 44/117 44/120 42/130, fp32
#     41/74 39/76 36/82), stands in for it.
COUNT_F64 = ("c3_64_64", "c2_130", "c3_50_49", "c3_64_192")
COUNT_F32 = ("c3_64_64", "c2_130", "c3_50_49", "c3_64_192")
COUNT_OF = {"f64": COUNT_F64, "f32": COUNT_F32}
RULE = {"f64": dict(tol=1e-8, fd_eps=1e-7, ratio=2.5), "f32": dict(tol=1e-5, fd_eps=1e-3, ratio=1.75)}


def layer_widths(mlp):
    return [mlp.weights[0].shape[1]] + [w.shape[0] for w in mlp.weights]


@functools.lru_cache(maxsize=None)
def parity_mlp(cid, seed=NET_SEED):
    """PARITY_SCALE: a factor on the weights for a case the oracle's Newton does not solve with make_mlp's plain ones."""
    import cosserat_oracle as orc
    sizes, act = PARITY[cid]
    mlp = orc.make_mlp(list(sizes), act, seed=seed)
    s = PARITY_SCALE.get(cid, 1.0)
    if s != 1.0:
        mlp.weights = [(w * np.float32(s)).astype(np.float32) for w in mlp.weights]
    return mlp


@functools.lru_cache(maxsize=None)
def count_mlp(cid):
    import cosserat_oracle as orc
    sizes, act, gain = COUNT[cid]
    rng = np.random.default_rng(NET_SEED)
    Ws, bs, codes = [], [], []
    for k in range(len(sizes) - 1):
        W = (gain * rng.normal(0.0, 1.0, size=(sizes[k + 1], sizes[k])) / np.sqrt(sizes[k])).astype(np.float32)
        if k == 0:
            W[:, :3] = 0.0  # the network does not read p (module docstring)
        Ws.append(W)
        bs.append(rng.normal(0.0, 0.01, size=(sizes[k + 1],)).astype(np.float32))
        codes.append(orc._ACT_BY_NAME[act] if k < len(sizes) - 2 else orc.ACT_NONE)
    return orc.Mlp(Ws, bs, codes, False)


@functools.lru_cache(maxsize=None)
def controls(T):
    import cosserat_oracle as orc
    c = orc.batch_sine_controls(B, T, DEL_T, CTL_SEED)
    c.setflags(write=False)
    return c


def _tight(D, ctl, mlp, what):
    """float64[T + 1, 25, N]: entry t the state after step t (orc.simulate drops its last solve: one control repeated)."""
    import cosserat_oracle as orc
    traj, info = orc.simulate(D, np.vstack([ctl, ctl[-1:]]), mlp=mlp, solver="newton", return_info=True)
    assert np.all(info["ier"] == 1), (what, info["ier"])
    ref = np.ascontiguousarray(traj[:, :25])
    ref.setflags(write=False)
    return ref, info


@functools.lru_cache(maxsize=None)
def parity_rod(cid, N, b, mod=None, seed=NET_SEED):
    """(trajectory float64[T_PARITY + 1, 25, N], nfev per step) of rod b of ``controls(T_PARITY)`` with network ``seed`` of
    the case on parameter preset ``mod``."""
    import cosserat_oracle as orc
    ref, info = _tight(orc.setup_params(mod, N).derived(), controls(T_PARITY)[b], parity_mlp(cid, seed), (cid, N, b, mod, seed))
    return ref, tuple(int(n) for n in info["nfev"][:T_PARITY])


@functools.lru_cache(maxsize=None)
def plain_rod(N, b):
    """The same rod with the MLP off (how much a network matters)."""
    import cosserat_oracle as orc
    return _tight(orc.setup_params(None, N).derived(), controls(T_PARITY)[b], None, ("plain", N, b))[0]


def parity_case(cid, N):
    return [parity_rod(cid, N, b)[0] for b in range(B)]


def bank_case(cid, N=20):
    """Rod b: preset BANK_MODS[b], network BANK_NETS[b] of the bank (the case's shape at BANK_SEEDS)."""
    return [parity_rod(cid, N, b, BANK_MODS[b], BANK_SEEDS[BANK_NETS[b]])[0] for b in range(B)]


def parity_rows(cid, Q, N=20):
    """(y[Q, 19], yh[Q, 19], zh[Q, 6], tensions[Q, 4]): grid points of the case's oracle trajectory (rod 0), with the
    BDF2 history terms of knode.py:74-75, repeated cyclically up to Q rows."""
    import cosserat_oracle as orc
    ref = parity_rod(cid, N, 0)[0]
    D = orc.setup_params(None, N).derived()
    ctl = controls(T_PARITY)[0]
    ys, yhs, zhs, ts = [], [], [], []
    for t in range(2, T_PARITY + 1):
        hist = D.c1 * ref[t - 1] + D.c2 * ref[t - 2]
        for j in range(N - 1):
            ys.append(ref[t][:19, j])
            yhs.append(hist[:19, j])
            zhs.append(hist[19:, j])
            ts.append(ctl[t - 1])
    idx = (np.arange(Q) * 7) % len(ys)  # (7 and (T_PARITY - 1)(N - 1) are coprime at N = 20: Q distinct rows)
    pick = lambda a: np.ascontiguousarray(np.array(a)[idx])
    return pick(ys), pick(yhs), pick(zhs), pick(ts)


@functools.lru_cache(maxsize=None)
def count_ref(cid, b, N=20):
    """Tightly converged trajectory float64[T_COUNT + 1, 25, N] of rod b with the count network."""
    import cosserat_oracle as orc
    return _tight(orc.setup_params(None, N).derived(), controls(T_COUNT)[b], count_mlp(cid), (cid, b))[0]


class _Frozen:
    """Stands in for the network (``Mlp.tap``): records the outputs of a base sweep grid point by grid point and hands
    them back, in order, during a perturbed sweep."""

    def __init__(self, orc):
        self.orc = orc
        self.replay = False
        self.k = 0
        self.rec = []

    def start(self, replay):
        self.replay, self.k = replay, 0
        if not replay:
            self.rec = []

    def __call__(self, mlp, x):
        if self.replay:
            out = self.rec[self.k]
            self.k += 1
            return out
        a = x
        for W, b, act in zip(mlp.weights, mlp.biases, mlp.acts):
            a = self.orc._activate(act, W @ a + b)
        self.rec.append(a)
        return a


def newton_steps(D, ctl, tol, fd_eps, mlp=None, scheme="euler", fd_hist=None, fd_mid=None, fd_point=None, start=None,
                 on_sweep=None):
    """The BDF2 loop of orc.simulate with ``orc.newton_shoot`` at every step, counted: dict(iters=per-step iterations,
    ok=per-step convergence, base=per-step base / line-search sweeps, traj=float64[T + 1, 25, N], entry t the state after
    step t).  A step without backtracking has base == iters + 1 (the first residual, one full step per iteration but the
    last, the final sweep).  The hooks change the six PERTURBED sweeps of an iteration (``fun_fd``) or the start of a
    step, never a base sweep: the root stays what it is (tests/sweep_count_cases.py builds its mutants from them).

    * ``fd_hist(yh, zh, y_cur, z_cur, y_old, z_old) -> (yh, zh)``: the histories a perturbed sweep reads;
    * ``fd_mid(yh, zh) -> (yh_int, zh_int)``: RK4, the midpoint histories of a perturbed sweep (default: knode.simulate's
      means of neighbours, of the histories the perturbed sweep reads).  With either of the two the Jacobian is that of the
      ALTERED sweep: its columns are the altered sweep's difference quotients against the altered sweep at the base point
      (one more sweep per iteration), put on the true residual - what a solver whose Jacobian sweeps all read the wrong
      history computes.  (Against the true base sweep the difference of the two sweeps would be divided by the step.);
    * ``fd_point(G_base, G_perturbed) -> G``: the point a perturbed sweep starts from (the quotient keeps its step);
    * ``start(t, Gs) -> G``: the start of step t from ``Gs``, the (n, m) at the base of states t, t - 1, .. 0 (``Gs[0]``
      is also the G the previous step accepted: a sweep writes its G there); default: the warm start ``Gs[0]``;
    * ``on_sweep(perturbed)``: called before every sweep."""
    import cosserat_oracle as orc
    own_base = fd_hist is not None or fd_mid is not None
    y, z = orc.straight_state(D)
    y_prev, z_prev = y.copy(), z.copy()
    G = np.zeros(6)
    Gs = [G.copy()]
    iters, oks, bases, traj = [], [], [], [np.vstack([y, z])]
    mids = lambda a, c: (0.5 * (a[:, :-1] + a[:, 1:]), 0.5 * (c[:, :-1] + c[:, 1:]))   # knode.py:80-81
    for t, tensions in enumerate(ctl):
        yh = D.c1 * y + D.c2 * y_prev
        zh = D.c1 * z + D.c2 * z_prev
        yh_fd, zh_fd = (yh, zh) if fd_hist is None else fd_hist(yh, zh, y.copy(), z.copy(), y_prev, z_prev)
        y_prev, z_prev = y.copy(), z.copy()
        if scheme == "rk4":
            yi, zi = mids(yh, zh)
            yi_fd, zi_fd = (fd_mid or mids)(yh_fd, zh_fd)
        elif scheme != "euler":
            raise ValueError(scheme)
        n_base, at = [0], [None, None, None, None]  # (at: base point, its residual; the altered sweep's base point, residual)

        def sweep(g, yh, zh, yi, zi):
            if scheme == "euler":
                return orc.residual_euler(D, g, y, z, yh, zh, tensions, mlp)
            return orc.residual_rk4(D, g, y, z, yh, yi, zh, zi, tensions, mlp)

        def base(g):
            n_base[0] += 1
            at[0] = np.array(g, float)
            if on_sweep is not None:
                on_sweep(False)
            at[1] = sweep(g, yh, zh, *((yi, zi) if scheme == "rk4" else (None, None)))
            return at[1]

        def perturbed(g):
            if on_sweep is not None:
                on_sweep(True)
            if fd_point is not None:
                g = fd_point(at[0], g)
            r = sweep(g, yh_fd, zh_fd, *((yi_fd, zi_fd) if scheme == "rk4" else (None, None)))
            if own_base:  # the quotient of the altered sweep against ITS OWN value at the base point
                if at[2] is not at[0]:
                    at[2], at[3] = at[0], sweep(at[0], yh_fd, zh_fd, *((yi_fd, zi_fd) if scheme == "rk4" else (None, None)))
                r = at[1] + (r - at[3])
            return r

        if start is not None:
            G = np.array(start(t, Gs), float)
        G, ok, it = orc.newton_shoot(base, G, tol=tol, fd_eps=fd_eps, fun_fd=perturbed)
        Gs.insert(0, np.array(G))
        iters.append(it)
        oks.append(bool(ok))
        bases.append(n_base[0])
        traj.append(np.vstack([y, z]))
    return dict(iters=tuple(iters), ok=tuple(oks), base=tuple(bases), traj=np.array(traj))


@functools.lru_cache(maxsize=None)
def sweep_counts(cid, b, dtype, frozen, N=20):
    """dict(iters=per-step newton_shoot iterations, ok=per-step convergence, base=per-step base / line-search sweeps):
    ``newton_steps`` from the reference's warm start, at the stopping rule of ``dtype``."""
    import copy

    import cosserat_oracle as orc
    rule = RULE[dtype]
    D = orc.setup_params(None, N).derived()
    mlp = copy.copy(count_mlp(cid))
    tap = _Frozen(orc) if frozen else None
    mlp.tap = tap
    out = newton_steps(D, controls(T_COUNT)[b], rule["tol"], rule["fd_eps"], mlp=mlp,
                       on_sweep=None if tap is None else tap.start)
    return dict(iters=out["iters"], ok=out["ok"], base=out["base"])


def count_sums(cid, b, dtype):
    """(S_full, S_frozen) of rod b."""
    return sum(sweep_counts(cid, b, dtype, False)["iters"]), sum(sweep_counts(cid, b, dtype, True)["iters"])


def count_bound(cid, b, dtype):
    s_full, s_frozen = count_sums(cid, b, dtype)
    return s_full + T_COUNT + (s_frozen - s_full) / 3.0
