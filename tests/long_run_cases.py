"""Shared by tests/test_oracle_golden.py and tests/test_gpu_long_runs.py (not a test module): the three reference runs at
the lengths the BASELINE configurations run (tests/golden/sim_long_*.npz, written by make_golden.py from the unmodified
reference), the windows a tip path is compared in, and the batch of rough inputs whose answer is the C oracle's.

A case is a dict: ``N``, ``T``, ``ctl[B, T, 4]``, ``tip[B, L, 3]`` (entry 0 = the initial tip, entry t = the state after
solve t - 1; L = T for the reference, which drops its last solve, knode.py:96-102, and T + 1 for the C oracle),
``states`` = {entry index: [B, 25, N]} and ``window``.  A kernel's ``tip[b, t]`` is the tip after solve t, i.e. entry
t + 1: ``got[:, :L - 1]`` against ``tip[:, 1:]``."""
import numpy as np

from conftest import load_golden

DEL_T = 0.05  # every preset's time step (knode.setup_robot)


def windows(n, width):
    """[(a, b)] cutting range(n) into windows of ``width`` entries (the last one shorter)."""
    return [(a, min(a + width, n)) for a in range(0, n, width)]


def window_errors(got, ref, width):
    """Relative L2 error of a tip path [n, 3] per window, and over the whole run (last entry)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    errs = [float(np.linalg.norm(got[a:b] - ref[a:b]) / np.linalg.norm(ref[a:b])) for a, b in windows(len(ref), width)]
    return errs + [float(np.linalg.norm(got - ref) / np.linalg.norm(ref))]


def long_case(name):
    g = load_golden("sim_long_" + name)
    assert np.all(g["ier"] == 1), name
    if name == "n100":
        tip, B = g["tip"], g["tip"].shape[0]
        T = tip.shape[1]
        states = {20 * k: g["every20"][:, k] for k in range(g["every20"].shape[1])}
        states[T - 1] = g["last"]
        return dict(name=name, N=100, T=T, ctl=g["ctl"], tip=tip, states=states, window=50, B=B, jump_a=float(g["jump_a"]))
    if name == "n400":
        T = g["tip"].shape[0]
        states = {25 * k: g["every25"][None, k] for k in range(g["every25"].shape[0])}
        states[T - 1] = g["last"][None]
        return dict(name=name, N=400, T=T, ctl=g["ctl"][None], tip=g["tip"][None], states=states, window=50, B=1)
    if name == "nn":
        import cosserat_oracle as orc
        T = g["tip"].shape[1]
        states = {8 * k: g["every8"][:, k] for k in range(g["every8"].shape[1])}
        states[T - 1] = g["last"]
        return dict(name=name, N=100, T=T, ctl=g["ctl"], tip=g["tip"], states=states, window=16, B=g["tip"].shape[0],
                    mlp=orc.mlp_from_arrays(g, "mlp"), rods=[int(b) for b in g["rods"]])
    raise ValueError(name)


# ---------------------------------------------------------------------------
# rough inputs late in a run: B = 12 rods whose answer is the C oracle's damped Newton (the reference's fsolve gives up on
# such inputs; the oracle is pinned to it on the short step / random fixtures)
# ---------------------------------------------------------------------------
ROUGH = {100: dict(T=200, seed=20), 400: dict(T=100, seed=21)}
ROUGH_B = 12
ROUGH_MIN_GOOD = 10  # at least this many of the twelve rods must be rods the oracle converged on at every step


def rough_controls(N):
    """ctl[12, T, 4]: rods 0..3 smooth (the cfg2 draw); 4..7 one jump of U(-2, 2) N on one tendon from a step of the last
    third of the run on; 8..11 fresh 5 + 5 U(0, 1) tensions at every step of the last 30 steps only."""
    import cosserat_oracle as orc
    T, seed = ROUGH[N]["T"], ROUGH[N]["seed"]
    ctl = orc.batch_sine_controls(256, T, DEL_T, 1234)[:ROUGH_B].copy()
    rng = np.random.default_rng(seed)
    for b in range(4, 8):
        t0 = int(rng.integers(T - T // 3, T - 1))
        ctl[b, t0:, int(rng.integers(4))] += rng.uniform(-2.0, 2.0)
    for b in range(8, 12):
        ctl[b, T - 30:] = 5.0 + 5.0 * rng.uniform(size=(30, 4))
    ctl.setflags(write=False)
    return ctl


_rough_cache = {}


def rough_case(N):
    """The rough batch with the C oracle's answer, computed once per process: ``tip[B, T + 1, 3]`` (entry 0 = the initial
    tip, all T solves), ``states`` at every 20th entry and the last, ``good[B]`` = the oracle converged at every step."""
    if N in _rough_cache:
        return _rough_cache[N]
    import cosserat_oracle as orc
    import cosserat_oracle_c as oc
    ctl = rough_controls(N)
    T = ctl.shape[1]
    P = orc.params_for(None, N)
    keep = sorted(set(range(0, T + 1, 20)) | {T})
    tips, states, good = [], {k: [] for k in keep}, []
    for b in range(ROUGH_B):
        tip, tr, bad = oc.simulate(P, ctl[b])
        tips.append(np.concatenate([tr[0, :3, -1][None], tip]))
        good.append(bad == 0 and bool(np.all(np.isfinite(tr))))
        for k in keep:
            states[k].append(tr[k])
    case = dict(name=f"rough{N}", N=N, T=T, B=ROUGH_B, ctl=ctl, tip=np.array(tips), window=50,
                states={k: np.array(v) for k, v in states.items()}, good=np.array(good))
    _rough_cache[N] = case
    return case
