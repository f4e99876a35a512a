"""Every step kernel against an independent answer over a FULL-LENGTH run (``-m gpu``, through the C ABI).

The BASELINE configurations run 200 steps (cfg2: N = 100), 64 steps with the MLP in every sweep (cfg3: N = 100) and 100
steps (cfg5: N = 400).  What the persistent kernels carry from step to step - the ``t & 1`` tile parity, the ring slot,
the fitted-recurrence predictor, lean ring steps that store no interior record, the roll-back and the plain-step ladder,
the take-over at ``resume[rod]``, with the MLP on the low-precision first sweeps - can only go wrong deep into a run, and
a stale tile then still yields status 0 and an accepted root, of the wrong problem.  So:

(a) ``test_reference_*``: the three runs the unmodified reference solved throughout (``ier == 1`` at every step;
    tests/golden/sim_long_*.npz, tests/long_run_cases.py) through every kernel that serves them, in fp64 and fp32, in up to
    three call forms - ``full``: one call that writes every state; ``ring``: one call on a 3-slot ring, tips only;
    ``driver``: 20-step calls on a ring with ``keep_predictor = 1`` and ``prev_init`` pointing into the ring, the form
    bench.py times.  Every form is compared with the reference, never with another form.
(b) ``test_rough_*``: twelve rods, four of them smooth, four with one tension jump in the last third of the run, four with
    fresh random tensions at every one of the last 30 steps - the kind of input tools/soak_rough.py uses to force
    roll-backs and plain steps (no release build reports whether one ran, and nothing here claims it did).  The reference's
    fsolve gives up on such inputs; the answer is the C oracle's damped Newton (pinned to the reference on the short step /
    random fixtures and on the long runs above by tests/test_oracle_golden.py), on the rods where it converged at every
    step - at least ten of the twelve (all twelve with the committed seeds).

Bounds.  fp64: tips per window 1e-8 (the reference stops at xtol 1.5e-8), stored states 1e-7, every status 0.  fp32: tips
per window 1e-5 (the contract of BASELINE.json), every status 0; the stored states are not under that contract and are
held to 1e-4 of the state's norm, chosen before anything was measured: a sweep is N - 1 dependent Euler steps, whose
rounding may add up to N u = 2.4e-5 at N = 400 (u = 6e-8), and the velocity rows are history differences scaled by
c0 = 30 / s; a stale tile or a ring slot one step off is the motion of a step away, 1e-2 and more.  Windows: 50 steps (16
with the MLP on).  Every case asserts the kernel that ran: ``last_sim_path``, ``last_waves_per_rod``, ``last_overlap``.
Measured window errors: LABBOOK.md (long runs)."""
import numpy as np
import pytest

import long_run_cases as lc
from conftest import rel_l2
from gpu_helpers import inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 20  # steps per call of the driver's form (bench.py --steps 20)

# kernel -> (mode of gpu_helpers.set_mode_env, waves_per_rod, handle options, call kind, (path, waves per rod, overlap) that
# must have run).  Call kinds: plain, table (one row per rod), loads (each row's own zero wrench as loads[b][t]), bank1 (one
# network), bank2 (two identical networks, net_of_rod = [0, 1]).
KERNELS = {
    "K2a": ("single", 1, {}, "plain", (0, 1, 0)),
    "K2b": ("multi", 1, {}, "plain", (1, 1, 0)),
    "K2c": ("persistent", 1, {}, "plain", (2, 1, 0)),
    "K2e": ("overlap", 1, {}, "plain", (2, 1, 1)),
    "K2d-step-W2": ("multi", 2, {}, "plain", (1, 2, 0)),
    "K2d-step-W4": ("multi", 4, {}, "plain", (1, 4, 0)),
    "K2d-W2": ("persistent", 2, {"msw_overlap": 0}, "plain", (2, 2, 0)),
    "K2d-W4": ("persistent", 4, {"msw_overlap": 0}, "plain", (2, 4, 0)),
    "K2f-W2": ("persistent", 2, {"msw_overlap": 1}, "plain", (2, 2, 1)),
    "K2f-W4": ("persistent", 4, {"msw_overlap": 1}, "plain", (2, 4, 1)),
    "table-K2e": ("overlap", 1, {"overlap": 1}, "table", (2, 1, 1)),
    "table-K2c": ("overlap", 1, {"overlap": 0}, "table", (2, 1, 0)),
    "loads-K2e": ("overlap", 1, {"overlap": 1}, "loads", (2, 1, 1)),
    "loads-K2c": ("overlap", 1, {"overlap": 0}, "loads", (2, 1, 0)),
    # MLP on (the overlapped kernels do not evaluate a network: "overlap" stays 0)
    "mswn-W2": ("persistent", 2, {}, "plain", (2, 2, 0)),
    "mswn-W4": ("persistent", 4, {}, "plain", (2, 4, 0)),
    "table-nn": ("persistent", 1, {}, "table", (2, 1, 0)),
    "bank1": ("overlap", 1, {}, "bank1", (2, 1, 0)),
    "bank2": ("overlap", 1, {}, "bank2", (2, 1, 0)),
}
ALL_FORMS = ("full", "ring", "driver")


def _cases(kernels_full, kernels_all_forms):
    return [(k, "full") for k in kernels_full] + [(k, f) for k in kernels_all_forms for f in ALL_FORMS]


N100 = _cases(["K2a", "K2b", "K2d-W2", "K2d-W4", "table-K2e", "table-K2c", "loads-K2e", "loads-K2c"],
              ["K2c", "K2e", "K2f-W2", "K2f-W4"])
N400 = _cases(["K2b", "K2d-step-W2", "K2d-step-W4", "K2d-W2", "K2d-W4"], ["K2f-W2", "K2f-W4"])
NN = _cases(["K2a", "K2b", "mswn-W2", "mswn-W4", "table-nn", "bank1", "bank2"], ["K2c"])
ROUGH100 = [(k, f) for k in ("K2c", "K2e", "K2f-W2", "K2f-W4", "table-K2e") for f in ("full", "ring")]
ROUGH400 = [(k, f) for k in ("K2f-W2", "K2f-W4") for f in ("full", "ring")]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def run(torch, monkeypatch, case, kernel, form, dtype):
    """-> (tips [B, T, 3], status [B, T], {entry: states [B, 25, N]} of the entries the case stores) of one run of the case's
    controls from the straight rod; asserts the kernel after every call."""
    mode, W, options, kind, ran = KERNELS[kernel]
    set_mode_env(monkeypatch, mode, waves_per_rod=W)
    N, T, B = case["N"], case["T"], case["B"]
    mlp = case.get("mlp")
    carrier = make_robot(None, N)
    if mlp is not None and not kind.startswith("bank"):
        inject(carrier, mlp)
    h = carrier._native()
    for k, v in options.items():
        h.set_option(k, v)
    dt = torch.float64 if dtype == "f64" else torch.float32
    ctl = torch.as_tensor(np.ascontiguousarray(case["ctl"]), device=DEV).to(dt).contiguous()
    kw = {}
    opened = []
    if kind != "plain":
        opened.append(h.param_table([carrier._params()] * B))
        kw["table"] = opened[0]
    if kind.startswith("bank"):
        K = int(kind[4:])
        opened.append(h.mlp_bank([(mlp.weights, mlp.biases, mlp.acts)] * K))
        kw.update(bank=opened[1], net_of_rod=list(range(K)) if K == B else [0] * B)
    elif mlp is not None:
        kw["use_nn"] = True
    loads = torch.zeros((B, T, 6), dtype=dt, device=DEV) if kind == "loads" else None  # (the rows' own wrench: zero)

    def check_kernel():
        got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
        assert got == ran, f"{kernel}: (path, waves per rod, overlap) = {got}, the test is meant to exercise {ran}"

    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), float("nan"), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    st = h.new_state(B, dt, n_slots=T + 1 if form == "full" else 3)
    h.init_straight(st[0], table=kw.get("table"))
    stored = {}
    try:
        if form != "driver":
            h.simulate(ctl, st, G, ring=form == "ring", tip=tip, status=status, loads=loads, **kw)
            torch.cuda.synchronize()
            check_kernel()
            last = T  # entry e sits in slot e (full) or e % 3 (ring: T, T - 1, T - 2 only)
            slot = (lambda e: e) if form == "full" else (lambda e: e % 3)
        else:
            h.set_option("keep_predictor", 0)  # (drops a stored image)
            h.set_option("keep_predictor", 1)
            prev, a = None, 0
            while a < T:
                n = min(CHUNK, T - a)
                tp = torch.full((B, n, 3), float("nan"), dtype=dt, device=DEV)
                sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
                h.simulate(ctl[:, a:a + n].contiguous(), st, G, ring=True, tip=tp, status=sx, prev_init=prev,
                           loads=None if loads is None else loads[:, a:a + n].contiguous(), **kw)
                torch.cuda.synchronize()
                check_kernel()
                tip[:, a:a + n], status[:, a:a + n] = tp, sx
                a += n
                if a < T:
                    # the call left the newest state in slot n % 3 and the one before it in slot (n - 1) % 3; the next call starts
                    # from slot 0 again, with the older state in slot 2 of the ring itself (knode_rod.h: prev_init may point
                    # into the ring; slot 2 is written by the call's second step)
                    newest, older = st[n % 3].clone(), st[(n - 1) % 3].clone()
                    st[0].copy_(newest)
                    st[2].copy_(older)
                    prev = st[2]
            last = T
            slot = lambda e: (e - (T - n)) % 3
        for e in case["states"]:
            if e > 0 and (form == "full" or e >= last - 2):
                y, z = h.unpack(st[slot(e)])
                stored[e] = torch.cat([y, z], dim=1).double().cpu().numpy()
    finally:
        h.set_option("keep_predictor", 0)
        for o in reversed(opened):
            o.close()
    return tip.double().cpu().numpy(), status.cpu().numpy(), stored


def check(label, case, dtype, tips, status, stored, rods=None):
    """The bounds of the module docstring on the rods ``rods`` (default: all); prints every figure before it asserts."""
    tip_tol, state_tol = (1e-8, 1e-7) if dtype == "f64" else (1e-5, 1e-4)
    rods = range(case["B"]) if rods is None else rods
    L = case["tip"].shape[1]
    worst, lines = 0.0, []
    for b in rods:
        errs = lc.window_errors(tips[b, : L - 1], case["tip"][b, 1:], case["window"])
        serr = {e: rel_l2(s[b], case["states"][e][b]) for e, s in stored.items()}
        lines.append((b, errs, serr))
        print(f"{label} rod {b}: tip windows {' '.join('%.1e' % e for e in errs)} | states "
              f"{' '.join('%d:%.1e' % kv for kv in sorted(serr.items()))} | status != 0 at {np.flatnonzero(status[b]).tolist()[:8]}")
    for b, errs, serr in lines:
        bad = np.flatnonzero(status[b])
        assert bad.size == 0, f"{label} rod {b}: status {status[b][bad].tolist()} at steps {bad.tolist()}"
        assert np.all(np.isfinite(tips[b]))
        assert max(errs) < tip_tol, f"{label} rod {b}: tip windows {errs}"
        assert all(v < state_tol for v in serr.values()), f"{label} rod {b}: states {serr}"
        worst = max(worst, max(errs))
    return worst


def _reference(torch, monkeypatch, name, kernel, form, dtype):
    case = lc.long_case(name)
    tips, status, stored = run(torch, monkeypatch, case, kernel, form, dtype)
    if form == "full":
        assert set(stored) == {e for e in case["states"] if e > 0}
    else:
        assert set(stored) == {case["T"] - 1}  # (the reference's last entry is state T - 1: still in the ring)
    check(f"{name} {kernel} {form} {dtype}", case, dtype, tips, status, stored)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,form", N100)
def test_reference_n100_200_steps(torch_cuda, monkeypatch, kernel, form, dtype):
    """cfg2 at its length: rod A (rod 0 of the cfg2 draw, smooth) and rod B (the same with + 0.5 N on tendon 0 from step 120
    and - 0.5 N on tendon 2 from step 170) in one batch."""
    _reference(torch_cuda, monkeypatch, "n100", kernel, form, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,form", N400)
def test_reference_n400_100_steps(torch_cuda, monkeypatch, kernel, form, dtype):
    """cfg5 at its length.  The persistent overlapped kernels take their tiles from the states at this N by default (the GT
    instantiations); ``KR_MSWO_GT`` is read once per process, nothing is asserted about it."""
    _reference(torch_cuda, monkeypatch, "n400", kernel, form, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,form", NN)
def test_reference_nn_64_steps(torch_cuda, monkeypatch, kernel, form, dtype):
    """cfg3 at its length: the network 28 -> 64 -> 64 -> 25 in every sweep, rods 3 and 1000 of the cfg3 draw.  The only
    several-wavefront form with the MLP on is the persistent one (kr_mswn_*.hip), at W = 2 and 4."""
    _reference(torch_cuda, monkeypatch, "nn", kernel, form, dtype)


def _rough(torch, monkeypatch, N, kernel, form, dtype):
    case = lc.rough_case(N)
    good = np.flatnonzero(case["good"])
    assert len(good) >= lc.ROUGH_MIN_GOOD
    tips, status, stored = run(torch, monkeypatch, case, kernel, form, dtype)
    check(f"rough N={N} {kernel} {form} {dtype}", case, dtype, tips, status, stored, rods=good)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,form", ROUGH100)
def test_rough_n100_200_steps(torch_cuda, monkeypatch, kernel, form, dtype):
    _rough(torch_cuda, monkeypatch, 100, kernel, form, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,form", ROUGH400)
def test_rough_n400_100_steps(torch_cuda, monkeypatch, kernel, form, dtype):
    _rough(torch_cuda, monkeypatch, 400, kernel, form, dtype)
