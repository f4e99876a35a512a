"""A failing rod in a batch, on every step kernel (``-m gpu``, through the C ABI).

knode_rod.h (kr_step_batch / kr_simulate_batch) and DESIGN section 6 state what a step leaves behind whose inputs are not
finite; these tests pin it.  Every case builds a clean input set and its sick twin (tests/sick_rod_cases.py: ONE entry of
ONE rod ``s`` differs, first read by the solve of step ``t0``), runs the clean call, the sick call and the clean call again
on the SAME handle, every output a view into a larger buffer of sentinels, and asserts
  a. all calls return KR_OK and no ``status`` entry is left at its sentinel;
  b. the clean call converges everywhere (``status == 0``);
  c. the healthy rods of the sick call equal the clean call BIT FOR BIT: status, tip, G, every state slot;
  d. so does the sick rod before t0 (ring runs: status and tips; full runs also states 0 .. t0);
  e. the sick rod reports 2 at t0 for the NaN kinds (nonzero for ``overflow_ctl``) and 1 or 2 on every later step - except
     ``nan_load``, the documented exception: a tip wrench enters the tip condition only, never a sweep, so the state stored
     for the failed step is the (finite) sweep of the last finite iterate and later steps, whose inputs are finite again,
     may report 0; what is pinned there is 2 at t0 and finite states throughout;
  f. the guards around every output are untouched, slots 25..27 of every healthy rod are zero;
  g. the third call equals the first bit for bit: nothing stale is left in the per-handle scratch, the history workspace
     or the predictor buffer.  The third call's output buffers (state slots 1 .., tips) are filled with NaN beforehand:
     no kernel may read a state before it has written it.  (What a previous launch left in the LDS is not under a test's
     control; run in file order a handle's first call follows the sick call of the case before, which is incidental.)
The reference of (c), (d), (g) is the library's own clean call - the property is independence, there is no tolerance; that
the clean inputs converge and the sick ones defeat a plain Newton solve is shown on the CPU oracle by
tests/test_sick_rod_cpu.py.  Every case asserts WHICH kernel ran.

Why each family ends when its norms are NaN (read from the kernels before the first run; no float-to-int conversion of a
value that can be NaN is used as an index or a trip count: the ``(int)`` casts of ``ms_pred_load`` read back what
``ms_pred_save`` wrote from integers - avail, next_order, lp_age, lp_good -, the predictor's order choice compares
``update_ratio`` values, which are +inf for a NaN, with ``<``, and every sweep's trip count comes from N):
  K2a  step_kernel (kr_sim_impl.hpp): ``!(nr <= nr_old ...)`` is true on a NaN norm, but backtracking needs
       ``have_trial``, ``lam > 1/1024`` and ``cnt < maxit`` - at most ten halvings per update and never past the cap; a NaN
       update takes the ``!finite`` branch (done, status 2); ``__all(done)`` then starts the damped phase ONCE (``damped``
       is wave-uniform and never cleared) for the rods that failed, their first sweep there is ``!finite`` again; after
       the second ``__all(done)`` at most one flush pass runs and the loop breaks.  A done rod keeps sweeping but stores
       nothing (``st`` needs ``!done``).
  K2b / K2c  ms_newton, ss_newton_damped (kr_ms_impl.hpp): one rod per wavefront, no workgroup barrier.  ``dnf`` is a
       wave maximum of ``update_ratio`` (+inf for a NaN), ``finite = dnf <= 3e38`` fails, the solve is done with status 2
       and one flush sweep; the inner chord / defect-correction loop only ever goes round on one-way flags (``pcorr``,
       ``chord = false``).  The ladder is predicted start -> warm start (``order = 0`` ends it) -> damped single shooting,
       whose first update is not finite (break) and whose backtracking is bounded like K2a's.  The time loop counts t.
  K2e  mso_sim_kernel (kr_mso_impl.hpp): every pass of its loop either accepts step tB, spends the one ``reverify`` of a
       step, rolls back to tB (plain sweeps from there: ``it`` counts up to maxit), retries from the warm start once
       (``retried``), hands a step over, or breaks with ``resume_at``.  A NaN in the forward-difference lanes of step tA
       makes ``finite`` false: one retry, then ``resume_at = tA``; the verdict of step tB = tA - 1 is formed before that
       from the verifying lanes' own end states (XsB / EsB).  The take-over launch (ms_sim_kernel) starts at
       ``resume[rod]``, rods with ``resume >= T`` leave at once.
  K2d / mswn  msw_newton, msw_ss_damped (kr_msw_impl.hpp): one rod per workgroup; every decision variable (``U.dnf``, the
       residual estimate) comes out of ``msw_max``, a reduction over the workgroup of values that are +inf for a NaN, so
       all wavefronts take the same branch; the damped phase runs on wavefront 0 between two ``__syncthreads`` and hands
       its status to the others through the LDS.
  K2f  mswo_sim_kernel (kr_mswo_impl.hpp): the loop of K2e with workgroup-uniform decisions; where K2e gives a rod up it
       calls ``plain_step`` (the ladder of K2d) in place, which always advances tA.
  MLP on: the evaluators (mlp_jvp.hpp, mlp_mfma.hpp) have fixed trip counts; a NaN only travels through their tiles,
       which every evaluation rewrites before it reads them.

Sick-rod scores of the Python front end (last test): with a NaN tension the rod's states are NaN from t0 + 1 on, and its
``dtw`` and ``mse`` are NaN - the last compared sample is NaN, so the last DTW cell is ``NaN + min(...)``, and the MSE is a
plain sum over terms some of which are NaN.  With a NaN tip load the states stay finite (e. above): ``dtw`` and ``mse`` are
finite numbers, of a trajectory that ``status`` 2 at t0 marks as not the rod's."""
import numpy as np
import pytest

import sick_rod_cases as sc
from conftest import load_golden
from gpu_helpers import assert_path, inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64       # elements in front of and behind every output (a multiple of 16 bytes in both types)
FSENT = -7.25    # sentinel of the floating-point buffers
ISENT = -7       # ... of status / iters
KEYS = ("status", "tip", "G", "states")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def tdtype(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def dev(torch, x, dt):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dt).contiguous()


class Guarded:
    """A tensor that is a view into a larger buffer of sentinels."""

    def __init__(self, torch, shape, dtype, sentinel, fill=None):
        self.n = int(np.prod(shape))
        self.sentinel = sentinel
        self.buf = torch.full((self.n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all() and (self.buf[GUARD + self.n:] == self.sentinel).all())


def call(torch, h, inp, dt, ring=False, table=None, loads=False, bank=None, net_of_rod=None, use_nn=False, scheme=0,
         maxit=0, chunks=None, poison=False):
    """One kr_simulate_batch* call from the straight rod (or one per chunk, the state before handed over as
    tests/test_gpu_tip_loads.py::test_calls_in_pieces does) into guarded outputs; NumPy arrays in the call's own type.
    poison: every state slot but the initial one and the tips hold NaN when the call starts."""
    ctl = dev(torch, inp["ctl"], dt)
    L = dev(torch, inp["loads"], dt) if loads else None
    B, T = ctl.shape[0], ctl.shape[1]
    assert not (ring and chunks)
    st = Guarded(torch, (3 if ring else T + 1, B, h.N, 28), dt, FSENT, fill=0.0)  # (Handle.new_state: zeros)
    G = Guarded(torch, (B, 6), dt, FSENT, fill=0.0)                                # (knode.py:67: the first guess)
    tip = Guarded(torch, (B, T, 3), dt, FSENT)
    status = Guarded(torch, (B, T), torch.int32, ISENT)
    h.init_straight(st.t[0], table=table)
    if poison:
        st.t[1:].fill_(float("nan"))
        tip.t.fill_(float("nan"))
    kw = dict(table=table, bank=bank, net_of_rod=net_of_rod, scheme=scheme, maxit=maxit)
    if bank is None:
        kw["use_nn"] = use_nn
    if chunks is None:
        h.simulate(ctl, st.t, G.t, ring=ring, tip=tip.t, status=status.t, loads=L, **kw)  # (raises unless KR_OK)
    else:
        a = 0
        for n in chunks:
            tp = Guarded(torch, (B, n, 3), dt, FSENT, fill=float("nan") if poison else None)
            sx = Guarded(torch, (B, n), torch.int32, ISENT)
            h.simulate(ctl[:, a:a + n].contiguous(), st.t[a:], G.t, tip=tp.t, status=sx.t,
                       prev_init=st.t[a - 1] if a else None, loads=None if L is None else L[:, a:a + n].contiguous(), **kw)
            torch.cuda.synchronize()
            assert tp.intact() and sx.intact()
            tip.t[:, a:a + n] = tp.t
            status.t[:, a:a + n] = sx.t
            a += n
        assert a == T
    torch.cuda.synchronize()
    out = dict(status=status.t.cpu().numpy(), tip=tip.t.cpu().numpy(), G=G.t.cpu().numpy(), states=st.t.cpu().numpy())
    out["guards"] = st.intact() and G.intact() and tip.intact() and status.intact()
    return out


def same(a, b, rods, what):
    for k in KEYS:
        x, y = (a[k][:, rods], b[k][:, rods]) if k == "states" else (a[k][rods], b[k][rods])
        assert np.array_equal(x, y), f"{what}: {k} differs at {np.argwhere(x != y)[:4].tolist()}"


def check_triple(label, clean, sick, again, kind, s, t_sick, ring):
    """Assertions a - g of the module docstring on one clean / sick / clean triple."""
    B, T = clean["status"].shape
    healthy = np.arange(B) != s
    for name, o in (("clean", clean), ("sick", sick), ("clean again", again)):
        assert np.all((o["status"] >= 0) & (o["status"] <= 2)), f"{label} {name}: status {o['status'].tolist()}"  # a
        assert o["guards"], f"{label} {name}: a guard was written"                                               # f
        assert np.all(o["states"][:, healthy][..., 25:] == 0), f"{label} {name}: padding slots"
    assert np.all(clean["status"] == 0), f"{label}: clean status {clean['status'].tolist()}"                    # b
    same(sick, clean, healthy, f"{label}: healthy rods, sick call against clean call")                          # c
    assert np.all(np.isfinite(sick["tip"][healthy])) and np.all(np.isfinite(sick["states"][:, healthy]))
    assert not np.any(sick["tip"][healthy] == FSENT)
    got = sick["status"][s]
    print(f"{label}: sick rod {s} status {got.tolist()}")
    assert np.array_equal(got[:t_sick], clean["status"][s, :t_sick]), f"{label}: status before t0 {got.tolist()}"  # d
    assert np.array_equal(sick["tip"][s, :t_sick], clean["tip"][s, :t_sick]), f"{label}: tips before t0"
    if not ring:
        assert np.array_equal(sick["states"][:t_sick + 1, s], clean["states"][:t_sick + 1, s]), f"{label}: states before t0"
    if kind == "overflow_ctl":  # (nonzero, not necessarily 2 - the tension enters the sweeps: nonzero ever after)       # e
        assert np.all((got[t_sick:] == 1) | (got[t_sick:] == 2)), f"{label}: status {got.tolist()}"
    elif kind == "nan_load":  # (the wrench reaches no sweep: module docstring)
        assert got[t_sick] == 2, f"{label}: status {got.tolist()}"
        assert np.all(np.isfinite(sick["states"][:, s])) and np.all(np.isfinite(sick["tip"][s])), f"{label}: sick rod's states"
    else:
        assert got[t_sick] == 2 and np.all((got[t_sick:] == 1) | (got[t_sick:] == 2)), f"{label}: status {got.tolist()}"
    same(again, clean, np.arange(B), f"{label}: third call against the first")                                  # g


def ring_is_complete(label, ringed, full, rods, dt_name):
    """The three slots of a ring call hold the last three states of the full-trajectory call (the project's bar between
    two persistent forms, tests/test_gpu_msw.py: 1e-6 fp64, 1e-3 fp32 of the largest entry; a slot one step stale is off
    by the motion of a step, 1e-2 and more)."""
    T = full["states"].shape[0] - 1
    for k in (T, T - 1, T - 2):
        a, b = ringed["states"][k % 3][rods].astype(np.float64), full["states"][k][rods].astype(np.float64)
        err = np.max(np.abs(a - b)) / np.max(np.abs(b))
        assert err < (1e-6 if dt_name == "f64" else 1e-3), f"{label}: ring slot of state {k}: {err:.2e}"


def triples(torch, h, label, family, dt_name, ran, kinds=("nan_ctl",), t0s=(sc.T0,), rings=(False,), full_clean=None, **kw):
    """clean / sick / clean on one handle for every (ring, kind, sick rod, t0); ``ran()`` asserts the kernel after each call."""
    dt = tdtype(torch, dt_name)
    N, B, T, sick_rods = sc.SHAPES[family]
    c = sc.clean_set(family)
    for ring in rings:
        for kind in kinds:
            if kind == "overflow_ctl" and dt_name != "f64":
                continue  # (1e200 is not an fp32 number)
            for s in sick_rods:
                for t0 in t0s:
                    if t0 != sc.T0 and (kind != "nan_ctl" or s != sick_rods[0]):
                        continue
                    tag = f"{label} {dt_name} ring={int(ring)} {kind} s={s} t0={t0}"
                    tw = sc.sick_twin(c, kind, s, t0)
                    outs = []
                    for k, inp in enumerate((c, tw, c)):
                        outs.append(run_inputs(torch, h, inp, dt, ring, poison=k == 2, **kw))
                        ran()
                    check_triple(tag, *outs, kind, s, sc.first_sick_step(kind, t0), ring)
                    if not ring:
                        full_clean = outs[0]
                    elif full_clean is not None:
                        healthy = np.arange(B) != s
                        ring_is_complete(tag + " sick call", outs[1], full_clean, healthy, dt_name)
                        ring_is_complete(tag + " clean call", outs[0], full_clean, np.arange(B), dt_name)


def run_inputs(torch, h, inp, dt, ring, rows=None, loads=False, bank_nets=None, **kw):
    """``call`` with the table (rows: the presets of sick_rod_cases.MODS5, each with the wrench the input set gives it) and
    the bank built from the input set."""
    if rows is None:
        return call(torch, h, inp, dt, ring=ring, **kw)
    robots = []
    for b, m in enumerate(rows):
        r = make_robot(m, h.N)
        r.F_tip, r.M_tip = inp["wrench"][b, :3].copy(), inp["wrench"][b, 3:].copy()
        robots.append(r)
    with h.param_table([r._params() for r in robots]) as tab:
        if bank_nets is None:
            return call(torch, h, inp, dt, ring=ring, table=tab, loads=loads, **kw)
        with h.mlp_bank([(m.weights, m.biases, m.acts) for m in bank_nets]) as bank:
            return call(torch, h, inp, dt, ring=ring, table=tab, bank=bank, net_of_rod=list(sc.BANK_NETS), **kw)


def ran_persistent(h, W, overlap):
    def f():
        got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
        assert got == (2, W, overlap), f"(path, waves per rod, overlap) = {got}, expected (2, {W}, {overlap})"
    return f


def golden_mlp():
    import cosserat_oracle as orc
    return orc.mlp_from_arrays(load_golden("bc"), "mlp_elu6464")  # (the network of tests/test_gpu_bc.py)


# ---------------------------------------------------------------------------
# K2a: eight rods share a wavefront
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["euler", "rk4"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_k2a_single_shooting(torch_cuda, monkeypatch, dtype, scheme):
    import krod_native as kn
    set_mode_env(monkeypatch, "single")
    h = make_robot(None, sc.SHAPES["k2a"][0])._native()
    triples(torch_cuda, h, f"K2a {scheme}", "k2a", dtype, lambda: assert_path(h, 0), kinds=("nan_ctl", "overflow_ctl"),
            scheme=kn.KR_RK4 if scheme == "rk4" else kn.KR_EULER)


# ---------------------------------------------------------------------------
# one wavefront per rod: K2b, K2c, K2e + take-over launch, their table / loads / MLP / bank twins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_k2b_one_launch_per_step(torch_cuda, monkeypatch, dtype):
    set_mode_env(monkeypatch, "multi")
    h = make_robot(None, sc.SHAPES["one_wave"][0])._native()
    triples(torch_cuda, h, "K2b", "one_wave", dtype, lambda: assert_path(h, 1, 1), kinds=("nan_ctl", "overflow_ctl"))


@pytest.mark.parametrize("mode", ["persistent", "overlap"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_k2c_k2e_persistent(torch_cuda, monkeypatch, dtype, mode):
    """K2c alone, and K2e with K2c launched behind it for the rod it gives up: full trajectory and ring; t0 = 0 (the rod is
    given up at step 0) and t0 = T - 1 (on a ring the healthy rods' last three states must be complete)."""
    set_mode_env(monkeypatch, mode)
    N, B, T, _ = sc.SHAPES["one_wave"]
    h = make_robot(None, N)._native()
    triples(torch_cuda, h, "K2e" if mode == "overlap" else "K2c", "one_wave", dtype,
            ran_persistent(h, 1, 1 if mode == "overlap" else 0), kinds=("nan_ctl", "overflow_ctl"), t0s=(sc.T0, 0, T - 1),
            rings=(False, True))


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_table_twin(torch_cuda, monkeypatch, dtype, overlap):
    set_mode_env(monkeypatch, "overlap")
    h = make_robot(None, sc.SHAPES["one_wave"][0])._native()
    h.set_option("overlap", overlap)
    triples(torch_cuda, h, f"table overlap={overlap}", "one_wave", dtype, ran_persistent(h, 1, overlap),
            kinds=("nan_ctl", "nan_row"), rings=(False, True), rows=sc.MODS5)


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_loads_twin(torch_cuda, monkeypatch, dtype, overlap):
    set_mode_env(monkeypatch, "overlap")
    h = make_robot(None, sc.SHAPES["one_wave"][0])._native()
    h.set_option("overlap", overlap)
    triples(torch_cuda, h, f"loads overlap={overlap}", "one_wave", dtype, ran_persistent(h, 1, overlap),
            kinds=("nan_load",), rings=(False, True), rows=sc.MODS5, loads=True)


@pytest.mark.parametrize("mode", ["persistent", "multi"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mlp_on_one_wavefront(torch_cuda, monkeypatch, dtype, mode):
    """K2c and K2b (kr_msn_*) with the network inside the sweeps: the NaN goes through bf16 packing and the MFMA evaluators
    into LDS tiles the next evaluation reuses."""
    set_mode_env(monkeypatch, mode)
    carrier = make_robot(None, sc.SHAPES["one_wave"][0])
    inject(carrier, golden_mlp())
    h = carrier._native()
    ran = ran_persistent(h, 1, 0) if mode == "persistent" else (lambda: assert_path(h, 1, 1))
    triples(torch_cuda, h, f"MLP on, {mode}", "one_wave", dtype, ran, use_nn=True)


def test_network_bank(torch_cuda, monkeypatch):
    import mlp_bank_cases as mb
    set_mode_env(monkeypatch, "overlap")
    h = make_robot(None, sc.SHAPES["one_wave"][0])._native()
    triples(torch_cuda, h, "bank", "one_wave", "f64", ran_persistent(h, 1, 0), rows=(None,) * 5, bank_nets=mb.bank_three()[:2])


# ---------------------------------------------------------------------------
# several wavefronts per rod: K2d, K2f, mswn
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [0, 1])
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_k2d_several_wavefronts(torch_cuda, monkeypatch, dtype, W, persistent):
    set_mode_env(monkeypatch, "persistent" if persistent else "multi", waves_per_rod=W)
    h = make_robot(None, sc.SHAPES["waves"][0])._native()
    h.set_option("msw_overlap", 0)
    ran = ran_persistent(h, W, 0) if persistent else (lambda: assert_path(h, 1, W))
    triples(torch_cuda, h, f"K2d W={W} persistent={persistent}", "waves", dtype, ran, kinds=("nan_ctl", "overflow_ctl"))


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_k2f_overlapped_several_wavefronts(torch_cuda, monkeypatch, dtype, W):
    set_mode_env(monkeypatch, "persistent", waves_per_rod=W)
    N, B, T, _ = sc.SHAPES["waves"]
    h = make_robot(None, N)._native()
    triples(torch_cuda, h, f"K2f W={W}", "waves", dtype, ran_persistent(h, W, 1), kinds=("nan_ctl", "overflow_ctl"),
            t0s=(sc.T0, 0, T - 1), rings=(False, True))


def test_k2f_tiles_read_from_the_states(torch_cuda, monkeypatch):
    """N = 400, B = 2: the plan picks four wavefronts per rod with overlapped steps by itself, and the tiles of leading slots
    do not fit the LDS (the GT instantiation: tests/test_select_cpu.py pins that choice) - the three slots of the ring ARE
    the tiles, so a NaN record of the sick rod must stay inside that rod's records."""
    set_mode_env(monkeypatch, "persistent", waves_per_rod=0)
    h = make_robot(None, sc.SHAPES["long"][0])._native()
    N, B, T, _ = sc.SHAPES["long"]
    full = call(torch_cuda, h, sc.clean_set("long"), tdtype(torch_cuda, "f64"))  # the clean trajectory the rings are held against
    ran_persistent(h, 4, 1)()
    assert np.all(full["status"] == 0) and full["guards"]
    triples(torch_cuda, h, "K2f GT", "long", "f64", ran_persistent(h, 4, 1), t0s=(sc.T0, 0, T - 1), rings=(True,), full_clean=full)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mlp_on_two_wavefronts(torch_cuda, monkeypatch, dtype):
    set_mode_env(monkeypatch, "persistent", waves_per_rod=2)
    carrier = make_robot(None, sc.SHAPES["waves"][0])
    inject(carrier, golden_mlp())
    h = carrier._native()
    triples(torch_cuda, h, "MLP on, W=2", "waves", dtype, ran_persistent(h, 2, 0), use_nn=True)


# ---------------------------------------------------------------------------
# the kernel family does not change the sick rod's status
# ---------------------------------------------------------------------------
def test_sick_status_does_not_depend_on_the_kernel(torch_cuda, monkeypatch):
    """Precedent: tests/test_gpu_msw.py::test_hard_step_status_does_not_depend_on_the_kernel.  The same batch (N = 27,
    B = 3, rod 1 sick at t0) through every family that serves it: one status table."""
    torch = torch_cuda
    N, B, T, (s,) = sc.SHAPES["waves"]
    tw = sc.sick_twin(sc.clean_set("waves"), "nan_ctl", s)
    want = np.zeros((B, T), dtype=np.int32)
    want[s, sc.T0:] = 2
    for mode, W, mswo in (("single", 1, 1), ("multi", 1, 1), ("persistent", 1, 1), ("overlap", 1, 1), ("multi", 2, 1),
                          ("multi", 4, 1), ("persistent", 2, 0), ("persistent", 4, 0), ("persistent", 2, 1), ("persistent", 4, 1)):
        set_mode_env(monkeypatch, mode, waves_per_rod=W)
        h = make_robot(None, N)._native()
        h.set_option("msw_overlap", mswo)
        for dt_name in ("f64", "f32"):
            out = call(torch, h, tw, tdtype(torch, dt_name))
            assert h.get_option("last_waves_per_rod") == W
            assert h.get_option("last_sim_path") == {"single": 0, "multi": 1}.get(mode, 2)
            assert np.array_equal(out["status"], want), (mode, W, mswo, dt_name, out["status"].tolist())


# ---------------------------------------------------------------------------
# a run advanced by several calls with a kept predictor
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,mode,W", [("one_wave", "persistent", 1), ("one_wave", "overlap", 1), ("waves", "persistent", 2)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chunked_call_with_kept_predictor(torch_cuda, monkeypatch, dtype, family, mode, W):
    """K2c, K2e and K2f (W = 2) with ``keep_predictor = 1``, chunks [3, 1, 3]: the sick step is the one-step chunk, so the rod
    fails at step 0 of a call that loaded the predictor image of the call before - and the image the failing call leaves
    is what the last chunk loads."""
    torch = torch_cuda
    set_mode_env(monkeypatch, mode, waves_per_rod=W)
    N, B, T, sick_rods = sc.SHAPES[family]
    h = make_robot(None, N)._native()
    dt = tdtype(torch, dtype)
    c = sc.clean_set(family)
    ran = ran_persistent(h, W, 1 if (mode == "overlap" or W > 1) else 0)

    def chunked(inp, poison=False):
        h.set_option("keep_predictor", 0)  # (drops the stored image)
        h.set_option("keep_predictor", 1)
        try:
            out = call(torch, h, inp, dt, chunks=[3, 1, 3], poison=poison)
        finally:
            h.set_option("keep_predictor", 0)
        ran()
        return out

    for s in sick_rods:
        tw = sc.sick_twin(c, "nan_ctl", s)
        clean, sick, again = chunked(c), chunked(tw), chunked(c, poison=True)
        label = f"chunked {family} {mode} W={W} {dtype} s={s}"
        healthy = np.arange(B) != s
        assert clean["guards"] and sick["guards"] and again["guards"]
        assert np.all(clean["status"] == 0), clean["status"].tolist()
        same(sick, clean, healthy, f"{label}: healthy rods")
        got = sick["status"][s]
        print(f"{label}: sick rod status {got.tolist()}")
        assert np.all(got[:sc.T0] == 0) and got[sc.T0] == 2 and np.all((got[sc.T0:] == 1) | (got[sc.T0:] == 2)), got.tolist()
        assert np.array_equal(sick["states"][:sc.T0 + 1, s], clean["states"][:sc.T0 + 1, s])
        same(again, clean, np.arange(B), f"{label}: third run against the first")


# ---------------------------------------------------------------------------
# kr_step_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,mode,W", [("k2a", "single", 1), ("one_wave", "multi", 1), ("waves", "multi", 2)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_step_batch(torch_cuda, monkeypatch, dtype, family, mode, W):
    """One step from the reference's warm start (predictor 0: the caller's G) with one NaN tension: status 2 for that rod,
    1 <= iters <= maxit + 8 maxit (the header's two caps), the other rods as in the clean call bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, mode, waves_per_rod=W)
    N, B, T, sick_rods = sc.SHAPES[family]
    h = make_robot(None, N)._native()
    dt = tdtype(torch, dtype)
    c = sc.clean_set(family)
    t0 = sc.T0
    warm = call(torch, h, dict(c, ctl=c["ctl"][:, :t0]), dt)  # states 0 .. t0 and the G of step t0 - 1
    assert np.all(warm["status"] == 0)
    path = {"single": 0, "multi": 1}[mode]

    def step(tens, maxit, poison=False):
        prev, cur = dev(torch, warm["states"][t0 - 1], dt), dev(torch, warm["states"][t0], dt)
        nxt = Guarded(torch, (B, N, 28), dt, FSENT, fill=float("nan") if poison else 0.0)
        G = Guarded(torch, (B, 6), dt, FSENT)
        G.t.copy_(dev(torch, warm["G"], dt))
        status = Guarded(torch, (B,), torch.int32, ISENT)
        iters = Guarded(torch, (B,), torch.int32, ISENT)
        h.step(prev, cur, nxt.t, G.t, dev(torch, tens, dt), maxit=maxit, status=status.t, iters=iters.t, predictor=0)
        torch.cuda.synchronize()
        assert_path(h, path, W)
        assert nxt.intact() and G.intact() and status.intact() and iters.intact()
        return dict(status=status.t.cpu().numpy(), iters=iters.t.cpu().numpy(), G=G.t.cpu().numpy(), nxt=nxt.t.cpu().numpy())

    for maxit in (2, 30):
        clean = step(c["ctl"][:, t0], maxit)
        assert np.all((clean["status"] >= 0) & (clean["status"] <= 2)) and np.all(clean["iters"] >= 1)
        assert np.all(clean["iters"] <= 9 * maxit), clean["iters"].tolist()
        if maxit == 30:
            assert np.all(clean["status"] == 0), clean["status"].tolist()
        for s in sick_rods:
            sick = step(sc.sick_twin(c, "nan_ctl", s)["ctl"][:, t0], maxit)
            healthy = np.arange(B) != s
            print(f"step {family} {mode} W={W} {dtype} maxit={maxit} s={s}: status {sick['status'].tolist()} iters {sick['iters'].tolist()}")
            assert sick["status"][s] == 2 and 1 <= sick["iters"][s] <= 9 * maxit, (sick["status"].tolist(), sick["iters"].tolist())
            for k in ("status", "iters", "G", "nxt"):
                assert np.array_equal(sick[k][healthy], clean[k][healthy]), (k, maxit, s)
            assert np.all(sick["nxt"][healthy][..., 25:] == 0)
        again = step(c["ctl"][:, t0], maxit, poison=True)
        for k in ("status", "iters", "G", "nxt"):
            assert np.array_equal(again[k], clean[k]), (k, maxit)


# ---------------------------------------------------------------------------
# Python front end
# ---------------------------------------------------------------------------
def test_simulate_batch_front_end(torch_cuda, monkeypatch):
    """``simulate_batch(..., robots=, tip_loads=, score=)`` with one NaN load - and with one NaN tension - returns normally; the
    healthy rods' scores are those of the clean call bit for bit; the sick rod's ``dtw`` and ``mse`` are finite for the NaN
    load and NaN for the NaN tension (module docstring)."""
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    N, B, T, sick_rods = sc.SHAPES["one_wave"]
    c = sc.clean_set("one_wave")
    carrier = make_robot(None, N)

    def robots(inp):
        out = []
        for b, m in enumerate(sc.MODS5):
            r = make_robot(m, N)
            r.F_tip, r.M_tip = inp["wrench"][b, :3].copy(), inp["wrench"][b, 3:].copy()
            out.append(r)
        return out

    plain = simulate_batch(carrier, c["ctl"], robots=robots(c), tip_loads=c["loads"])
    ref = plain["traj"][0, :T]
    clean = simulate_batch(carrier, c["ctl"], robots=robots(c), tip_loads=c["loads"], score={"reference": ref})
    ran_persistent(carrier._handle, 1, 1)()
    assert np.all(clean["status"] == 0) and np.all(np.isfinite(clean["dtw"])) and np.all(np.isfinite(clean["mse"]))
    assert clean["dtw"][0] == 0.0 and np.all(clean["dtw"][1:] > 0)
    for kind, s in [(kind, s) for kind in ("nan_load", "nan_ctl") for s in sick_rods]:
        tw = sc.sick_twin(c, kind, s)
        sick = simulate_batch(carrier, tw["ctl"], robots=robots(tw), tip_loads=tw["loads"], score={"reference": ref},
                              check_finite=False)
        ran_persistent(carrier._handle, 1, 1)()
        healthy = np.arange(B) != s
        print(f"front end {kind} s={s}: status {sick['status'][s].tolist()} dtw {sick['dtw'].tolist()} mse {sick['mse'].tolist()}")
        for k in ("dtw", "mse", "status", "tip", "G", "traj"):
            assert np.array_equal(sick[k][healthy], clean[k][healthy]), (kind, k)
        assert np.all(sick["status"][s, :sc.T0] == 0) and sick["status"][s, sc.T0] == 2
        if kind == "nan_load":
            assert np.isfinite(sick["dtw"][s]) and np.isfinite(sick["mse"][s]) and np.all(np.isfinite(sick["traj"][s]))
        else:
            assert np.all(sick["status"][s, sc.T0:] != 0)
            assert np.isnan(sick["dtw"][s]) and np.isnan(sick["mse"][s])
    again = simulate_batch(carrier, c["ctl"], robots=robots(c), tip_loads=c["loads"], score={"reference": ref})
    for k in ("dtw", "mse", "status", "tip", "G", "traj"):
        assert np.array_equal(again[k], clean[k]), k
