"""Per-step boundary data (kr_simulate_batch_boundary) on the MI355X: a moving base per rod in one simulate call.

Rod b solves step t with ``bnd[b, t]`` = p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3) in place of those values of
its table row.  The reference side of a comparison is the fixture tests/golden/base_motion.npz (the unmodified reference
with ``robot.p0 / h0 / q0 / w0`` assigned while ``knode.simulate`` draws control t; its last solve is dropped, so T
controls give states 0 .. T-1), the oracle's own time loop with the same assignment (tests/base_motion_cases.py), or the
table / loads call on inputs where both must do the same arithmetic.  Tolerances are those of tests/test_gpu_tip_loads.py:
fp64 ``rel_l2 < 1e-8`` against reference-held trajectories, fp32 tips ``< 1e-5``; a base taken one step late moves the tips
of every history but ``still`` by 1.7e-2 and more (tests/test_base_motion_cpu.py).

Shapes: B = 6 (two workgroups of four rods, the second partial), N in {10, 23} (ragged interval lengths), T in {12, 13}
(both step parities at the end of a call - the overlapped kernel keeps step t's boundary in set t & 1).  Every test
asserts what ran: one persistent launch, one wavefront per rod, the overlapped kernel or not as asked."""
import numpy as np
import pytest

from base_motion_cases import CASES, SHAPES, UNMOVED, base_history, oracle_loop
from conftest import load_golden, rel_l2
from gpu_helpers import inject, make_robot, set_mode_env
from tip_loads_cases import load_history

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODS6 = [None, "damping", "short", "youngs", "noair", "nsw"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check(label, value, bound):
    print(f"{label}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, f"{label}: {value:.3e} >= {bound:.0e}"


def assert_ran(h, overlap):
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
    assert got == (2, 1, overlap), f"(path, waves per rod, overlap) = {got}, expected (2, 1, {overlap})"


def dev(torch, x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype).contiguous()


def run(torch, h, ctl, dtype, table, bnd=None, loads=None, ring=False, chunks=None, maxit=0, use_nn=False):
    """One call (or one per chunk, the state before handed over) from the straight rod; everything as float64 NumPy."""
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dtype, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dtype, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dtype, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    if chunks is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, bnd=bnd, loads=loads, maxit=maxit, use_nn=use_nn)
    else:
        assert not ring
        t0 = 0
        for n in chunks:
            tp = torch.empty((B, n, 3), dtype=dtype, device=DEV)
            sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + n].contiguous(), st[t0:], G, tip=tp, status=sx, prev_init=st[t0 - 1] if t0 else None,
                       table=table, bnd=bnd[:, t0:t0 + n].contiguous(), maxit=maxit)
            tip[:, t0:t0 + n] = tp
            status[:, t0:t0 + n] = sx
            t0 += n
    torch.cuda.synchronize()
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def unpack(st):
    """packed records [.., N, 28] (q w v u p h n m) -> reference rows [.., 25, N] (p h n m q w v u)"""
    st = np.swapaxes(st, -1, -2)
    return np.concatenate([st[..., 12:25, :], st[..., 0:12, :]], axis=-2)


def base_of_record0(st):
    """p0 h0 q0 w0 as record 0 of packed states [.., N, 28] holds them"""
    r = st[..., 0, :]
    return np.concatenate([r[..., 12:19], r[..., 0:6]], axis=-1)


def sine_ctl(B, T, del_t, seed):
    import cosserat_oracle as orc
    return orc.batch_sine_controls(B, T, del_t, seed)


def boundary_rows(N):
    """six presets, each with a tilted (non-unit) base, a base velocity and a tip wrench of its own"""
    rng = np.random.default_rng(15 + N)
    robots = []
    for m in MODS6:
        r = make_robot(m, N)
        r.p0 = rng.normal(0, 0.02, 3)
        r.h0 = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.08, 4)
        r.q0, r.w0 = rng.normal(0, 0.02, 3), rng.normal(0, 0.05, 3)
        r.F_tip, r.M_tip = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3)
        robots.append(r)
    return robots


def row_boundary(r):
    return np.concatenate([r.p0, r.h0, r.q0, r.w0, r.F_tip, r.M_tip]).astype(np.float64)


def scaled(hist, f):
    """a base history with its departure from the unmoved base scaled by f"""
    return UNMOVED + (hist - UNMOVED) * f


# ---------------------------------------------------------------------------
# 1. a constant boundary equal to the rows' own values is the table call, bit for bit
# ---------------------------------------------------------------------------
def _constant_boundary_case(torch, h, robots, dtype, overlap, T, use_nn, seed):
    B = len(robots)
    ctl = dev(torch, sine_ctl(B, T, robots[0].del_t, seed), dtype)
    bnd = np.stack([np.tile(row_boundary(r), (T, 1)) for r in robots])
    with h.param_table([r._params() for r in robots]) as tab:
        for ring in (False, True):
            a = run(torch, h, ctl, dtype, tab, ring=ring, use_nn=use_nn)
            assert_ran(h, overlap)
            b = run(torch, h, ctl, dtype, tab, bnd=dev(torch, bnd, dtype), ring=ring, use_nn=use_nn)
            assert_ran(h, overlap)
            print(f"N={robots[0].N} ring={ring} use_nn={use_nn}: {int((a['status'] != 0).sum())} steps not converged")
            if not use_nn:
                assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            for k in ("status", "tip", "G", "states"):
                assert np.array_equal(a[k], b[k]), f"ring={ring}: {k} differs from the table call"
    # the rows do differ (the comparison is not between six copies of one rod), and their bases are in the states
    assert rel_l2(a["tip"][1], a["tip"][0]) > 1e-3
    want = bnd[:, 0, :13] if dtype == torch.float64 else bnd[:, 0, :13].astype(np.float32).astype(np.float64)
    assert np.array_equal(base_of_record0(a["states"][T % 3]), want)


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constant_boundary_is_the_table_call(torch_cuda, monkeypatch, dtype, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    for N, T in SHAPES:
        h = make_robot(None, N)._native()
        h.set_option("overlap", overlap)
        _constant_boundary_case(torch, h, boundary_rows(N), dt, overlap, T, False, 60 + N)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constant_boundary_is_the_table_call_mlp_on(torch_cuda, monkeypatch, dtype):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    mlp = orc.mlp_from_arrays(load_golden("bc"), "mlp_elu64")  # (the network of test_gpu_param_table's MLP-on calls)
    for N, T in SHAPES:
        carrier = make_robot(None, N)
        inject(carrier, mlp)
        _constant_boundary_case(torch, carrier._native(), boundary_rows(N), dt, 0, T, True, 70 + N)


# ---------------------------------------------------------------------------
# 2. the rows' own base with a varying wrench is the loads call, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_own_base_with_a_varying_wrench_is_the_loads_call(torch_cuda, monkeypatch, dtype, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    cases = ["const", "jump", "alt", "sine", "alt", "sine"]
    for N, T in SHAPES:
        robots = boundary_rows(N)
        B = len(robots)
        h = make_robot(None, N)._native()
        h.set_option("overlap", overlap)
        ctl = dev(torch, sine_ctl(B, T, robots[0].del_t, 80 + N), dt)
        L = np.stack([load_history(c, T) * (1 + 0.1 * b) for b, c in enumerate(cases)])
        bnd = np.concatenate([np.stack([np.tile(row_boundary(r)[:13], (T, 1)) for r in robots]), L], axis=2)
        with h.param_table([r._params() for r in robots]) as tab:
            for ring in (False, True):
                a = run(torch, h, ctl, dt, tab, loads=dev(torch, L, dt), ring=ring)
                assert_ran(h, overlap)
                b = run(torch, h, ctl, dt, tab, bnd=dev(torch, bnd, dt), ring=ring)
                assert_ran(h, overlap)
                assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
                for k in ("status", "tip", "G", "states"):
                    assert np.array_equal(a[k], b[k]), f"N={N} ring={ring}: {k} differs from the loads call"


# ---------------------------------------------------------------------------
# 3. against the reference fixture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("N,T", SHAPES)
def test_against_the_reference_fixture(torch_cuda, monkeypatch, N, T, overlap):
    """The five histories in one batch (rod b gets case b), padded with an unmoved rod that must be the table call."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("base_motion")
    k = f"_n{N}"
    assert np.all(g["ier" + k] == 1)
    r = make_robot(None, N)
    h = r._native()
    h.set_option("overlap", overlap)
    B = 6
    bnd = np.zeros((B, T, 19))
    bnd[:5, :, :13] = g["base" + k]
    bnd[5, :, :13] = UNMOVED
    bnd[:, :, 13:] = row_boundary(r)[13:]
    assert np.array_equal(row_boundary(r)[:13], UNMOVED)
    ctl = np.stack([g["ctl" + k]] * B)
    with h.param_table([r._params()] * B) as tab:
        for dtype in (torch.float64, torch.float32):
            a = run(torch, h, dev(torch, ctl, dtype), dtype, tab, bnd=dev(torch, bnd, dtype))
            assert_ran(h, overlap)
            assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            plain = run(torch, h, dev(torch, ctl, dtype), dtype, tab)
            assert_ran(h, overlap)
            for key in ("tip", "status", "G"):
                assert np.array_equal(a[key][5], plain[key][5]), f"unmoved rod: {key} differs from the table call"
            assert np.array_equal(a["states"][:, 5], plain["states"][:, 5])
            # record 0 of state t + 1 holds the base of step t, exactly (in the precision of the call)
            given = bnd[:, :, :13] if dtype == torch.float64 else bnd[:, :, :13].astype(np.float32).astype(np.float64)
            assert np.array_equal(base_of_record0(a["states"][1:]).transpose(1, 0, 2), given)
            # tip after step t = tip of state t + 1; the fixture holds states 0 .. T-1
            for c, case in enumerate(CASES):
                tips = unpack(a["states"][:T, c])[:, :3, -1]
                if dtype == torch.float64:
                    check(f"N={N} overlap={overlap} {case} tips", rel_l2(tips, g["tips" + k][c]), 1e-8)
                    check(f"N={N} overlap={overlap} {case} tip output", rel_l2(a["tip"][c, :T - 1], g["tips" + k][c][1:]), 1e-8)
                    check(f"N={N} overlap={overlap} {case} state T-1", rel_l2(unpack(a["states"][T - 1, c]), g["last" + k][c]), 1e-8)
                    if N == 10:
                        check(f"N={N} overlap={overlap} {case} trajectory", rel_l2(unpack(a["states"][:T, c]), g["traj" + k][c]), 1e-8)
                else:
                    check(f"N={N} overlap={overlap} {case} fp32 tips", rel_l2(tips, g["tips" + k][c]), 1e-5)


# ---------------------------------------------------------------------------
# 4. against the oracle loop: per-rod constants, base motion and tip loads together, through simulate_batch
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_oracle():
    import cosserat_oracle as orc
    N, T = 23, 13
    mods = [None, "damping", None, "damping", "damping", None]
    bases = ["slide", "tilt", "alt", "jump", "alt", "still"]
    loads = ["const", "jump", "alt", "sine", "alt", "sine"]
    ctl = orc.batch_sine_controls(6, T, 0.05, 313)
    M = np.stack([base_history(c, T) for c in bases])
    L = np.stack([load_history(c, T) for c in loads])
    refs = []
    for b in range(6):
        states, ok, _ = oracle_loop(orc.params_for(mods[b], N), ctl[b], M[b], L[b])
        assert ok.all(), b
        refs.append(states)
    return N, T, mods, ctl, M, L, refs


def test_against_the_oracle_with_per_rod_constants_and_tip_loads(torch_cuda, monkeypatch, mixed_oracle):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    N, T, mods, ctl, M, L, refs = mixed_oracle
    carrier = make_robot(None, N)
    robots = [make_robot(m, N) for m in mods]
    out = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_loads=L)
    h = carrier._handle
    assert_ran(h, 1)
    assert np.all(out["status"] == 0), np.argwhere(out["status"] != 0)[:8]
    for b in range(6):
        check(f"rod {b} ({mods[b]}) tips", rel_l2(out["tip"][b], refs[b][1:, :3, -1]), 1e-8)
        check(f"rod {b} ({mods[b]}) state T", rel_l2(out["traj"][b, T], refs[b][T]), 1e-8)
    assert rel_l2(out["tip"][4], out["tip"][2]) > 1e-3  # same histories, another rod
    # without tip_loads every rod keeps its own wrench: the same call with the rows' wrench written out
    for b, r in enumerate(robots):
        r.F_tip, r.M_tip = np.array([0.02 * (b + 1), -0.01, 0.03]), np.array([1e-3, -5e-4 * b, 2e-4])
    own = simulate_batch(carrier, ctl, robots=robots, base_motion=M)
    assert_ran(h, 1)
    rows = np.stack([np.tile(np.concatenate([r.F_tip, r.M_tip]), (T, 1)) for r in robots])
    both = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_loads=rows)
    assert np.all(own["status"] == 0)
    for key in ("tip", "G", "traj", "status"):
        assert np.array_equal(own[key], both[key]), key
    assert rel_l2(own["tip"], out["tip"]) > 1e-3
    # [T, 13] is shared by all rods; tip_only keeps the tips; tip_loads alone is still the loads call
    shared = simulate_batch(carrier, ctl, base_motion=M[0])
    full = simulate_batch(carrier, ctl, base_motion=np.stack([M[0]] * 6))
    assert np.array_equal(shared["tip"], full["tip"]) and np.array_equal(shared["traj"], full["traj"])
    lean = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_only=True)
    assert np.array_equal(lean["tip"], own["tip"]) and "traj" not in lean


# ---------------------------------------------------------------------------
# 5. hand-over to the take-over launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("history", ["alt", "jump"])
def test_hand_over_to_second_launch(torch_cuda, monkeypatch, history):
    """An iteration cap of 2 from the straight rod (tests/test_gpu_tip_loads.py::test_hand_over_to_second_launch): the
    overlapped kernel gives rods up and the plain persistent kernel takes over at their resume step, where it must load
    that step's boundary.  ``alt`` scaled per rod, and ``jump`` the same way.  (Measured: under this cap every step of both
    batches still ends converged, and a take-over launch that loads step 0's values at every resume step passes both - the
    rods given up here are given up at step 0.  A resume step in mid-call is what
    test_nan_base_value_fails_one_rod_from_that_step[1] goes through, and that mutation fails it.)"""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 6
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 77), dt)
    bnd = np.zeros((B, T, 19))
    bnd[:, :, :13] = np.stack([scaled(base_history(history, T), 1 + 0.25 * b) for b in range(B)])
    bnd = dev(torch, bnd, dt)
    with h.param_table([r._params()] * B) as tab:
        h.set_option("overlap", 1)
        a = run(torch, h, ctl, dt, tab, bnd=bnd, maxit=2)
        assert_ran(h, 1)
        ar = run(torch, h, ctl, dt, tab, bnd=bnd, maxit=2, ring=True)
        assert_ran(h, 1)
        h.set_option("overlap", 0)
        b = run(torch, h, ctl, dt, tab, bnd=bnd, maxit=2)
        assert_ran(h, 0)
        h.set_option("overlap", 1)
        c = run(torch, h, ctl, dt, tab, bnd=bnd)
    print(f"{history}: steps not converged at the cap: {int((a['status'] != 0).sum())} of {B * T}")
    assert np.all(a["status"] >= 0) and np.all(a["status"] <= 2)
    assert np.array_equal(a["status"] != 0, b["status"] != 0)
    assert np.all(np.isfinite(a["tip"]))
    check("overlapped + take-over against the plain kernel, tips", rel_l2(a["tip"], b["tip"]), 1e-6)
    assert np.array_equal(base_of_record0(a["states"][1:]).transpose(1, 0, 2), bnd.cpu().numpy()[:, :, :13])
    assert np.array_equal(ar["status"], a["status"])
    check("ring against full history, tips", rel_l2(ar["tip"], a["tip"]), 1e-9)
    assert np.all(c["status"] == 0)  # with the default cap everything converges again on the same handle


# ---------------------------------------------------------------------------
# 6. calls in pieces
# ---------------------------------------------------------------------------
def test_calls_in_pieces(torch_cuda, monkeypatch):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 6
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 21), dt)
    bnd = np.zeros((B, T, 19))
    bnd[:, :, :13] = np.stack([base_history(c, T) for c in ("still", "slide", "tilt", "jump", "alt", "slide")])
    bnd[:, :, 13:] = np.stack([load_history(c, T) for c in ("const", "jump", "alt", "sine", "alt", "const")])
    bnd = dev(torch, bnd, dt)
    with h.param_table([r._params()] * B) as tab:
        one = run(torch, h, ctl, dt, tab, bnd=bnd)
        assert_ran(h, 1)
        assert np.all(one["status"] == 0)
        for keep in (0, 1):
            h.set_option("keep_predictor", 0)
            h.set_option("keep_predictor", keep)
            try:
                ch = run(torch, h, ctl, dt, tab, bnd=bnd, chunks=[5, 1, 7])
            finally:
                h.set_option("keep_predictor", 0)
            assert_ran(h, 1)
            assert np.all(ch["status"] == 0)
            check(f"keep_predictor={keep} chunks, last state", rel_l2(ch["states"][T][..., :25], one["states"][T][..., :25]), 1e-7)
            check(f"keep_predictor={keep} chunks, tips", rel_l2(ch["tip"], one["tip"]), 1e-7)
            assert np.array_equal(base_of_record0(ch["states"][1:]), base_of_record0(one["states"][1:]))
        ring = run(torch, h, ctl, dt, tab, bnd=bnd, ring=True)
        assert_ran(h, 1)
    assert np.array_equal(ring["tip"], one["tip"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(ring["states"][k % 3], one["states"][k]), k


# ---------------------------------------------------------------------------
# 7. a base value that is not finite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
def test_nan_base_value_fails_one_rod_from_that_step(torch_cuda, monkeypatch, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 6
    r = make_robot(None, N)
    h = r._native()
    h.set_option("overlap", overlap)
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 33), dt)
    clean = np.zeros((B, T, 19))
    clean[:, :, :13] = np.stack([base_history(c, T) for c in ("slide", "tilt", "alt", "jump", "still", "slide")])
    bad = clean.copy()
    bad[1, 5, 0] = np.nan  # p0.x of rod 1 at step 5
    with h.param_table([r._params()] * B) as tab:
        want = run(torch, h, ctl, dt, tab, bnd=dev(torch, clean, dt))
        assert_ran(h, overlap)
        assert np.all(want["status"] == 0)
        got = run(torch, h, ctl, dt, tab, bnd=dev(torch, bad, dt))
        assert_ran(h, overlap)
        again = run(torch, h, ctl, dt, tab, bnd=dev(torch, clean, dt))
        assert_ran(h, overlap)
    print(f"overlap={overlap}: status of rod 1: {got['status'][1].tolist()}")
    assert np.all(got["status"][1, :5] == 0) and got["status"][1, 5] == 2 and np.all(got["status"][1, 6:] != 0)
    # before the bad step the rod is the clean run's, bit for bit
    assert np.array_equal(got["tip"][1, :5], want["tip"][1, :5]) and np.array_equal(got["states"][:6, 1], want["states"][:6, 1])
    others = [0, 2, 3, 4, 5]
    for k in ("status", "tip", "G"):
        assert np.array_equal(got[k][others], want[k][others]), f"{k} of another rod differs from the clean call"
    assert np.array_equal(got["states"][:, others], want["states"][:, others])
    for k in ("status", "tip", "G", "states"):  # nothing of the failure stays behind in the handle
        assert np.array_equal(again[k], want[k]), f"{k} of the next call differs from the clean call"


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch_cuda, monkeypatch):
    import ctypes as C
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    T, B = 12, 6
    NAME = "kr_simulate_batch_boundary"

    def setup(N):
        r = make_robot(None, N)
        h = r._native()
        ctl = dev(torch, sine_ctl(B, T, r.del_t, 9), dt)
        bnd = np.zeros((B, T, 19))
        bnd[:, :, :13] = base_history("slide", T)
        st = h.new_state(B, dt, n_slots=T + 1)
        return r, h, ctl, dev(torch, bnd, dt), st

    SENT = -7.0
    G = torch.full((B, 6), SENT, dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dt, device=DEV)
    status = torch.full((B, T), -7, dtype=torch.int32, device=DEV)

    def untouched(st):
        torch.cuda.synchronize()
        return bool((st[1:] == 0).all() and (G == SENT).all() and (tip == SENT).all() and (status == -7).all())

    def raw(h, ctl, st, table, bnd, scheme=kn.KR_EULER):
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        return h.lib.kr_simulate_batch_boundary(h._h, table, T, scheme, p(ctl), p(bnd), p(st), 0, p(G), p(tip), 0.0, 0, p(status),
                                                0, None, kn.dtype_code(dt), None)

    def refused(h, rc, *words):
        assert rc == kn.KR_E_UNSUPPORTED, rc
        msg = h.lib.kr_last_error().decode()
        assert NAME in msg and all(w in msg for w in words), msg

    r, h, ctl, bnd, st = setup(23)
    with h.param_table([r._params()] * B) as tab:
        h.init_straight(st[0], table=tab)
        ok = run(torch, h, ctl, dt, tab, bnd=bnd)
        assert_ran(h, 1)
        assert np.all(ok["status"] == 0)
        assert raw(h, ctl, st, tab._t, None) == kn.KR_E_ARG and "bnd" in h.lib.kr_last_error().decode()  # a NULL bnd
        assert raw(h, ctl, st, None, bnd) == kn.KR_E_ARG                                               # a NULL table
        assert untouched(st)
        refused(h, raw(h, ctl, st, tab._t, bnd, kn.KR_RK4), "Euler")
        assert untouched(st)
        h.set_option("waves_per_rod", 2)
        refused(h, raw(h, ctl, st, tab._t, bnd), "waves_per_rod = 2")
        assert untouched(st) and h.get_option("last_waves_per_rod") == 1
        h.set_option("waves_per_rod", 1)
        h.set_option("persistent", 0)
        refused(h, raw(h, ctl, st, tab._t, bnd), "persistent = 0")
        assert untouched(st)
        h.set_option("persistent", 1)
        # the binding: a boundary needs a table, and does not ride with a bank
        with pytest.raises(kn.KrError, match="table"):
            h.simulate(ctl, st, G, bnd=bnd)
        with pytest.raises(kn.KrError, match="bank"):
            h.simulate(ctl, st, G, table=tab, bank=object(), net_of_rod=[0] * B, bnd=bnd)
        assert untouched(st)
        again = run(torch, h, ctl, dt, tab, bnd=bnd)
        assert_ran(h, 1)
        assert np.array_equal(again["tip"], ok["tip"])
    # N = 8: no table can be made for the call to take (the planner's own refusal of N = 8, worded for this call, is held
    # in tests/test_base_motion_cpu.py::test_boundary_query_plans_as_the_loads_query)
    r8, h8, ctl8, bnd8, st8 = setup(8)
    with pytest.raises(kn.KrError, match=r"N = 8.*9 <= N <= 128"):
        h8.param_table([r8._params()] * B)
    assert raw(h8, ctl8, st8, None, bnd8) == kn.KR_E_ARG and untouched(st8)
