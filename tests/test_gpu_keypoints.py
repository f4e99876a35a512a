"""Key-point records (kr_simulate_batch_keypoints) on the MI355X: the states at chosen grid points from a tip-only run.

``kp[t, b, k]`` is the complete 28-slot record of grid point ``idx[k]`` of the state step t writes - what a full-history
call leaves in ``states[t + 1, b, idx[k]]``.  Comparisons within one call, between a ring and a full-history call, against
the parent's boundary call and against the clean call of a failing batch are BITWISE (the key-point store copies a record
the kernel has in registers; nothing is recomputed).  Bounds against the reference fixtures are those of the existing
tests of the same fixtures (tests/test_gpu_base_motion.py, tests/test_gpu_tip_loads.py: fp64 ``rel_l2 < 1e-8`` over the
trajectory, fp32 tips ``< 1e-5``; tests/test_gpu_forward.py::test_simulate_with_mlp: ``< 1e-8``), of
test_hand_over_to_second_launch for ring against full history at an iteration cap (``< 1e-9``) and of
test_calls_in_pieces (``< 1e-7``).

Shapes: B = 6 (two workgroups of four rods, the second partial); N = 10 (every point marked), 23 (ragged intervals,
sixteen points with both ends and their neighbours), 128 (the mask's word boundary: 63, 64, 65) and 100; T from 1 to 13
(lean steps of a ring call exist from ``tB + 4 <= T``; both step parities at the end).  Every test asserts what ran.
Four fp64 rods of 128 grid points do not fit the LDS of a compute unit: the table family refuses N = 128 in fp64 (about
N <= 111 is served), so there the test holds the key-point call to the parent's refusal and N = 101 with {0, 63, 64, 65,
100} carries the word boundary in fp64; fp32 runs N = 128 itself."""
import ctypes as C

import numpy as np
import pytest

from base_motion_cases import CASES as BASE_CASES, UNMOVED, base_history
from conftest import load_golden, rel_l2
from gpu_helpers import inject, make_robot, set_mode_env
from tip_loads_cases import CASES as LOAD_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODS6 = [None, "damping", "short", "youngs", "noair", "nsw"]
SENT = -12345.5
POINTS = {10: list(range(10)),
          23: [0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 15, 17, 19, 20, 21, 22],
          128: [0, 63, 64, 65, 127],
          100: [33, 55, 77, 99],
          101: [0, 63, 64, 65, 100],
          20: [0, 1, 2, 3, 5, 6, 8, 9, 10, 12, 13, 15, 16, 17, 18, 19]}
STEPS = [1, 2, 3, 4, 7, 13]


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


def same_bits(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(torch, h, ctl, dtype, table, bnd, idx=None, ring=False, chunks=None, maxit=0, use_nn=False):
    """One call (or one per chunk, the state before handed over) from the straight rod; arrays in the call's dtype.
    idx = None: the parent's boundary call."""
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dtype, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dtype, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dtype, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    kp = torch.full((T, B, len(idx), 28), SENT, dtype=dtype, device=DEV) if idx is not None else None
    kw = lambda k: dict(key_points=idx, kp=k) if idx is not None else {}
    if chunks is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, bnd=bnd, maxit=maxit, use_nn=use_nn, **kw(kp))
    else:
        assert not ring
        t0 = 0
        for n in chunks:
            tp = torch.empty((B, n, 3), dtype=dtype, device=DEV)
            sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + n].contiguous(), st[t0:], G, tip=tp, status=sx, prev_init=st[t0 - 1] if t0 else None,
                       table=table, bnd=bnd[:, t0:t0 + n].contiguous(), maxit=maxit, **kw(kp[t0:t0 + n]))  # (kp is time-major)
            tip[:, t0:t0 + n] = tp
            status[:, t0:t0 + n] = sx
            t0 += n
    torch.cuda.synchronize()
    out = dict(tip=tip.cpu().numpy(), status=status.cpu().numpy(), G=G.cpu().numpy(), states=st.cpu().numpy())
    if kp is not None:
        out["kp"] = kp.cpu().numpy()
        assert not (out["kp"] == SENT).any(), f"{int((out['kp'] == SENT).sum())} sentinel values left in kp"
    return out


def unpack(st):
    """packed records [.., P, 28] (q w v u p h n m) -> reference rows [.., 25, P] (p h n m q w v u)"""
    st = np.swapaxes(st.astype(np.float64), -1, -2)
    return np.concatenate([st[..., 12:25, :], st[..., 0:12, :]], axis=-2)


def sine_ctl(B, T, del_t, seed):
    import cosserat_oracle as orc
    return orc.batch_sine_controls(B, T, del_t, seed)


def boundary_rows(N):
    """six presets, each with a tilted (non-unit) base, a base velocity and a tip wrench of its own"""
    rng = np.random.default_rng(16 + N)
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


def rows_bnd(robots, T):
    return np.stack([np.tile(row_boundary(r), (T, 1)) for r in robots])


def scaled(hist, f):
    return UNMOVED + (hist - UNMOVED) * f


def kp_is_the_states(out, idx, label):
    """rule 1: kp[t, b, k] == states[t + 1, b, idx[k]], all 28 slots, bit for bit"""
    assert same_bits(out["kp"], out["states"][1:][:, :, idx]), f"{label}: kp differs from the marked records of the states"


# ---------------------------------------------------------------------------
# 1. the same call with the full history
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kp_is_the_marked_records_of_the_full_history(torch_cuda, monkeypatch, dtype, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    import krod_native as kn
    ran = []
    for N in (10, 23, 128, 100, 101):
        idx = POINTS[N]
        robots = boundary_rows(N)
        h = make_robot(None, N)._native()
        h.set_option("overlap", overlap)
        with h.param_table([r._params() for r in robots]) as tab:
            try:  # the parent's boundary call decides whether the shape is served at all
                ctl2 = dev(torch, sine_ctl(6, 2, robots[0].del_t, 1), dt)
                run(torch, h, ctl2, dt, tab, dev(torch, rows_bnd(robots, 2), dt))
            except kn.KrError as e:
                assert "kr_simulate_batch_boundary" in str(e) and "does not fit the LDS" in str(e), str(e)
                with pytest.raises(kn.KrError, match="kr_simulate_batch_keypoints.*does not fit the LDS"):
                    run(torch, h, ctl2, dt, tab, dev(torch, rows_bnd(robots, 2), dt), idx=idx)
                print(f"N={N} {dtype}: refused by the table family's plan (LDS), key-point call refused alike")
                continue
            ran.append(N)
            for T in STEPS:
                ctl = dev(torch, sine_ctl(6, T, robots[0].del_t, 160 + N + T), dt)
                a = run(torch, h, ctl, dt, tab, dev(torch, rows_bnd(robots, T), dt), idx=idx)
                assert_ran(h, overlap)
                print(f"N={N} T={T}: {int((a['status'] != 0).sum())} steps not converged")
                kp_is_the_states(a, idx, f"N={N} T={T}")
                assert np.all(a["kp"][..., 25:] == 0)  # the pad slots
        assert rel_l2(a["kp"][:, 1].astype(np.float64), a["kp"][:, 0].astype(np.float64)) > 1e-3  # the rods do differ
    assert ran == ([10, 23, 128, 100, 101] if dtype == "f32" else [10, 23, 100, 101]), ran


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kp_is_the_marked_records_of_the_full_history_mlp_on(torch_cuda, monkeypatch, dtype):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    N, idx = 20, POINTS[20]
    assert len(idx) == 16
    carrier = make_robot(None, N)
    inject(carrier, orc.mlp_from_arrays(load_golden("sim_nn"), "mlp_elu6464"))
    h = carrier._native()
    robots = boundary_rows(N)
    with h.param_table([r._params() for r in robots]) as tab:
        for T in STEPS:
            ctl = dev(torch, sine_ctl(6, T, robots[0].del_t, 190 + T), dt)
            bnd = dev(torch, rows_bnd(robots, T), dt)
            for ring in (False, True):
                a = run(torch, h, ctl, dt, tab, bnd, idx=idx, ring=ring, use_nn=True)
                assert_ran(h, 0)
                print(f"MLP on, T={T} ring={ring}: {int((a['status'] != 0).sum())} steps not converged")
                if not ring:
                    kp_is_the_states(a, idx, f"MLP on, T={T}")
                    full = a
                else:  # the ring call runs the same stores
                    assert same_bits(a["status"], full["status"]) and same_bits(a["tip"], full["tip"])
                    assert same_bits(a["kp"], full["kp"]), f"MLP on, T={T}: kp of the ring call differs from the full call's"


# ---------------------------------------------------------------------------
# 2. ring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ring_call_gives_the_same_kp(torch_cuda, monkeypatch, dtype, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    for N in (23, 100):
        idx = POINTS[N]
        assert idx[-1] == N - 1
        robots = boundary_rows(N)
        h = make_robot(None, N)._native()
        h.set_option("overlap", overlap)
        with h.param_table([r._params() for r in robots]) as tab:
            for T in (3, 4, 7, 13):
                ctl = dev(torch, sine_ctl(6, T, robots[0].del_t, 260 + N + T), dt)
                bnd = dev(torch, rows_bnd(robots, T), dt)
                full = run(torch, h, ctl, dt, tab, bnd, idx=idx)
                assert_ran(h, overlap)
                ring = run(torch, h, ctl, dt, tab, bnd, idx=idx, ring=True)
                assert_ran(h, overlap)
                parent = run(torch, h, ctl, dt, tab, bnd, ring=True)
                assert_ran(h, overlap)
                label = f"N={N} T={T}"
                assert np.all(full["status"] == 0) and np.all(ring["status"] == 0), label
                assert same_bits(ring["kp"], full["kp"]), f"{label}: kp of the ring call differs from the full call's"
                for t in (T - 3, T - 2, T - 1):  # the ring's three complete slots
                    assert same_bits(ring["kp"][t], ring["states"][(t + 1) % 3][:, idx]), (label, t)
                for k in ("tip", "status", "G", "states"):
                    assert same_bits(ring[k], parent[k]), f"{label}: {k} differs from the parent's boundary call"
                assert same_bits(ring["kp"][:, :, -1, 12:15].transpose(1, 0, 2), ring["tip"]), f"{label}: the tip's key point is not the tip"
                assert not (ring["tip"] == SENT).any()


# ---------------------------------------------------------------------------
# 3. against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("fixture", ["base_motion", "tip_loads"])
def test_against_the_reference_fixtures(torch_cuda, monkeypatch, fixture, overlap):
    """The cases of a fixture in one batch at N = 10, every grid point marked, on a ring: kp[t] is state t + 1, and the
    fixture holds states 0 .. T-1."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden(fixture)
    N, idx = 10, POINTS[10]
    cases = BASE_CASES if fixture == "base_motion" else LOAD_CASES
    B, T = len(cases), g["ctl_n10"].shape[0]
    assert np.all(g["ier_n10"] == 1) and g["traj_n10"].shape == (B, T, 25, N)
    r = make_robot(None, N)
    h = r._native()
    h.set_option("overlap", overlap)
    bnd = np.tile(row_boundary(r), (B, T, 1))
    if fixture == "base_motion":
        bnd[:, :, :13] = g["base_n10"]
    else:
        bnd[:, :, 13:] = g["loads_n10"]
    ctl = np.stack([g["ctl_n10"]] * B)
    with h.param_table([r._params()] * B) as tab:
        for dtype in (torch.float64, torch.float32):
            a = run(torch, h, dev(torch, ctl, dtype), dtype, tab, dev(torch, bnd, dtype), idx=idx, ring=True)
            assert_ran(h, overlap)
            assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            got = unpack(a["kp"]).transpose(1, 0, 2, 3)  # [B, T, 25, N]
            for c, case in enumerate(cases):
                if dtype == torch.float64:
                    check(f"{fixture} overlap={overlap} {case} trajectory", rel_l2(got[c, :T - 1], g["traj_n10"][c][1:]), 1e-8)
                else:
                    check(f"{fixture} overlap={overlap} {case} fp32 tips", rel_l2(got[c, :T - 1, :3, -1], g["tips_n10"][c][1:]), 1e-5)


def test_against_the_reference_with_the_mlp_on(torch_cuda, monkeypatch):
    """sim_nn.npz ``elu6464`` (N = 20): the fixture's T controls give states 0 .. T-1 (the reference drops the last solve)."""
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("sim_nn")
    N, idx = int(g["elu6464_N"]), POINTS[20]
    assert N == 20
    r = make_robot(None, N)
    inject(r, orc.mlp_from_arrays(g, "mlp_elu6464"))
    h = r._native()
    ref = g["elu6464_traj"]
    T = ref.shape[0] - 1
    B = 2
    ctl = dev(torch, np.stack([g["elu6464_ctl"][:T]] * B), torch.float64)
    bnd = dev(torch, np.tile(row_boundary(r), (B, T, 1)), torch.float64)
    with h.param_table([r._params()] * B) as tab:
        a = run(torch, h, ctl, torch.float64, tab, bnd, idx=idx, ring=True, use_nn=True)
        assert_ran(h, 0)
    assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
    got = unpack(a["kp"]).transpose(1, 0, 2, 3)
    for b in range(B):
        check(f"elu6464 rod {b}, sixteen key points", rel_l2(got[b], ref[1:, :, idx]), 1e-8)


# ---------------------------------------------------------------------------
# 4. hand-over to the take-over launch, damped fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("history", ["alt", "jump"])
def test_hand_over_to_second_launch(torch_cuda, monkeypatch, history):
    """The maxit = 2 batches of tests/test_gpu_base_motion.py::test_hand_over_to_second_launch: the overlapped kernel gives
    rods up, the plain persistent kernel takes over at resume[rod] and writes the key points of every step from there on."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 6
    idx = POINTS[N]
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 77), dt)
    bnd = np.zeros((B, T, 19))
    bnd[:, :, :13] = np.stack([scaled(base_history(history, T), 1 + 0.25 * b) for b in range(B)])
    bnd = dev(torch, bnd, dt)
    with h.param_table([r._params()] * B) as tab:
        for overlap in (1, 0):
            h.set_option("overlap", overlap)
            a = run(torch, h, ctl, dt, tab, bnd, idx=idx, maxit=2)
            assert_ran(h, overlap)
            ar = run(torch, h, ctl, dt, tab, bnd, idx=idx, maxit=2, ring=True)
            assert_ran(h, overlap)
            print(f"{history} overlap={overlap}: steps not converged at the cap: {int((a['status'] != 0).sum())} of {B * T}")
            kp_is_the_states(a, idx, f"{history} overlap={overlap}")
            assert np.array_equal(ar["status"], a["status"])
            assert np.all(np.isfinite(a["kp"]))
            check(f"{history} overlap={overlap}: ring against full history, kp", rel_l2(ar["kp"], a["kp"]), 1e-9)
        h.set_option("overlap", 1)
        c = run(torch, h, ctl, dt, tab, bnd, idx=idx)
        assert np.all(c["status"] == 0)  # with the default cap everything converges again on the same handle
        kp_is_the_states(c, idx, history)


# ---------------------------------------------------------------------------
# 5. a failing rod
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("overlap", [1, 0])
def test_nan_tension_fails_one_rod_from_that_step(torch_cuda, monkeypatch, overlap, ring):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B, t0, sick = 23, 13, 6, 5, 1
    idx = POINTS[N]
    robots = boundary_rows(N)
    h = make_robot(None, N)._native()
    h.set_option("overlap", overlap)
    clean = sine_ctl(B, T, robots[0].del_t, 33)
    bad = clean.copy()
    bad[sick, t0, 1] = np.nan
    bnd = dev(torch, rows_bnd(robots, T), dt)
    with h.param_table([r._params() for r in robots]) as tab:
        want = run(torch, h, dev(torch, clean, dt), dt, tab, bnd, idx=idx, ring=ring)
        assert_ran(h, overlap)
        assert np.all(want["status"] == 0)
        got = run(torch, h, dev(torch, bad, dt), dt, tab, bnd, idx=idx, ring=ring)  # (run: no sentinel is left in kp)
        assert_ran(h, overlap)
        again = run(torch, h, dev(torch, clean, dt), dt, tab, bnd, idx=idx, ring=ring)
        assert_ran(h, overlap)
    print(f"overlap={overlap} ring={ring}: status of rod {sick}: {got['status'][sick].tolist()}")
    assert np.all(got["status"][sick, :t0] == 0) and got["status"][sick, t0] == 2 and np.all(got["status"][sick, t0 + 1:] != 0)
    others = [b for b in range(B) if b != sick]
    assert same_bits(got["kp"][:, others], want["kp"][:, others]), "kp of another rod differs from the clean call"
    assert same_bits(got["kp"][:t0, sick], want["kp"][:t0, sick]), "kp of the failing rod before t0 differs from the clean call"
    for k in ("status", "tip", "G"):
        assert same_bits(got[k][others], want[k][others]), f"{k} of another rod differs from the clean call"
    if not ring:
        kp_is_the_states(got, idx, "failing batch")
    for k in ("status", "tip", "G", "states", "kp"):  # nothing of the failure stays behind in the handle
        assert same_bits(again[k], want[k]), f"{k} of the next call differs from the clean call"


# ---------------------------------------------------------------------------
# 6. calls in pieces
# ---------------------------------------------------------------------------
def test_calls_in_pieces(torch_cuda, monkeypatch):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 6
    idx = POINTS[N]
    robots = boundary_rows(N)
    h = make_robot(None, N)._native()
    ctl = dev(torch, sine_ctl(B, T, robots[0].del_t, 21), dt)
    bnd = rows_bnd(robots, T)
    bnd[:, :, :13] = np.stack([base_history(c, T) for c in ("still", "slide", "tilt", "jump", "alt", "slide")])
    bnd = dev(torch, bnd, dt)
    with h.param_table([r._params() for r in robots]) as tab:
        one = run(torch, h, ctl, dt, tab, bnd, idx=idx)
        assert_ran(h, 1)
        assert np.all(one["status"] == 0)
        for keep in (0, 1):
            h.set_option("keep_predictor", 0)
            h.set_option("keep_predictor", keep)
            try:
                ch = run(torch, h, ctl, dt, tab, bnd, idx=idx, chunks=[5, 1, 7])
            finally:
                h.set_option("keep_predictor", 0)
            assert_ran(h, 1)
            assert np.all(ch["status"] == 0)
            kp_is_the_states(ch, idx, f"keep_predictor={keep} chunks")
            check(f"keep_predictor={keep} chunks, kp", rel_l2(ch["kp"][..., :25], one["kp"][..., :25]), 1e-7)


# ---------------------------------------------------------------------------
# 7. metrics
# ---------------------------------------------------------------------------
SCORED = [None, "damping", "short", "youngs", "lengthstiff", "nsw"]


def scored_run():
    """N = 23, T = 13, six presets under ONE tension history: rod 0 (no modification) is the reference of all.  (Presets
    whose trajectories leave the reference's visibly: a relative bound on an MSE says nothing about a rod that all but
    repeats the reference - ``noair`` scores 7e-10 here, and the angles' rounding alone is 2e-11 of that.)"""
    N, T, B = 23, 13, 6
    robots = [make_robot(m, N) for m in SCORED]
    ctl = np.stack([sine_ctl(1, T, robots[0].del_t, 707)[0]] * B)
    return N, T, B, robots, ctl


def test_pose_mse_points_and_dtw_on_kp(torch_cuda, monkeypatch):
    """Measured: kr_pose_mse_points_batch on kp against pos_euler_mse 2.1e-15 relative at most (fp64), 1.5e-15 (fp32
    inputs), bound 1e-13, on MSEs of 3.3e-2 .. 12.9."""
    from krod_eval import dtw_distance, pos_euler_mse
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    N, T, B, robots, ctl = scored_run()
    h = make_robot(None, N)._native()
    idx = [2, 6, 9, 22]
    for dt in (torch.float64, torch.float32):
        with h.param_table([r._params() for r in robots]) as tab:
            a = run(torch, h, dev(torch, ctl, dt), dt, tab, dev(torch, rows_bnd(robots, T), dt), idx=idx)
        assert_ran(h, 1)
        assert np.all(a["status"] == 0)
        states, kp = dev(torch, a["states"], dt), dev(torch, a["kp"], dt)
        ref = states[:, :1].contiguous()  # rod 0 (no modification) as the reference of all
        # P = N on a full history: kr_pose_mse_batch, bit for bit
        m_n, p_n = h.pose_mse(states, ref)
        m_p, p_p = h.pose_mse_points(states, ref)
        assert same_bits(m_p.cpu().numpy(), m_n.cpu().numpy()) and same_bits(p_p.cpu().numpy(), p_n.cpu().numpy())
        # P = K on kp against the reference gathered at the key points (states 1 .. T)
        ref_kp = ref[1:, :, idx].contiguous()
        got = h.pose_mse_points(kp, ref_kp)[0].cpu().numpy()
        rows, ref_rows = unpack(a["kp"]).transpose(1, 0, 2, 3), unpack(a["states"][1:, 0][:, idx])
        want = np.array([pos_euler_mse(rows[b], ref_rows) for b in range(B)])
        assert got[0] == 0.0 and want[0] == 0.0  # rod 0 is the reference
        assert np.all(want[1:] >= 1e-2), want  # (squared differences large enough for a relative bound to mean something)
        rel = np.abs(got[1:] - want[1:]) / want[1:]
        err = float(np.max(rel))
        print(f"{dt}: kr_pose_mse_points_batch on kp against pos_euler_mse, relative errors {rel} (bound 1e-13); mse {want[1:]}")
        assert err <= 1e-13, (got, want)
        # kr_dtw_batch on one column of kp: krod_eval.dtw_distance, bit for bit
        for k in (0, len(idx) - 1):
            d = h.dtw(kp[:, :, k, 12:15].permute(1, 0, 2), ref_kp[:, 0, k, 12:15].contiguous()).cpu().numpy()
            host = np.array([dtw_distance(rows[b][:, :3, k], ref_rows[:, :3, k]) for b in range(B)])
            assert same_bits(d, host), (k, d, host)


def test_simulate_batch_key_points_and_score(torch_cuda, monkeypatch):
    from knode import simulate_batch
    import krod_native as kn
    set_mode_env(monkeypatch, "overlap")
    N, T, B, robots, ctl = scored_run()
    carrier = make_robot(None, N)
    pts = [-1, 6, 2, 9, 6]  # the wrapper sorts, de-duplicates and counts negative indices from the tip
    full = simulate_batch(carrier, ctl, robots=robots, key_points=pts)
    assert_ran(carrier._handle, 1)
    assert full["key_points"].tolist() == [2, 6, 9, 22] and full["kp"].shape == (B, T + 1, 25, 4)
    assert same_bits(full["kp"], np.ascontiguousarray(full["traj"][:, :, :, [2, 6, 9, 22]]))
    plain = simulate_batch(carrier, ctl, robots=robots)  # the table call: a constant boundary changes nothing
    for k in ("tip", "status", "G", "traj"):
        assert same_bits(full[k], plain[k]), k
    ref = full["traj"][0]
    for point in (-1, 6):
        score = {"reference": ref, "point": point}
        want = simulate_batch(carrier, ctl, robots=robots, score=score)
        both = simulate_batch(carrier, ctl, robots=robots, key_points=pts, score=score)
        lean = simulate_batch(carrier, ctl, robots=robots, key_points=pts, score=score, tip_only=True)
        assert_ran(carrier._handle, 1)
        assert "traj" not in lean and "mse" not in lean and "mse_kp" not in want
        assert same_bits(lean["dtw"], want["dtw"]) and same_bits(both["dtw"], want["dtw"]) and same_bits(both["mse"], want["mse"])
        assert same_bits(lean["mse_kp"], both["mse_kp"]) and same_bits(lean["kp"], full["kp"]) and same_bits(lean["tip"], full["tip"])
        assert lean["mse_kp"][0] == 0.0 and np.all(lean["mse_kp"][1:] > 0)
    with pytest.raises(kn.KrError, match="not one of the key points"):
        simulate_batch(carrier, ctl, robots=robots, key_points=pts, score={"reference": ref, "point": 5}, tip_only=True)
    # composes with base_motion and tip_loads
    M = np.stack([base_history(c, T) for c in ("slide", "tilt", "alt", "jump", "alt", "still")])
    L = np.tile(np.array([0.02, -0.01, 0.03, 1e-3, -5e-4, 2e-4]), (B, T, 1))
    moved = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_loads=L, key_points=pts)
    parent = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_loads=L)
    assert same_bits(moved["traj"], parent["traj"]) and same_bits(moved["kp"], np.ascontiguousarray(parent["traj"][:, :, :, [2, 6, 9, 22]]))
    lean = simulate_batch(carrier, ctl, robots=robots, base_motion=M, tip_loads=L, key_points=pts, tip_only=True)
    assert same_bits(lean["kp"], moved["kp"])


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch_cuda, monkeypatch):
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    T, B = 12, 6
    NAME = "kr_simulate_batch_keypoints"
    idx = [3, 5, 7, 9]

    def setup(N):
        r = make_robot(None, N)
        h = r._native()
        ctl = dev(torch, sine_ctl(B, T, r.del_t, 9), dt)
        bnd = np.tile(row_boundary(r), (B, T, 1))
        bnd[:, :, :13] = base_history("slide", T)
        st = h.new_state(B, dt, n_slots=T + 1)
        return r, h, ctl, dev(torch, bnd, dt), st

    G = torch.full((B, 6), SENT, dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dt, device=DEV)
    status = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    kp = torch.full((T, B, len(idx), 28), SENT, dtype=dt, device=DEV)

    def untouched(st):
        torch.cuda.synchronize()
        return bool((st[1:] == 0).all() and (G == SENT).all() and (tip == SENT).all() and (status == -7).all() and (kp == SENT).all())

    def raw(h, ctl, st, table, bnd, pts=idx, kp_=kp, scheme=kn.KR_EULER, K=None):
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        arr = (C.c_int32 * max(len(pts), 1))(*pts)
        return h.lib.kr_simulate_batch_keypoints(h._h, table, T, scheme, p(ctl), p(bnd), len(pts) if K is None else K, arr, p(kp_),
                                                 p(st), 0, p(G), p(tip), 0.0, 0, p(status), 0, None, kn.dtype_code(dt), None)

    def last():
        return tuple(h.get_option(o) for o in ("last_sim_path", "last_waves_per_rod", "last_overlap"))

    def refused(h, rc, code, *words):
        assert rc == code, (rc, h.lib.kr_last_error().decode())
        msg = h.lib.kr_last_error().decode()
        assert NAME in msg and all(w in msg for w in words), msg

    r, h, ctl, bnd, st = setup(23)
    with h.param_table([r._params()] * B) as tab:
        ok = run(torch, h, ctl, dt, tab, bnd, idx=idx)
        assert_ran(h, 1)
        assert np.all(ok["status"] == 0)
        h.init_straight(st[0], table=tab)
        before = last()
        # the point set: decided on the host, the first bad entry named
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=[]), kn.KR_E_ARG, "K = 0")
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=list(range(17))), kn.KR_E_ARG, "K = 17")
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=[3, 5, 5, 9]), kn.KR_E_ARG, "idx[2] = 5")
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=[3, 9, 7, 11]), kn.KR_E_ARG, "idx[2] = 7")
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=[-1, 5, 7, 9]), kn.KR_E_ARG, "idx[0] = -1")
        refused(h, raw(h, ctl, st, tab._t, bnd, pts=[3, 5, 7, 23]), kn.KR_E_ARG, "idx[3] = 23", "[0, 23)")
        assert untouched(st) and last() == before
        # required pointers
        refused(h, raw(h, ctl, st, tab._t, bnd, kp_=None), kn.KR_E_ARG, "kp")
        refused(h, raw(h, ctl, st, tab._t, None), kn.KR_E_ARG, "bnd")
        refused(h, raw(h, ctl, st, None, bnd), kn.KR_E_ARG, "null pointer argument: t")
        assert untouched(st) and last() == before
        # what the boundary call refuses
        refused(h, raw(h, ctl, st, tab._t, bnd, scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, "Euler")
        assert untouched(st) and last() == before
        h.set_option("waves_per_rod", 2)
        refused(h, raw(h, ctl, st, tab._t, bnd), kn.KR_E_UNSUPPORTED, "waves_per_rod = 2", "key-point calls run one wavefront per rod")
        assert untouched(st) and last() == before
        h.set_option("waves_per_rod", 1)
        h.set_option("persistent", 0)
        refused(h, raw(h, ctl, st, tab._t, bnd), kn.KR_E_UNSUPPORTED, "persistent = 0")
        assert untouched(st) and last() == before
        h.set_option("persistent", 1)
        again = run(torch, h, ctl, dt, tab, bnd, idx=idx)
        assert_ran(h, 1)
        assert same_bits(again["kp"], ok["kp"]) and same_bits(again["tip"], ok["tip"])
    # N = 8: no table can be made for the call to take (the table family's range, 9 <= N <= 128); without one the call
    # is refused by name
    r8, h8, ctl8, bnd8, st8 = setup(8)
    with pytest.raises(kn.KrError, match=r"N = 8.*9 <= N <= 128"):
        h8.param_table([r8._params()] * B)
    refused(h8, raw(h8, ctl8, st8, None, bnd8), kn.KR_E_ARG, "null pointer argument: t")
    assert untouched(st8)
