"""GPU tests (``-m gpu``) of what a steady lean ring step of the overlapped persistent kernel (kr_mso_impl.hpp) leaves
out: on a 3-slot ring a step whose state is not among the last three of the call stores no full record for the last
grid point (its leading slots go out with the tile, like every other grid point's), and while the fitted recurrence
predicts well the predictor update takes a straight path of its own (mso_pred_update).  Shapes: B = 5 (one workgroup of
four rods + one with three idle wavefronts), N = 9, 10, 12, 101 - (N - 1) mod 4 = 0, 1, 3, 0, so the last interval,
whose verifying lane owns the last grid point, has every length relation to the others - fp64 and fp32.  A ring call of
T = 4 has one lean step, T = 5 two, T = 9 lean steps on every ring slot; T = 1 and T = 2 have none.  Where the overlapped
kernel runs twice (ring, full trajectory) the results must be equal bit for bit; the yardstick otherwise is the plain
persistent kernel (overlap = 0) at the tolerances of test_gpu_overlap.py / test_gpu_mso_small.py."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from gpu_helpers import make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_SMALL = 5
GRIDS = [9, 10, 12, 101]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _sine(B, T, del_t, seed):
    import cosserat_oracle as orc
    c = orc.batch_sine_controls(B, T, del_t, seed)
    c.setflags(write=False)
    return c


def _run(torch, h, ctl, dt, overlap, ring=False, maxit=0):
    """one call from the straight rod; asserts which kernel ran"""
    B, T = ctl.shape[0], ctl.shape[1]
    h.set_option("overlap", overlap)
    st = h.new_state(B, dt, n_slots=3 if ring else T + 1)
    h.init_straight(st[0])
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, maxit=maxit)
    torch.cuda.synchronize()
    assert h.get_option("last_overlap") == overlap and h.get_option("last_sim_path") == 2
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def _ring_calls(torch, h, ctl, dt, chunks, overlap):
    """the trajectory in several calls on ONE 3-slot ring, handed from call to call the way bench.py does it: every call
    starts from slot 0, the state before it comes in as prev_init"""
    B = ctl.shape[0]
    h.set_option("overlap", overlap)
    st = h.new_state(B, dt, n_slots=3)
    h.init_straight(st[0])
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tips, stats, prev, t0 = [], [], None, 0
    for K in chunks:
        tip = torch.empty((B, K, 3), dtype=dt, device=DEV)
        status = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
        h.simulate(ctl[:, t0:t0 + K].contiguous(), st, G, ring=True, tip=tip, status=status, prev_init=prev)
        assert h.get_option("last_overlap") == overlap and h.get_option("last_sim_path") == 2
        newest, prev = st[K % 3].clone(), st[(K - 1) % 3].clone()
        st[0].copy_(newest)
        tips.append(tip)
        stats.append(status)
        t0 += K
    torch.cuda.synchronize()
    return dict(tip=torch.cat(tips, 1).double().cpu().numpy(), status=torch.cat(stats, 1).cpu().numpy(),
                G=G.double().cpu().numpy(), last=st[0].double().cpu().numpy(), before=prev.double().cpu().numpy())


def _close(a, b, dtype, T):
    """a ring call with overlap = 1 (a) against overlap = 0 (b): the bounds of test_bench_workload_vs_plain_persistent"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    B = a["tip"].shape[0]
    assert np.array_equal(a["status"], b["status"])
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B, -1), axis=1)
    print(f"  T={T}: tip err {err.max():.2e} (bound {tol:.0e})")
    assert err.max() < tol
    k = T % 3
    assert np.abs(a["states"][k] - b["states"][k]).max() < tol * np.abs(b["states"][k]).max()
    assert np.abs(a["G"] - b["G"]).max() < (1e-7 if dtype == "f64" else 1e-3) * max(1.0, np.abs(b["G"]).max())


def _ring_against_trajectory(torch, N, dtype, calls):
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    for T in calls:
        ctl = torch.as_tensor(_sine(B_SMALL, 9, r.del_t, 170 + N)[:, :T], device=DEV).to(dt).contiguous()
        full = _run(torch, h, ctl, dt, 1)
        ring = _run(torch, h, ctl, dt, 1, ring=True)
        assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"]), T
        for k in range(max(0, T - 2), T + 1):  # the states a ring ends with are complete records
            assert np.array_equal(ring["states"][k % 3], full["states"][k]), (T, k)
        assert float(np.abs(ring["states"][..., 25:]).max()) == 0.0  # padding slots
        _close(ring, _run(torch, h, ctl, dt, 0, ring=True), dtype, T)


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ring_with_lean_steps_equals_trajectory(torch_cuda, monkeypatch, N, dtype):
    """Ring calls of 4, 5 and 9 steps against the trajectory-mode call of the same inputs: tips and status bit for bit,
    the last three states as complete records (what a lean step leaves out of HBM is read by nobody); and the plain
    persistent kernel's tips, final state and base wrench."""
    set_mode_env(monkeypatch, "overlap")
    _ring_against_trajectory(torch_cuda, N, dtype, (4, 5, 9))


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ring_calls_without_a_lean_step(torch_cuda, monkeypatch, N, dtype):
    """A one-step and a two-step ring call: every state is among the last three, no step is lean."""
    set_mode_env(monkeypatch, "overlap")
    _ring_against_trajectory(torch_cuda, N, dtype, (1, 2))


@pytest.mark.parametrize("kind", ["step", "random"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rough_inputs_small_iteration_cap(torch_cuda, monkeypatch, kind, dtype):
    """The "step" and "random" inputs of test_gpu_mso_trip.py::test_rough_inputs_on_a_ring at N = 12 with an iteration
    cap of 3 on a ring: verifying sweeps are rejected (the tiles rebuilt from what lean steps left in HBM) and a rod
    that runs into the cap is handed to the take-over kernel in the middle of the ring, which reads the leading slots
    of every grid point, v and u of the last one and full records at the interval starts from those states.  Against
    the overlap = 0 run of the same call.  A step that ends at the cap is no root, so what the two runs agree to there
    is what test_hand_over_to_second_launch asks (the same steps unconverged, tips to 1e-6 in fp64); the fp32 bound is
    the one of the rough-input tests (5e-4)."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, 12)
    h = r._native()
    B, T = 8, 12
    rng = np.random.default_rng(5)
    if kind == "step":
        ctl = np.full((B, T, 4), 5.0)
        jump = rng.uniform(0.5, 2.0, size=(B, 1))
        ctl[:, 4:, 0] += jump
        ctl[:, 4:, 3] += jump
        ctl[:, 8:, 1] += 0.5 * jump
    else:
        ctl = 5.0 + 5.0 * rng.uniform(size=(B, T, 4))
    ctl_t = torch.as_tensor(ctl, device=DEV).to(dt).contiguous()
    a = _run(torch, h, ctl_t, dt, 1, ring=True, maxit=3)
    b = _run(torch, h, ctl_t, dt, 0, ring=True, maxit=3)
    print(f"  unconverged rod-steps: {int((a['status'] != 0).sum())} / {int((b['status'] != 0).sum())} of {B * T}")
    assert np.all(a["status"] >= 0) and np.all(a["status"] <= 2)
    assert np.array_equal(a["status"] != 0, b["status"] != 0)
    assert np.all(np.isfinite(a["tip"]))
    tol = 1e-6 if dtype == "f64" else 5e-4
    e_tip = rel_l2(a["tip"], b["tip"])
    print(f"  tips: {e_tip:.2e} (bound {tol:.0e})")
    assert e_tip < tol
    for t in (T - 2, T - 1, T):
        e = rel_l2(a["states"][t % 3][..., :25], b["states"][t % 3][..., :25])
        print(f"  state {t}: {e:.2e} (bound {tol:.0e})")
        assert e < tol, t
    assert float(np.abs(a["states"][..., 25:]).max()) == 0.0  # padding slots
    # with the default cap the same inputs converge everywhere, with the bounds of test_rough_inputs_on_a_ring
    a = _run(torch, h, ctl_t, dt, 1, ring=True)
    b = _run(torch, h, ctl_t, dt, 0, ring=True)
    assert np.array_equal(a["status"], b["status"])
    tol = 1e-7 if dtype == "f64" else 5e-4
    assert rel_l2(a["tip"], b["tip"]) < tol
    for t in (T - 2, T - 1, T):
        assert rel_l2(a["states"][t % 3][..., :25], b["states"][t % 3][..., :25]) < tol, t


@pytest.mark.parametrize("N", [12, 101])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kept_predictor_three_ring_calls(torch_cuda, monkeypatch, N, dtype):
    """Three ring calls of seven steps with keep_predictor = 1 on smooth sine inputs: from the second call on the fitted
    recurrence is in use and good, i.e. the steady path of the predictor update runs, lean steps included, and its
    state crosses the calls through the image in HBM.  Against the overlap = 0 run of the same calls with the bounds
    of test_bench_workload_vs_plain_persistent.  (The predictor only chooses start values: a wrong decision there
    costs sweeps, or convergence - status -, and never gives another root; the event counts of the stamped builds are
    the check of the decisions themselves, LABBOOK.)"""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    ctl = torch.as_tensor(_sine(B_SMALL, 21, r.del_t, 190 + N), device=DEV).to(dt).contiguous()
    res = []
    for overlap in (1, 0):
        h.set_option("keep_predictor", 0)
        h.set_option("keep_predictor", 1)
        try:
            res.append(_ring_calls(torch, h, ctl, dt, [7, 7, 7], overlap))
        finally:
            h.set_option("keep_predictor", 0)
    a, b = res
    print(f"  unconverged rod-steps: {int((a['status'] != 0).sum())} / {int((b['status'] != 0).sum())}")
    assert np.array_equal(a["status"], b["status"])
    tol = 1e-8 if dtype == "f64" else 2e-5
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B_SMALL, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B_SMALL, -1), axis=1)
    print(f"  N={N}: tip err {err.max():.2e} (bound {tol:.0e})")
    assert err.max() < tol
    for key in ("last", "before"):
        assert np.abs(a[key] - b[key]).max() < tol * np.abs(b[key]).max(), key
    assert np.abs(a["G"] - b["G"]).max() < (1e-7 if dtype == "f64" else 1e-3) * max(1.0, np.abs(b["G"]).max())
