"""GPU tests (``-m gpu``) of the merged trip of the overlapped persistent kernel (kr_mso_impl.hpp): the trip reads the
older tile of the next grid point in front of the verifying lanes' store block and the newest tile behind it, runs its
full trips two per pass in a ring-lean and in a complete copy, and on a lean ring step stores no record in the trailing
predicated trips.  The grids are those where the count of full trips changes shape: N = 13, 17, 21 have sbase = 3, 4, 5,
i.e. 2, 3, 4 full trips (one pair, a pair plus the remainder, two pairs); N = 14, 15, 16 have 1, 2, 3 intervals one
segment longer at sbase = 3 (a trailing predicated trip with one, two, three verifying lanes alive).  Calls of 1, 2, 4, 5
and 9 steps: on a 3-slot ring T = 4 is the first call with a lean step, T = 9 has lean steps on every ring slot.  The
yardstick is the plain persistent kernel (overlap = 0) at the tolerances of test_gpu_overlap.py; where the overlapped
kernel runs twice (ring, full trajectory) the results must be equal bit for bit."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from gpu_helpers import make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_SMALL = 5  # one workgroup of four rods + one with three idle wavefronts
CALLS = (1, 2, 4, 5, 9)


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


def _run(torch, h, ctl, dt, overlap, ring=False):
    """one call from the straight rod; asserts which kernel ran"""
    B, T = ctl.shape[0], ctl.shape[1]
    h.set_option("overlap", overlap)
    st = h.new_state(B, dt, n_slots=3 if ring else T + 1)
    h.init_straight(st[0])
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    h.simulate(ctl, st, G, ring=ring, tip=tip, status=status)
    torch.cuda.synchronize()
    assert h.get_option("last_overlap") == overlap and h.get_option("last_sim_path") == 2
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def _close(a, b, dtype, T, ring):
    """overlap = 1 (a) against overlap = 0 (b): the bounds of test_bench_workload_vs_plain_persistent"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    B = a["tip"].shape[0]
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B, -1), axis=1)
    print(f"  T={T} ring={ring}: tip err {err.max():.2e} (bound {tol:.0e})")
    assert err.max() < tol
    k = T % 3 if ring else T
    assert np.abs(a["states"][k] - b["states"][k]).max() < tol * np.abs(b["states"][k]).max()
    assert np.abs(a["G"] - b["G"]).max() < (1e-7 if dtype == "f64" else 1e-3) * max(1.0, np.abs(b["G"]).max())


@pytest.mark.parametrize("N", [13, 14, 15, 16, 17, 21])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_trip_shapes_and_call_lengths(torch_cuda, monkeypatch, N, dtype):
    """Every call length on every grid, full trajectory and ring: status 0 everywhere and the plain persistent kernel's
    tips, final state and base wrench; the ring call's tips and its last three states equal the trajectory call's bit
    for bit (the lean and the complete copy of the loop of full trips compute the same, and what a lean step leaves
    out of HBM is read by nobody)."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    for T in CALLS:
        ctl = torch.as_tensor(_sine(B_SMALL, max(CALLS), r.del_t, 140 + N)[:, :T], device=DEV).to(dt).contiguous()
        full = _run(torch, h, ctl, dt, 1)
        _close(full, _run(torch, h, ctl, dt, 0), dtype, T, False)
        ring = _run(torch, h, ctl, dt, 1, ring=True)
        _close(ring, _run(torch, h, ctl, dt, 0, ring=True), dtype, T, True)
        assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"])
        for k in range(max(0, T - 2), T + 1):  # the states a ring ends with are complete records
            assert np.array_equal(ring["states"][k % 3], full["states"][k]), (T, k)
        assert float(np.abs(full["states"][..., 25:]).max()) == 0.0  # padding slots


@pytest.mark.parametrize("kind", ["step", "random"])
@pytest.mark.parametrize("N", [13, 16])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rough_inputs_on_a_ring(torch_cuda, monkeypatch, kind, N, dtype):
    """The "step" and "random" inputs of test_gpu_mso_small.py::test_rough_inputs (its jumps at 14 / 40 and 28 / 40 of the
    call moved to steps 4 and 8 of 12) on a ring, with its bounds: verifying sweeps are rejected, verified again, the
    tiles rebuilt from HBM - from what lean steps have left there - and rods handed to the take-over kernel, all with
    the early reads of a trip in flight.  Equal status as the plain persistent kernel, its tips and last three states."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
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
    a = _run(torch, h, ctl_t, dt, 1, ring=True)
    b = _run(torch, h, ctl_t, dt, 0, ring=True)
    assert np.array_equal(a["status"], b["status"])
    tol = 1e-7 if dtype == "f64" else 5e-4
    e_tip = rel_l2(a["tip"], b["tip"])
    print(f"  tips: {e_tip:.2e} (bound {tol:.0e})")
    assert e_tip < tol
    for t in (T - 2, T - 1, T):
        e = rel_l2(a["states"][t % 3][..., :25], b["states"][t % 3][..., :25])
        print(f"  state {t}: {e:.2e} (bound {tol:.0e})")
        assert e < tol, t
    assert float(np.abs(a["states"][..., 25:]).max()) == 0.0  # padding slots
