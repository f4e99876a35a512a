"""GPU tests (``-m gpu``) of the forms the overlapped persistent kernel gives the ends of its step (kr_mso_impl.hpp):

* the merged sweep's edge trips - trip 0 (no forward-difference lane live), the trailing trips, and the FINAL trip of a
  sweep that also runs step t + 1, which evaluates and advances only: it reads no tile, forms no record and stores
  nothing.  A lane that needed what the final trip leaves out shows as an end state formed from another grid point;
* the chord verdict - the first hop of its chain formed from the end states by the lanes that use it, ``d = T^-1 rt`` one
  component per lane and broadcast - which ``residual_test = 0`` makes the verdict of every step;
* the predictor's refit with its nine sums reduced stage by stage, which a kept fit carries across call boundaries.

Grids (what the sweep is with four intervals):

    N = 9        two segments per interval: trip 0, no full trip, the final trip
    N = 10..12   every remainder of (N - 1) / 4: lanes leave their interval in different trailing trips
    N = 13       one pair of full trips
    N = 17       a pair and a remainder trip
    N = 101      the headline workload's own split

The yardstick is the plain persistent kernel (overlap = 0) with the bounds of test_gpu_overlap.py (1e-8 fp64, 2e-5
fp32) on tips and on the position slots of every stored record; where the same kernel runs twice the results must be
equal bit for bit.  Inputs and helpers are those of test_gpu_mso_small.py / test_gpu_mso_update_tail.py."""
import functools

import numpy as np
import pytest

from gpu_helpers import make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_SMALL = 5  # one workgroup of four rods + one with three idle wavefronts
T_SHORT = 6
GRIDS = [9, 10, 11, 12, 13, 17, 101]


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


def _dt(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def _run(torch, h, ctl, dt, overlap, ring=False, table=None, maxit=0):
    """one call from the straight rod; asserts which kernel ran"""
    B, T = ctl.shape[0], ctl.shape[1]
    h.set_option("overlap", overlap)
    st = h.new_state(B, dt, n_slots=3 if ring else T + 1)
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    if table is None:
        h.init_straight(st[0])
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, maxit=maxit)
    else:
        h.init_straight(st[0], table=table)
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, maxit=maxit)
    torch.cuda.synchronize()
    assert h.get_option("last_overlap") == overlap and h.get_option("last_sim_path") == 2
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def _ring_calls(torch, h, ctl, dt, chunks):
    """the trajectory in several calls on ONE 3-slot ring, handed from call to call the way bench.py does it: every call
    starts from slot 0, the state before it comes in as prev_init"""
    B = ctl.shape[0]
    h.set_option("overlap", 1)
    st = h.new_state(B, dt, n_slots=3)
    h.init_straight(st[0])
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tips, stats, prev, t0 = [], [], None, 0
    for K in chunks:
        tip = torch.empty((B, K, 3), dtype=dt, device=DEV)
        status = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
        h.simulate(ctl[:, t0:t0 + K].contiguous(), st, G, ring=True, tip=tip, status=status, prev_init=prev)
        assert h.get_option("last_overlap") == 1 and h.get_option("last_sim_path") == 2
        newest, prev = st[K % 3].clone(), st[(K - 1) % 3].clone()
        st[0].copy_(newest)
        tips.append(tip)
        stats.append(status)
        t0 += K
    torch.cuda.synchronize()
    return dict(tip=torch.cat(tips, 1).double().cpu().numpy(), status=torch.cat(stats, 1).cpu().numpy(),
                last=st[0].double().cpu().numpy())


def _close(a, b, dtype, label, rods=None):
    """overlap = 1 (a) against overlap = 0 (b), full trajectories: equal status, tips within the bound per rod, and the
    position slots of EVERY stored record within the same bound relative to the largest entry"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    rods = np.arange(a["tip"].shape[0]) if rods is None else rods
    ta, tb = a["tip"][rods], b["tip"][rods]
    assert np.array_equal(a["status"][rods], b["status"][rods]), (label, a["status"].tolist(), b["status"].tolist())
    err = np.linalg.norm((ta - tb).reshape(len(rods), -1), axis=1) / np.linalg.norm(tb.reshape(len(rods), -1), axis=1)
    pa, pb = a["states"][:, rods, :, 12:15], b["states"][:, rods, :, 12:15]
    perr = np.abs(pa - pb).max() / np.abs(pb).max()
    print(f"  {label}: tip err {err.max():.2e}, positions of all records {perr:.2e} (bound {tol:.0e})")
    assert np.all(np.isfinite(a["states"][:, rods])), label
    assert err.max() < tol, label
    assert perr < tol, label


def _ctl(torch, r, N, dt):
    return torch.as_tensor(_sine(B_SMALL, T_SHORT, r.del_t, 40 + N), device=DEV).to(dt).contiguous()


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_edge_trip_against_the_plain_kernel(torch_cuda, monkeypatch, N, dtype):
    """Six steps as a full trajectory, overlap = 1 against overlap = 0: status (all converged: no rod leaves the
    overlapped kernel), tips and the positions of every stored record."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = _dt(torch, dtype)
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    a = _run(torch, h, ctl, dt, 1)
    assert np.all(a["status"] == 0), a["status"].tolist()
    _close(a, _run(torch, h, ctl, dt, 0), dtype, f"N={N} {dtype}")


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chord_verdict_on_every_step(torch_cuda, monkeypatch, N, dtype):
    """``residual_test = 0``: every verdict is the chord verdict.  Every step converges on the sine inputs; same bounds
    against the plain kernel with the same option."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = _dt(torch, dtype)
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    assert h.get_option("residual_test") == 1
    h.set_option("residual_test", 0)
    try:
        a = _run(torch, h, ctl, dt, 1)
        b = _run(torch, h, ctl, dt, 0)
    finally:
        h.set_option("residual_test", 1)
    assert np.all(a["status"] == 0), a["status"].tolist()
    _close(a, b, dtype, f"N={N} {dtype} chord")


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_same_kernel_twice_is_bit_equal(torch_cuda, monkeypatch, N, dtype):
    """Ring call (lean full trips) against trajectory call (complete full trips): tips, status, the three complete states
    a ring keeps.  A parameter table of identical rows (the table twin of the kernel) against the plain call: every
    output.  All bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = _dt(torch, dtype)
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    T = T_SHORT
    full = _run(torch, h, ctl, dt, 1)
    ring = _run(torch, h, ctl, dt, 1, ring=True)
    with h.param_table([r._params()] * B_SMALL) as tab:
        tabd = _run(torch, h, ctl, dt, 1, table=tab)
    assert np.all(full["status"] == 0), full["status"].tolist()
    assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(ring["states"][k % 3], full["states"][k]), k
    for key in ("status", "tip", "G", "states"):
        assert np.array_equal(full[key], tabd[key]), ("table", key)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rejections_apply_the_chord_update(torch_cuda, monkeypatch, dtype):
    """The "random" inputs of test_gpu_mso_small.py::test_rough_inputs at N = 12 with an iteration cap of 3 on a 3-slot
    ring: verifying sweeps are rejected, the chord update is applied to the unknowns and the step verified again or
    rolled back.  Status equal to the plain kernel's with the same cap."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = _dt(torch, dtype)
    r = make_robot(None, 12)
    h = r._native()
    B, T = 8, 40
    ctl = 5.0 + 5.0 * np.random.default_rng(5).uniform(size=(B, T, 4))
    ctl_t = torch.as_tensor(ctl, device=DEV).to(dt).contiguous()
    a = _run(torch, h, ctl_t, dt, 1, ring=True, maxit=3)
    b = _run(torch, h, ctl_t, dt, 0, ring=True, maxit=3)
    print(f"  random {dtype}: steps not converged {int((a['status'] != 0).sum())} of {B * T}")
    assert np.all((a["status"] >= 0) & (a["status"] <= 2))
    assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sick_rod_beside_healthy_ones(torch_cuda, monkeypatch, dtype):
    """One rod of five (N = 12) with a NaN tension from step 2 on: that rod alone reports it (status 2 from that step),
    the other four match the plain kernel on the same inputs."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = _dt(torch, dtype)
    N, s, t0 = 12, 2, 2
    r = make_robot(None, N)
    h = r._native()
    sick_np = np.array(_sine(B_SMALL, T_SHORT, r.del_t, 40 + N))
    sick_np[s, t0:, 1] = np.nan
    ctl = torch.as_tensor(sick_np, device=DEV).to(dt).contiguous()
    a = _run(torch, h, ctl, dt, 1)
    b = _run(torch, h, ctl, dt, 0)
    got = a["status"][s]
    print(f"  {dtype}: sick rod status {got.tolist()}")
    assert np.all(got[:t0] == 0) and np.all(got[t0:] == 2), got.tolist()
    healthy = np.flatnonzero(np.arange(B_SMALL) != s)
    assert np.all(a["status"][healthy] == 0), a["status"].tolist()
    _close(a, b, dtype, f"sick rod {dtype}", rods=healthy)


@pytest.mark.parametrize("N", [12, 101])
def test_kept_predictor_across_calls(torch_cuda, monkeypatch, N):
    """Three ring calls of six steps with keep_predictor = 1 (the predictor image goes through HBM, bench.py's way of
    calling) against one call of 18: the refit and the kept fit cross call boundaries.  Status, tips and the last
    state bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    r = make_robot(None, N)
    h = r._native()
    T = 3 * T_SHORT
    ctl = torch.as_tensor(_sine(B_SMALL, T, r.del_t, 60 + N), device=DEV).contiguous()
    h.set_option("keep_predictor", 0)
    h.set_option("keep_predictor", 1)
    try:
        one = _run(torch, h, ctl, torch.float64, 1, ring=True)
        h.set_option("keep_predictor", 0)
        h.set_option("keep_predictor", 1)
        ch = _ring_calls(torch, h, ctl, torch.float64, [T_SHORT] * 3)
    finally:
        h.set_option("keep_predictor", 0)
    assert np.all(one["status"] == 0), one["status"].tolist()
    d_tip = np.abs(ch["tip"] - one["tip"]).max()
    d_st = np.abs(ch["last"][..., :25] - one["states"][T % 3][..., :25]).max()
    print(f"  N={N}: largest difference of tips {d_tip:.2e}, of the last state {d_st:.2e}")
    assert np.array_equal(ch["status"], one["status"])
    assert np.array_equal(ch["tip"], one["tip"])
    assert np.array_equal(ch["last"][..., :25], one["states"][T % 3][..., :25])
