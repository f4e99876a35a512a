"""GPU tests (``-m gpu``) of the overlapped persistent kernel (kr_mso_impl.hpp) at the small shapes where its
bookkeeping between two sweeps can go wrong: the shortest grids it serves and every remainder of (N - 1) / 4, a batch
that leaves three wavefronts of a workgroup idle, calls of 1 .. 7 steps on a ring and as a full trajectory (the ring
slot advanced without a modulo, the `lean` records at the end of a call), chunked calls with and without the kept
predictor (the unknowns of two steps change places instead of being copied), rough inputs (rejection, second
verification, rebuild, retry, hand-over to the take-over kernel: the paths that read their arguments where they need
them) and a parameter table of identical rows.  The yardstick is the plain persistent kernel (overlap = 0), with the
tolerances of test_gpu_overlap.py; where the same kernel runs twice the results must be equal bit for bit."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from gpu_helpers import make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_SMALL = 5  # one workgroup of four rods + one with three idle wavefronts


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


def _run(torch, h, ctl, dt, overlap, ring=False, table=None):
    """one call from the straight rod; asserts which kernel ran"""
    B, T = ctl.shape[0], ctl.shape[1]
    h.set_option("overlap", overlap)
    st = h.new_state(B, dt, n_slots=3 if ring else T + 1)
    if table is None:
        h.init_straight(st[0])
    else:
        h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    if table is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status)
    else:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table)
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
                last=st[0].double().cpu().numpy(), before=prev.double().cpu().numpy())


def _close(a, b, dtype, T, ring):
    """overlap = 1 (a) against overlap = 0 (b): the bounds of test_bench_workload_vs_plain_persistent"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    B = a["tip"].shape[0]
    assert np.array_equal(a["status"], b["status"])
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B, -1), axis=1)
    print(f"  T={T} ring={ring}: tip err {err.max():.2e} (bound {tol:.0e})")
    assert err.max() < tol
    k = T % 3 if ring else T
    assert np.abs(a["states"][k] - b["states"][k]).max() < tol * np.abs(b["states"][k]).max()
    assert np.abs(a["G"] - b["G"]).max() < (1e-7 if dtype == "f64" else 1e-3) * max(1.0, np.abs(b["G"]).max())


@pytest.mark.parametrize("N", [9, 10, 11, 12, 101])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_short_calls_small_grids(torch_cuda, monkeypatch, N, dtype):
    """N = 9 is the shortest grid served; 10, 11, 12 have 1, 2, 3 intervals one segment longer; 101 is the longest fp64
    grid with four rods per workgroup.  Calls of 1, 2, 3, 4 and 7 steps, full trajectory and ring: equal status, tips,
    final state and base wrench as the plain persistent kernel; the ring call equals the trajectory call bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    for T in (1, 2, 3, 4, 7):
        ctl = torch.as_tensor(_sine(B_SMALL, 7, r.del_t, 40 + N)[:, :T], device=DEV).to(dt).contiguous()
        full = _run(torch, h, ctl, dt, 1)
        _close(full, _run(torch, h, ctl, dt, 0), dtype, T, False)
        ring = _run(torch, h, ctl, dt, 1, ring=True)
        _close(ring, _run(torch, h, ctl, dt, 0, ring=True), dtype, T, True)
        assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"])
        for k in range(max(0, T - 2), T + 1):  # the states a ring ends with are complete records
            assert np.array_equal(ring["states"][k % 3], full["states"][k]), (T, k)
        assert float(np.abs(full["states"][..., 25:]).max()) == 0.0  # padding slots


@pytest.mark.parametrize("N", [12, 100])
def test_one_step_ring_calls(torch_cuda, monkeypatch, N):
    """Seven ring calls of one step, each handed the state before it, against one ring call of seven steps (the bound
    of test_chunked_calls_ring_and_single_steps: the start values of a call's first steps differ)."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    r = make_robot(None, N)
    h = r._native()
    ctl = torch.as_tensor(_sine(B_SMALL, 7, r.del_t, 40 + N), device=DEV).contiguous()
    one = _run(torch, h, ctl, torch.float64, 1, ring=True)
    ch = _ring_calls(torch, h, ctl, torch.float64, [1] * 7)
    assert np.array_equal(ch["status"], one["status"])
    e_tip, e_st = rel_l2(ch["tip"], one["tip"]), rel_l2(ch["last"][..., :25], one["states"][7 % 3][..., :25])
    print(f"  N={N}: tips {e_tip:.2e}, last state {e_st:.2e} (bound 1e-7)")
    assert e_tip < 1e-7 and e_st < 1e-7
    assert rel_l2(ch["before"][..., :25], one["states"][6 % 3][..., :25]) < 1e-7


@pytest.mark.parametrize("N", [12, 100])
def test_kept_predictor_across_calls(torch_cuda, monkeypatch, N):
    """Three ring calls of five steps with keep_predictor = 1 (the predictor image goes through HBM, bench.py's way of
    calling) against one call of fifteen."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    r = make_robot(None, N)
    h = r._native()
    ctl = torch.as_tensor(_sine(B_SMALL, 15, r.del_t, 60 + N), device=DEV).contiguous()
    one = _run(torch, h, ctl, torch.float64, 1, ring=True)
    h.set_option("keep_predictor", 0)
    h.set_option("keep_predictor", 1)
    try:
        ch = _ring_calls(torch, h, ctl, torch.float64, [5, 5, 5])
    finally:
        h.set_option("keep_predictor", 0)
    assert np.array_equal(ch["status"], one["status"])
    e_tip, e_st = rel_l2(ch["tip"], one["tip"]), rel_l2(ch["last"][..., :25], one["states"][15 % 3][..., :25])
    print(f"  N={N}: tips {e_tip:.2e}, last state {e_st:.2e} (bound 1e-7)")
    assert e_tip < 1e-7 and e_st < 1e-7


@pytest.mark.parametrize("kind", ["step", "random"])
@pytest.mark.parametrize("N", [12, 100])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rough_inputs(torch_cuda, monkeypatch, kind, N, dtype):
    """The "step" and "random" inputs of test_rough_inputs_full_trajectory (jumps moved into 40 steps) with its
    bounds: steps need several sweeps, verifying sweeps are rejected, verified again, rolled back from HBM, restarted
    from the warm start or handed to the take-over kernel.  Equal status and stored states as the plain persistent
    kernel; the ring call equals the trajectory call bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    B, T = 8, 40
    rng = np.random.default_rng(5)
    if kind == "step":
        ctl = np.full((B, T, 4), 5.0)
        jump = rng.uniform(0.5, 2.0, size=(B, 1))
        ctl[:, 14:, 0] += jump
        ctl[:, 14:, 3] += jump
        ctl[:, 28:, 1] += 0.5 * jump
    else:
        ctl = 5.0 + 5.0 * rng.uniform(size=(B, T, 4))
    ctl_t = torch.as_tensor(ctl, device=DEV).to(dt).contiguous()
    a = _run(torch, h, ctl_t, dt, 1)
    b = _run(torch, h, ctl_t, dt, 0)
    assert np.array_equal(a["status"], b["status"])
    tol = 1e-7 if dtype == "f64" else 5e-4
    for t in (1, 13, 15, 19, 29, T):
        e = rel_l2(a["states"][t][..., :25], b["states"][t][..., :25])
        print(f"  state {t}: {e:.2e} (bound {tol:.0e})")
        assert e < tol, t
    assert float(np.abs(a["states"][..., 25:]).max()) == 0.0  # padding slots
    c = _run(torch, h, ctl_t, dt, 1, ring=True)
    assert np.array_equal(c["status"], a["status"]) and np.array_equal(c["tip"], a["tip"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(c["states"][k % 3], a["states"][k])


@pytest.mark.parametrize("N", [12, 100])
def test_table_of_identical_rows_bitwise(torch_cuda, monkeypatch, N):
    """One table call whose rows are all the handle's own parameters: the per-rod-table instantiation of the kernel
    computes what the plain call computes, bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    r = make_robot(None, N)
    h = r._native()
    ctl = torch.as_tensor(_sine(B_SMALL, 7, r.del_t, 80 + N), device=DEV).contiguous()
    plain = _run(torch, h, ctl, torch.float64, 1)
    with h.param_table([r._params()] * B_SMALL) as tab:
        tabd = _run(torch, h, ctl, torch.float64, 1, table=tab)
    for key in ("status", "tip", "G", "states"):
        assert np.array_equal(plain[key], tabd[key]), key
