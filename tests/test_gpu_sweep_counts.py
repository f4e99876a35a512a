"""Newton sweep counts with the MLP off, per step kernel, against the oracle's (``-m gpu``; tests/sweep_count_cases.py has
the cases, the mutants and the bounds, tests/test_sweep_counts_cpu.py proves what each row here holds).

A step kernel finds the same root whatever its forward-difference Jacobian and its start values are, so no comparison of
trajectories or of ``status`` sees a wrong column, a perturbed sweep that reads the wrong history, a wrong RK4 stage of a
perturbed sweep or a time extrapolation that is not applied: only ``iters`` does.  Per rod, ``sum(iters)`` over the steps
must stay at or below  S_exact + slack + (S_held_min - S_exact) / 3  (sweep_count_cases.jac_row / start_row).

a. kr_step_batch step by step, G carried, ``predictor = 0``: K2a (step_kernel) at N = 9, 20; K2b (ms_step_kernel) at
   N = 9, 20, 27; K2d (msw_step_kernel) with 2 wavefronts at N = 20, 27 and 4 at N = 27, 40; fp64 and fp32; Euler on four
   parameter sets, RK4 on "full-asym" and its twin (K2d has Euler sweeps only).
b. the same loop with ``predictor`` 1, 2 and -1 at ``tol = 1e-10``, 16 steps, fp64, on K2a and K2b.
c. kr_debug_buffer: the per-step kr_simulate_batch writes the same counts as the loop of a. / b. with the same order, every
   entry of int32 [B][T] and nothing else; NULL switches it off; a persistent call leaves the buffer alone.
d. rod b's counts in the batch are those of its own B = 1 call (K2a: eight rods share a wavefront; K2b).

Every test asserts the kernel that ran, every ``status == 0``, every count >= 1, and the trajectory against the C oracle's
tight solve at the project's bounds (fp64: tips 1e-8, a block of the states 1e-7; fp32: tips 1e-5): a kernel cannot pass by
stopping early."""
import numpy as np
import pytest

import full_matrix_cases as fm
import sweep_count_cases as cc
from gpu_helpers import assert_path, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEME = {"euler": 0, "rk4": 1}  # KR_EULER, KR_RK4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def tdtype(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def make_handle(setenv, family, pset, N):
    """(robot, handle, path that must run, wavefronts per rod that must run); the robot owns the handle."""
    mode, W, grids = cc.FAMILIES[family]
    assert N in grids and (W == 1 or N - 1 >= 2 * (4 + 3 * (W - 1))), (family, N)
    set_mode_env(setenv, mode, waves_per_rod=W)
    r = cc.gpu_robot(pset, N)
    return r, r._native(), (0 if mode == "single" else 1), W


def ran(h, want, W):
    assert_path(h, want, waves_per_rod=W)
    got = h.get_option("last_waves_per_rod")
    assert got == W, f"{got} wavefronts per rod ran, the test is meant to exercise {W}"


def traj_of(torch, h, states):
    """float64[B, T + 1, 25, N] in the reference's row order from a full state history [T + 1, B, N, slots]."""
    out = []
    for t in range(states.shape[0]):
        y, z = h.unpack(states[t].contiguous())
        out.append(torch.cat([y, z], dim=1).double().cpu().numpy())
    return np.stack(out, axis=1)


def step_loop(torch, h, ctl, dtype, scheme, predictor, tol, want, W):
    """kr_step_batch over the steps of ctl[B, T, 4] from the straight rod, G carried, every state the loop has handed over
    (``prev2`` as test_gpu_bc.py::test_step_batch passes it): (iters int[B, T], status int[B, T], trajectory)."""
    dt = tdtype(torch, dtype)
    ctl = torch.as_tensor(np.asarray(ctl, dtype=np.float64), device=DEV).to(dt).contiguous()
    nb, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(nb, dt, n_slots=T + 1)
    h.init_straight(st[0])
    G = torch.zeros((nb, 6), dtype=dt, device=DEV)
    status = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
    iters = torch.zeros((nb,), dtype=torch.int32, device=DEV)
    got_iters, got_status = [], []
    for t in range(T):
        prev = st[t - 1] if t else st[0]
        h.step(prev, st[t], st[t + 1], G, ctl[:, t].contiguous(), scheme=SCHEME[scheme], tol=tol, status=status, iters=iters,
               prev2=st[t - 2] if t >= 2 else None, predictor=predictor)
        torch.cuda.synchronize()
        ran(h, want, W)
        got_iters.append(iters.cpu().numpy().copy())
        got_status.append(status.cpu().numpy().copy())
    return np.array(got_iters).T, np.array(got_status).T, traj_of(torch, h, st)


def check_answer(label, iters, status, traj, ref, dtype):
    assert np.all(status == 0), (label, np.argwhere(status != 0)[:8])
    assert np.all(iters >= 1), (label, iters)
    assert traj.shape == ref.shape, (traj.shape, ref.shape)
    tip_tol, state_tol = fm.TOL[dtype]
    for b in range(traj.shape[0]):
        te = fm.tip_error(traj[b, 1:, :3, -1], ref[b, 1:, :3, -1])
        print(f"{label} rod {b}: tips {te:.2e} (bound {tip_tol:.0e})")
        assert te < tip_tol, (label, b, te)
        if dtype == "f64":
            be = fm.block_errors(traj[b, 1:], ref[b, 1:])
            print(f"{label} rod {b}: {fm.fmt_blocks(be)} (bound {state_tol:.0e})")
            assert all(e < state_tol for e in be.values()), (label, b, be)


def check_counts(label, iters, row):
    over = []
    for b in range(iters.shape[0]):
        s = int(iters[b].sum())
        print(f"{label} rod {b}: GPU sweeps {iters[b].tolist()} = {s} | oracle exact {row['exact'][b].tolist()} = {int(row['s_exact'][b])} | "
              f"slack {row['slack']} held {row['held']} | bound {row['bound'][b]:.2f}")
        if not s <= row["bound"][b]:
            over.append((b, s, row["bound"][b]))
    assert not over, f"{label} (rod, GPU sweeps, bound): {over}"


# ---------------------------------------------------------------------------
# a. the Jacobian: predictor 0, default tolerances
# ---------------------------------------------------------------------------
JAC_ROWS = [r for r in cc.jac_rows() if cc.jac_row(*r)["bound"] is not None]


@pytest.mark.parametrize("family,scheme,pset,N,dtype", JAC_ROWS, ids=["-".join(map(str, r)) for r in JAC_ROWS])
def test_jacobian_sweep_counts(torch_cuda, monkeypatch, family, scheme, pset, N, dtype):
    torch = torch_cuda
    r, h, want, W = make_handle(monkeypatch, family, pset, N)
    iters, status, traj = step_loop(torch, h, cc.controls(cc.T_JAC), dtype, scheme, 0, 0.0, want, W)
    label = f"{family} {scheme} {pset} N={N} {dtype}"
    row = cc.jac_row(family, scheme, pset, N, dtype)
    for b in range(cc.B):
        print(f"{label} rod {b}: GPU sweeps {iters[b].tolist()}")
    check_answer(label, iters, status, traj, cc.exact_states(pset, scheme, N, cc.T_JAC), dtype)
    check_counts(label, iters, row)


# ---------------------------------------------------------------------------
# b. the start values: predictor 1, 2, -1 at tol = 1e-10
# ---------------------------------------------------------------------------
START_ROWS = [r for r in cc.start_rows() if cc.start_row(*r)["bound"] is not None]


@pytest.mark.parametrize("family,scheme,pset,N,rule", START_ROWS, ids=["-".join(map(str, r)) for r in START_ROWS])
def test_start_value_sweep_counts(torch_cuda, monkeypatch, family, scheme, pset, N, rule):
    torch = torch_cuda
    r, h, want, W = make_handle(monkeypatch, family, pset, N)
    iters, status, traj = step_loop(torch, h, cc.controls(cc.T_START), "f64", scheme, rule, cc.TOL_START, want, W)
    label = f"{family} {scheme} {pset} N={N} predictor={rule}"
    check_answer(label, iters, status, traj, cc.exact_states(pset, scheme, N, cc.T_START), "f64")
    check_counts(label, iters, cc.start_row(family, scheme, pset, N, rule))


# ---------------------------------------------------------------------------
# c. kr_debug_buffer
# ---------------------------------------------------------------------------
SENTINEL = -77


def set_debug_buffer(h, buf):
    import krod_native as kn
    kn.check(h.lib.kr_debug_buffer(h._h, kn._ptr(buf) if buf is not None else None))


def simulate(torch, h, ctl, dt):
    nb, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(nb, dt, n_slots=T + 1)
    h.init_straight(st[0])
    G = torch.zeros((nb, 6), dtype=dt, device=DEV)
    status = torch.full((nb, T), -1, dtype=torch.int32, device=DEV)
    try:
        h.simulate(ctl, st, G, status=status)
    finally:
        torch.cuda.synchronize()
    return status.cpu().numpy(), st


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("family,N", [("K2a", 20), ("K2b", 27)])
def test_debug_buffer(torch_cuda, monkeypatch, family, N, order):
    """The per-step kr_simulate_batch forms the same start as the loop of a. / b. (kr_api.hip, simulate_impl: order
    min(option, 2), limited by the states there are; the predictor image of ``pred_limit`` is only kept for options above
    2), so its counts ARE that loop's, entry by entry."""
    torch = torch_cuda
    pset, dtype, T, nb = "preset", "f64", cc.T_JAC, cc.B
    dt = tdtype(torch, dtype)
    r, h, want, W = make_handle(monkeypatch, family, pset, N)
    ctl = torch.as_tensor(np.asarray(cc.controls(T)), device=DEV).to(dt).contiguous()
    # guard row | the counts [B][T], in a region of B * 24 * 8 bytes (what a build with cycle stamps would fill) | guard row
    body = max(nb * T, nb * 24 * 2)
    buf = torch.full((T + body + T,), SENTINEL, dtype=torch.int32, device=DEV)
    payload = buf[T:T + body]
    h.set_option("persistent", 0)
    h.set_option("predictor", order)
    try:
        set_debug_buffer(h, payload)
        status, st = simulate(torch, h, ctl, dt)
        ran(h, want, W)
        got = buf.cpu().numpy().copy()
        counts = got[T:T + nb * T].reshape(nb, T)
        assert np.all(got[:T] == SENTINEL) and np.all(got[T + nb * T:] == SENTINEL), "written outside int32 [B][T]"
        assert np.all(counts != SENTINEL) and np.all(counts >= 1), counts
        label = f"{family} N={N} per-step simulate, predictor option {order}"
        check_answer(label, counts, status, traj_of(torch, h, st), cc.exact_states(pset, "euler", N, T), dtype)
        loop_iters, loop_status, _ = step_loop(torch, h, cc.controls(T), dtype, "euler", order, 0.0, want, W)
        print(f"{label}: buffer {counts.tolist()} | kr_step_batch loop {loop_iters.tolist()}")
        assert np.array_equal(counts, loop_iters)
        buf.fill_(SENTINEL)
        if family == "K2b":  # (a single-shooting handle has no persistent form)
            # a persistent call with the buffer set: a release build has no cycle stamps, nothing is written
            h.set_option("persistent", 1)
            status, _ = simulate(torch, h, ctl, dt)
            assert h.get_option("last_sim_path") == 2, "the persistent kernel did not run"
            assert np.all(status == 0)
            assert np.all(buf.cpu().numpy() == SENTINEL), "a persistent call wrote into the diagnostics buffer"
            h.set_option("persistent", 0)
        # NULL switches it off
        set_debug_buffer(h, None)
        status, _ = simulate(torch, h, ctl, dt)
        ran(h, want, W)
        assert np.all(status == 0)
        assert np.all(buf.cpu().numpy() == SENTINEL), "written after kr_debug_buffer(NULL)"
    finally:
        set_debug_buffer(h, None)


# ---------------------------------------------------------------------------
# d. independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("family,N", [("K2a", 20), ("K2b", 9)])
def test_counts_of_a_rod_are_its_own(torch_cuda, monkeypatch, family, N, dtype):
    torch = torch_cuda
    pset, T = "damping", cc.T_JAC
    r, h, want, W = make_handle(monkeypatch, family, pset, N)
    ctl = cc.controls(T)
    iters, status, traj = step_loop(torch, h, ctl, dtype, "euler", 0, 0.0, want, W)
    check_answer(f"{family} N={N} {dtype} batch", iters, status, traj, cc.exact_states(pset, "euler", N, T), dtype)
    for b in range(cc.B):
        i1, s1, _ = step_loop(torch, h, ctl[b:b + 1], dtype, "euler", 0, 0.0, want, W)
        print(f"{family} N={N} {dtype} rod {b}: in the batch {iters[b].tolist()} | alone {i1[0].tolist()}")
        assert np.all(s1 == 0) and np.array_equal(i1[0], iters[b])
