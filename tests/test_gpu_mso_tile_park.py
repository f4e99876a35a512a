"""GPU tests (``-m gpu``) of the park of the overlapped persistent kernel (kr_mso_impl.hpp, fp64, one wavefront per
SIMD): a lean step of a ring call no longer copies its accepted tile of leading slots to HBM.  The tile a verification
overwrites is kept in registers, lane per grid point, and written back when the verification is rejected; a rod that
gives up flushes its two tiles before the take-over kernel reads them.

Grid sizes: 9 (the smallest the planner serves, two-point intervals), 33, 64 (one grid point per lane, the second
round of the park empty), 65 (one lane in the second round), 100, 109 and 128.  Both rounds of the park are full at
128, but four fp64 rods of that size do not fit a CU's LDS: the overlapped kernel serves N <= 109 in fp64 (measured:
the planner's choice for N = 100 .. 128), so 109 is the largest second round the park ever holds, and at 128 the
planner runs another kernel (one launch per step at these batch sizes), for which the same equalities must hold.  A full-trajectory call has no lean
step - it stores every state as before - so wherever the same inputs run once on a 3-slot ring and once as a
trajectory the two must agree bit for bit: tips, status and the three states the ring ends with.

Roll-back cases (B = 8).  What the stamped build of the parent commit counted for the ring call of each, summed over
the eight rods (the `rejects`, `rebuilds` and `resume_at` columns of tools/overlap_stats.py's debug buffer; the
take-over kernel writes its own record over the row of a rod it takes over, so a given-up rod's rejections are not
known):

  "step", T = 12, iteration cap 3 (test_gpu_mso_lean_step.py::test_rough_inputs_small_iteration_cap's inputs):
      N = 33: 2 rejections, 2 restores, no rod given up;  N = 65: the same.
      N = 9, 64, 100, 109: none (nor with jumps twice as high; four times as high, four or five rods are given up and
      the other rods reject nothing) - REPLACED there by "random18" below.
  "random", T = 12, iteration cap 3 (the same test's other inputs): all eight rods run into the cap and are given up
      inside the lean range at every N <= 109, every step converges in the take-over kernel.
  "random18": the random inputs over T = 18 with the default cap - no rod given up, every step converged:
      N = 9: 6 rejections and restores, 33: 6, 64: 4, 65: 4, 100: 3, 109: 4.
  N = 128: the overlapped kernel does not run (above).

Chained calls (three ring calls of six steps with a kept predictor, the random inputs, default cap), rejections in
calls 1 / 2 / 3 on the same build: N = 9: 1 / 5 / 0, 33: 0 / 4 / 2, 64: 0 / 3 / 1, 65: 0 / 3 / 1, 100: 0 / 2 / 1,
109: 0 / 3 / 1; no rod given up.  The second call's first rejections come within its first steps.
"""
import functools

import numpy as np
import pytest

import sick_rod_cases as sc
from conftest import rel_l2
from gpu_helpers import make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [9, 33, 64, 65, 100, 109, 128]
K2E_MAX_N = 109  # largest fp64 grid of the overlapped kernel: four rods share the LDS of a CU (module docstring)
B_ROUGH, T_ROUGH = 8, 12


def served(N):
    """whether the overlapped kernel serves an fp64 rod of N grid points (four rods share a CU's LDS)"""
    return N <= K2E_MAX_N


def assert_kernel(h, overlap):
    """the persistent kernel the call asked for - or, past the overlapped kernel's range, whatever the planner chose instead"""
    if served(h.N):
        assert h.get_option("last_overlap") == overlap and h.get_option("last_sim_path") == 2
    else:
        assert h.get_option("last_overlap") == 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _handle(N):
    """one robot and native handle per grid size, shared by the tests of this module"""
    r = make_robot(None, N)
    return r, r._native()


@functools.lru_cache(maxsize=None)
def sine_ctl(B, T, seed):
    import cosserat_oracle as orc
    c = orc.batch_sine_controls(B, T, sc.DEL_T, seed)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def rough_ctl(kind, B=B_ROUGH, T=T_ROUGH):
    """test_rough_inputs_small_iteration_cap's inputs: jumps at a third and two thirds of the call, or fresh random
    tensions at every step"""
    rng = np.random.default_rng(5)
    if kind == "step":
        ctl = np.full((B, T, 4), 5.0)
        jump = rng.uniform(0.5, 2.0, size=(B, 1))
        ctl[:, T // 3:, 0] += jump
        ctl[:, T // 3:, 3] += jump
        ctl[:, 2 * T // 3:, 1] += 0.5 * jump
    else:
        ctl = 5.0 + 5.0 * rng.uniform(size=(B, T, 4))
    ctl.setflags(write=False)
    return ctl


def run(torch, h, ctl, overlap, ring, maxit=0, first=None):
    """One fp64 call of the persistent kernel from the straight rod, or - first = (ctl of a call before it) - from where
    that call ended, with the state before it as prev_init.  Ring: 3 slots, the later call starts from slot 0 as
    bench.py's chunks do.  Trajectory: the later call writes on behind the first."""
    dt = torch.float64
    h.set_option("overlap", overlap)
    ctl = torch.as_tensor(np.ascontiguousarray(ctl), device=DEV).to(dt)
    B, T = ctl.shape[0], ctl.shape[1]
    K = 0 if first is None else first.shape[1]
    st = h.new_state(B, dt, n_slots=3 if ring else K + T + 1)
    h.init_straight(st[0])
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    prev, base = None, st
    if first is not None:
        h.simulate(torch.as_tensor(np.ascontiguousarray(first), device=DEV).to(dt), st, G, ring=ring)
        if ring:
            newest, prev = st[K % 3].clone(), st[(K - 1) % 3].clone()
            st[0].copy_(newest)
        else:
            prev, base = st[K - 1], st[K:]
    tip = torch.empty((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    h.simulate(ctl, base, G, ring=ring, tip=tip, status=status, maxit=maxit, prev_init=prev)
    torch.cuda.synchronize()
    assert_kernel(h, overlap)
    states = base.cpu().numpy()
    last3 = np.stack([states[k % 3 if ring else k] for k in (T - 2, T - 1, T)])
    return dict(tip=tip.cpu().numpy(), status=status.cpu().numpy(), G=G.cpu().numpy(), last3=last3)


def same_bits(a, b, what):
    """tips, status and the last three states, bit for bit (a NaN equals a NaN: a sick rod's tips)"""
    assert np.array_equal(a["status"], b["status"]), what
    assert np.array_equal(a["tip"], b["tip"], equal_nan=True), what
    assert np.array_equal(a["last3"], b["last3"], equal_nan=True), what


@pytest.mark.parametrize("N", GRIDS)
def test_ring_equals_trajectory(torch_cuda, monkeypatch, N):
    """T = 9: lean steps on every ring slot; nothing a lean step leaves out of HBM changes a result."""
    set_mode_env(monkeypatch, "overlap")
    _, h = _handle(N)
    ctl = sine_ctl(9, 9, 310 + N)
    ring = run(torch_cuda, h, ctl, 1, ring=True)
    full = run(torch_cuda, h, ctl, 1, ring=False)
    assert np.all(full["status"] == 0)
    same_bits(ring, full, N)
    assert float(np.abs(ring["last3"][..., 25:]).max()) == 0.0  # padding slots


ROLL_BACK = ([("step", 33), ("step", 65)] + [("random", N) for N in GRIDS] + [("random18", N) for N in GRIDS])


@pytest.mark.parametrize("kind,N", ROLL_BACK)
def test_roll_back_from_the_park(torch_cuda, monkeypatch, kind, N):
    """Rough inputs on a ring: verifications are rejected inside the lean range (the tile comes back from the park) and,
    under the iteration cap of 3, rods that run into the cap are handed over there (the two tiles are flushed for the
    take-over kernel).  The ring call equals the trajectory call bit for bit, and both stay within test_gpu_overlap.py's
    bounds of the plain persistent kernel (overlap = 0) with the same cap: the same steps unconverged, and tips and
    states to 1e-6 where rods are taken over at the cap (test_hand_over_to_second_launch), to 1e-7 with the default cap
    (test_rough_inputs_full_trajectory).  The counts of the module docstring say what each case rolls back."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    _, h = _handle(N)
    cap = 0 if kind == "random18" else 3
    ctl = rough_ctl("random", B_ROUGH, 18) if kind == "random18" else rough_ctl(kind)
    ring = run(torch, h, ctl, 1, ring=True, maxit=cap)
    full = run(torch, h, ctl, 1, ring=False, maxit=cap)
    same_bits(ring, full, (kind, N))
    plain = run(torch, h, ctl, 0, ring=True, maxit=cap)
    print(f"  unconverged rod-steps: {int((ring['status'] != 0).sum())} / {int((plain['status'] != 0).sum())}")
    assert np.all(ring["status"] >= 0) and np.all(ring["status"] <= 2)
    assert np.array_equal(ring["status"] != 0, plain["status"] != 0)
    tol = 1e-6 if cap else 1e-7
    if not cap:
        assert np.all(plain["status"] == 0)
    for name, a in (("ring", ring), ("trajectory", full)):
        assert np.all(np.isfinite(a["tip"]))
        e_tip = rel_l2(a["tip"], plain["tip"])
        e_st = max(rel_l2(a["last3"][k][..., :25], plain["last3"][k][..., :25]) for k in range(3))
        print(f"  {name}: tips {e_tip:.2e}, last three states {e_st:.2e} (bound {tol:.0e})")
        assert e_tip < tol and e_st < tol, name


def _sick_pair(torch, h, N, t0, first):
    B, T, s = 9, 12, 5  # (rod 5: the second workgroup, beside healthy rods on the same CU)
    clean = dict(ctl=sine_ctl(B, T, 330 + N))
    sick = sc.sick_twin(clean, "nan_ctl", s, t0)
    assert sc.differing_entries(clean, sick) == [("ctl", (s, t0, 1))]
    lead = None if not first else sine_ctl(B, first, 350 + N)
    ring = run(torch, h, sick["ctl"], 1, ring=True, first=lead)
    full = run(torch, h, sick["ctl"], 1, ring=False, first=lead)
    healthy = np.arange(B) != s
    assert np.all(full["status"][healthy] == 0) and np.all(full["status"][s, :t0] == 0)
    assert np.all(full["status"][s, t0:] != 0)  # given up at t0, and the NaN stays in the rod's states
    assert np.all(np.isfinite(full["tip"][healthy])) and np.all(np.isfinite(full["tip"][s, :t0]))
    same_bits(ring, full, (N, t0))


@pytest.mark.parametrize("N", GRIDS)
def test_take_over_inside_the_lean_range(torch_cuda, monkeypatch, N):
    """A rod with a NaN tension at step 6 of 12 beside eight healthy ones, on a ring: it gives up in the middle of the
    lean range and flushes the leading slots of levels 6 and 5, the others finish."""
    set_mode_env(monkeypatch, "overlap")
    _sick_pair(torch_cuda, _handle(N)[1], N, 6, 0)


@pytest.mark.parametrize("N", GRIDS)
def test_take_over_at_step_0_with_prev_init(torch_cuda, monkeypatch, N):
    """The same rod sick at step 0 of a call that continues a four-step call (prev_init set): it flushes level 0 alone;
    prev_init is the caller's and is not written."""
    set_mode_env(monkeypatch, "overlap")
    _sick_pair(torch_cuda, _handle(N)[1], N, 0, 4)


def chained(torch, h, ctl, chunks, overlap=1, maxit=0):
    """the trajectory in several calls on ONE 3-slot ring with a kept predictor, handed from call to call the way
    bench.py does it: every call starts from slot 0, the state before it comes in as prev_init"""
    dt = torch.float64
    h.set_option("overlap", overlap)
    h.set_option("keep_predictor", 0)
    h.set_option("keep_predictor", 1)
    try:
        ctl = torch.as_tensor(np.ascontiguousarray(ctl), device=DEV).to(dt)
        B = ctl.shape[0]
        st = h.new_state(B, dt, n_slots=3)
        h.init_straight(st[0])
        G = torch.zeros((B, 6), dtype=dt, device=DEV)
        tips, stats, prev, t0 = [], [], None, 0
        for K in chunks:
            tip = torch.empty((B, K, 3), dtype=dt, device=DEV)
            status = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + K].contiguous(), st, G, ring=True, tip=tip, status=status, prev_init=prev, maxit=maxit)
            assert_kernel(h, overlap)
            last3 = torch.stack([st[k % 3] for k in (K - 2, K - 1, K)]).clone()
            prev = last3[1].clone()
            st[0].copy_(last3[2])
            tips.append(tip)
            stats.append(status)
            t0 += K
        torch.cuda.synchronize()
    finally:
        h.set_option("keep_predictor", 0)
    return dict(tip=torch.cat(tips, 1).cpu().numpy(), status=torch.cat(stats, 1).cpu().numpy(), G=G.cpu().numpy(),
                last3=last3.cpu().numpy())


@pytest.mark.parametrize("N", GRIDS)
def test_chained_calls_on_a_kept_predictor(torch_cuda, monkeypatch, N):
    """Three ring calls of six steps under the random inputs equal one ring call of 18 bit for bit: a roll-back next to
    a call boundary finds in the park what the call's rebuild loaded from prev_init and slot 0."""
    set_mode_env(monkeypatch, "overlap")
    _, h = _handle(N)
    ctl = rough_ctl("random", B_ROUGH, 18)
    three = chained(torch_cuda, h, ctl, [6, 6, 6])
    one = chained(torch_cuda, h, ctl, [18])
    same_bits(three, one, N)
    assert np.array_equal(three["G"], one["G"])
