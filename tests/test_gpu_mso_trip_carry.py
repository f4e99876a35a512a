"""GPU tests (``-m gpu``) of what a trip of the overlapped persistent kernel's merged sweep hands to the next one
(kr_mso_impl.hpp, ``trip()``): the two tile reads of the next grid point, which the fp64 kernels hold as 16-byte tuples
and consume behind ONE wait each, and - in builds with ``-DKR_MSO_TRIP_CARRY=1`` - the scale 2 / h.h of the rotation,
formed behind the Euler update from the state the next evaluation sees and carried in a register.  A moved wait or a
sunk read shows as a record formed from another grid point's leading slots; a carried value can go stale where a trip
does not advance a lane (``dsl = 0`` in a predicated trip), where the sweep changes its form (predicated -> full pair ->
odd remainder -> predicated) and where a sweep is thrown away and restarted.  Hence the grids:

    N = 9        intervals of 2: one full trip, the odd-remainder one
    N = 10..12   one, two, three intervals one segment longer: lanes leave their interval in different trailing trips
    N = 13       exactly one pair of full trips
    N = 17       a pair and the remainder trip
    N = 101      the LDS limit of the fp64 kernel

The yardstick is the plain persistent kernel (overlap = 0) with the bounds of test_gpu_mso_update_tail.py (1e-8 fp64,
2e-5 fp32); where the same kernel runs twice the results must be equal bit for bit.  Inputs and helpers are those of
test_gpu_mso_small.py."""
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


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


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


def _close(a, b, dtype, label):
    """overlap = 1 (a) against overlap = 0 (b), full trajectories: equal status, tips within the bound per rod, and every
    slot of EVERY stored record within the same bound relative to the largest entry (the form of
    test_gpu_mso_small.py's bound on a call's final state, here on all of them)"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    B = a["tip"].shape[0]
    assert np.array_equal(a["status"], b["status"]), (label, a["status"].tolist(), b["status"].tolist())
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B, -1), axis=1)
    pa, pb = a["states"][..., 12:15], b["states"][..., 12:15]
    perr = np.abs(pa - pb).max() / np.abs(pb).max()
    rerr = np.abs(a["states"] - b["states"]).max() / np.abs(b["states"]).max()
    print(f"  {label}: tip err {err.max():.2e}, positions of all records {perr:.2e}, all records {rerr:.2e} (bound {tol:.0e})")
    assert np.all(np.isfinite(a["states"])), label
    assert err.max() < tol, label
    assert perr < tol, label
    assert rerr < tol, label


def _ctl(torch, r, N, dt):
    return torch.as_tensor(_sine(B_SMALL, T_SHORT, r.del_t, 40 + N), device=DEV).to(dt).contiguous()


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_form_of_the_sweep(torch_cuda, monkeypatch, N, dtype):
    """Six steps as a full trajectory against the plain persistent kernel: status, tips and every stored record."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    _close(_run(torch, h, ctl, dt, 1), _run(torch, h, ctl, dt, 0), dtype, f"N={N} {dtype}")


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chord_verdict_on_every_step(torch_cuda, monkeypatch, N, dtype):
    """``residual_test = 0``: no verifying sweep is accepted from its residual alone, every verdict takes the chord path
    and a rejected sweep is restarted from its start state.  Every step
    converges on the sine inputs; same bounds against the plain kernel with the same option."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
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
    a ring ends with.  A parameter table of identical rows (the table twin of the kernel) against the plain call, and
    the same call a second time: every output.  All bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    T = T_SHORT
    full = _run(torch, h, ctl, dt, 1)
    ring = _run(torch, h, ctl, dt, 1, ring=True)
    with h.param_table([r._params()] * B_SMALL) as tab:
        tabd = _run(torch, h, ctl, dt, 1, table=tab)
    again = _run(torch, h, ctl, dt, 1)
    assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(ring["states"][k % 3], full["states"][k]), k
    for key in ("status", "tip", "G", "states"):
        assert np.array_equal(full[key], tabd[key]), ("table", key)
        assert np.array_equal(full[key], again[key]), ("again", key)


@pytest.mark.parametrize("kind", ["step", "random"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rejected_sweeps_and_hand_over(torch_cuda, monkeypatch, kind, dtype):
    """The "step" and "random" inputs of test_gpu_mso_small.py::test_rough_inputs at N = 12 with an iteration cap of 3 on
    a 3-slot ring: verifying sweeps are rejected and verified again, steps roll back to plain sweeps, run into the cap
    and are handed to the take-over kernel.  Status equal to the plain kernel's with the same cap."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, 12)
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
    a = _run(torch, h, ctl_t, dt, 1, ring=True, maxit=3)
    b = _run(torch, h, ctl_t, dt, 0, ring=True, maxit=3)
    print(f"  {kind} {dtype}: steps not converged {int((a['status'] != 0).sum())} of {B * T}")
    assert np.all((a["status"] >= 0) & (a["status"] <= 2))
    assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("N", [13, 17, 101])
def test_kept_predictor_across_calls(torch_cuda, monkeypatch, N):
    """Three ring calls of seven steps with keep_predictor = 1 (the predictor image goes through HBM, bench.py's way of
    calling) against one call of 21: equal status; tips and last state within 1e-7 (the bound of
    test_gpu_mso_small.py::test_kept_predictor_across_calls: the start values of a call's first steps differ)."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    r = make_robot(None, N)
    h = r._native()
    ctl = torch.as_tensor(_sine(B_SMALL, 21, r.del_t, 60 + N), device=DEV).contiguous()
    one = _run(torch, h, ctl, torch.float64, 1, ring=True)
    h.set_option("keep_predictor", 0)
    h.set_option("keep_predictor", 1)
    try:
        ch = _ring_calls(torch, h, ctl, torch.float64, [7, 7, 7])
    finally:
        h.set_option("keep_predictor", 0)
    assert np.array_equal(ch["status"], one["status"])
    e_tip, e_st = rel_l2(ch["tip"], one["tip"]), rel_l2(ch["last"][..., :25], one["states"][21 % 3][..., :25])
    print(f"  N={N}: tips {e_tip:.2e}, last state {e_st:.2e} (bound 1e-7)")
    assert e_tip < 1e-7 and e_st < 1e-7


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sick_rod_beside_healthy_ones(torch_cuda, monkeypatch, dtype):
    """One rod of five (N = 12) with a NaN tension from step 2 on: that rod reports 2 from that step (what
    test_gpu_sick_rod.py expects of this kernel), the other four are equal to the clean call bit for bit."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    N, s, t0 = 12, 2, 2
    r = make_robot(None, N)
    h = r._native()
    clean_np = np.array(_sine(B_SMALL, T_SHORT, r.del_t, 40 + N))
    sick_np = clean_np.copy()
    sick_np[s, t0:, 1] = np.nan
    clean = _run(torch, h, torch.as_tensor(clean_np, device=DEV).to(dt).contiguous(), dt, 1)
    sick = _run(torch, h, torch.as_tensor(sick_np, device=DEV).to(dt).contiguous(), dt, 1)
    assert np.all(clean["status"] == 0), clean["status"].tolist()
    got = sick["status"][s]
    print(f"  {dtype}: sick rod status {got.tolist()}")
    assert np.all(got[:t0] == 0) and np.all(got[t0:] == 2), got.tolist()
    healthy = np.arange(B_SMALL) != s
    for key in ("status", "tip", "G"):
        assert np.array_equal(sick[key][healthy], clean[key][healthy]), key
    assert np.array_equal(sick["states"][:, healthy], clean["states"][:, healthy])
    assert np.array_equal(sick["tip"][s, :t0], clean["tip"][s, :t0])
