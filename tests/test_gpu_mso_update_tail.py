"""GPU tests (``-m gpu``) of the tail every update of the overlapped persistent kernel shares (kr_mso_impl.hpp,
``finish()`` / ``apply()`` with the quad sums in front of them): the p rows that move the positions of the interval
starts, the scaled update norm and the per-lane pieces of the update.  The tail reads its operands unconditionally and
selects on the values, so what is pinned here is that no lane picks up a neighbour's element: at every split of the
rod (interval lengths 2 and every remainder of (N - 1) / 4), in the Newton update and in the chord update of the
verdict (``residual_test = 0`` runs the latter on every step), on the rejection path that applies the chord update to
the verified step's unknowns, and beside a rod whose update is not finite.  The yardstick is the plain persistent
kernel (overlap = 0) with the bounds of test_gpu_overlap.py::test_bench_workload_vs_plain_persistent (1e-8 fp64,
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
GRIDS = [9, 10, 11, 12, 101]


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


def _close(a, b, dtype, label):
    """overlap = 1 (a) against overlap = 0 (b), full trajectories: equal status, tips within the bound per rod, and the
    position slots 12..14 of EVERY stored record within the same bound (the p rows move the positions of the interval
    starts, which no tip-only check of an interior interval sees)"""
    tol = 1e-8 if dtype == "f64" else 2e-5
    B = a["tip"].shape[0]
    assert np.array_equal(a["status"], b["status"]), (label, a["status"].tolist(), b["status"].tolist())
    err = np.linalg.norm((a["tip"] - b["tip"]).reshape(B, -1), axis=1) / np.linalg.norm(b["tip"].reshape(B, -1), axis=1)
    pa, pb = a["states"][..., 12:15], b["states"][..., 12:15]
    perr = np.abs(pa - pb).max() / np.abs(pb).max()
    print(f"  {label}: tip err {err.max():.2e}, positions of all records {perr:.2e} (bound {tol:.0e})")
    assert err.max() < tol, label
    assert perr < tol, label


def _ctl(torch, r, N, dt):
    return torch.as_tensor(_sine(B_SMALL, T_SHORT, r.del_t, 40 + N), device=DEV).to(dt).contiguous()


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_split_of_the_rod(torch_cuda, monkeypatch, N, dtype):
    """N = 9 has intervals of two segments; 10, 11, 12 have 1, 2, 3 intervals one segment longer; 101 is the longest
    fp64 grid with four rods per workgroup.  Six steps as a full trajectory."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    _close(_run(torch, h, ctl, dt, 1), _run(torch, h, ctl, dt, 0), dtype, f"N={N} {dtype}")


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_chord_tail_on_every_step(torch_cuda, monkeypatch, N, dtype):
    """``residual_test = 0``: no verifying sweep is accepted from its residual alone, so every verdict runs the chord
    update and its copy of the tail.  Every step converges on the sine inputs; same bounds against the plain kernel
    with the same option."""
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
        assert h.get_option("last_overlap") == 1
        b = _run(torch, h, ctl, dt, 0)
    finally:
        h.set_option("residual_test", 1)
    assert np.all(a["status"] == 0), a["status"].tolist()
    _close(a, b, dtype, f"N={N} {dtype} chord")


@pytest.mark.parametrize("kind", ["step", "random"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rejection_applies_the_chord_update(torch_cuda, monkeypatch, kind, dtype):
    """The "step" and "random" inputs of test_gpu_mso_small.py::test_rough_inputs at N = 12 with an iteration cap of 3 on
    a 3-slot ring: verifying sweeps are rejected and the chord update goes into the verified step's unknowns
    (``apply(XsB)``), steps run into the cap and are handed over.  Status equal to the plain kernel's with the same cap."""
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


@pytest.mark.parametrize("N", [9, 12, 101])
@pytest.mark.parametrize("chord", [0, 1])
def test_same_kernel_twice_is_bit_equal(torch_cuda, monkeypatch, N, chord):
    """Ring call against trajectory call (tips, status, the three complete states a ring ends with) and a parameter table
    of identical rows against the plain call: equal bit for bit, with the Newton tail alone and with the chord tail on
    every step."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    r = make_robot(None, N)
    h = r._native()
    ctl = _ctl(torch, r, N, dt)
    T = T_SHORT
    h.set_option("residual_test", 0 if chord else 1)
    try:
        full = _run(torch, h, ctl, dt, 1)
        ring = _run(torch, h, ctl, dt, 1, ring=True)
        with h.param_table([r._params()] * B_SMALL) as tab:
            tabd = _run(torch, h, ctl, dt, 1, table=tab)
    finally:
        h.set_option("residual_test", 1)
    assert np.array_equal(ring["tip"], full["tip"]) and np.array_equal(ring["status"], full["status"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(ring["states"][k % 3], full["states"][k]), k
    for key in ("status", "tip", "G", "states"):
        assert np.array_equal(full[key], tabd[key]), key


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sick_rod_beside_healthy_ones(torch_cuda, monkeypatch, dtype):
    """One rod of five (N = 12) with a NaN tension from step 2 on: that rod reports 2 from that step, the other four are
    equal to the clean call bit for bit - the unconditional reads of the tail stay inside the rod's own LDS, and a NaN
    in an element a lane does not own is dropped by a select, never multiplied by zero."""
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
    again = _run(torch, h, torch.as_tensor(clean_np, device=DEV).to(dt).contiguous(), dt, 1)
    assert np.all(clean["status"] == 0), clean["status"].tolist()
    got = sick["status"][s]
    print(f"  {dtype}: sick rod status {got.tolist()}")
    assert np.all(got[:t0] == 0) and np.all(got[t0:] == 2), got.tolist()
    healthy = np.arange(B_SMALL) != s
    for key in ("status", "tip", "G"):
        assert np.array_equal(sick[key][healthy], clean[key][healthy]), key
    assert np.array_equal(sick["states"][:, healthy], clean["states"][:, healthy])
    assert np.array_equal(sick["tip"][s, :t0], clean["tip"][s, :t0])
    for key in ("status", "tip", "G", "states"):
        assert np.array_equal(again[key], clean[key]), key
