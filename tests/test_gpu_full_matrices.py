"""Full, asymmetric material matrices on every step kernel that serves them (``-m gpu``, through the C ABI).

``fill_consts`` (kr_api.hip) clears ``RodConst::diag`` when ``Bse``, ``Bbt`` or an inverse of ``Kse + c0 Bse`` /
``Kbt + c0 Bbt`` has an off-diagonal entry; every step-kernel family but the overlapped ones is compiled a second time for
such rods (``DIAG = false``: ``matvec`` for ``diagvec`` in ``ode_eval``, the full branches of ``hist_derive`` /
``hist_derive_cold`` / ``hist_lean``), and the plan (kr_plan.hip) moves the rod off the overlapped kernels and off the
persistent MLP kernels.  Here each of those instantiations computes the parameter set "full-asym"
(tests/full_matrix_cases.py: the None preset with the asymmetric, large ``Bse`` / ``Bbt`` of ode_derivative_cases.FULL) and
is compared with

  * the unmodified reference (tests/golden/full_matrices.npz), rod 0, where the fixture holds the grid;
  * the C oracle, every rod (B = 5: rod b runs rod 0's controls scaled by 1 + 0.01 b; B = 9 on K2a, where eight rods
    share a wavefront and the ninth starts a second one);
  * with the MLP on, the NumPy oracle, the only oracle with a network.

Bounds.  fp64 (``tol = 1e-12``, so that the arithmetic is measured and not the stopping rule): tips 1e-8, stored states
1e-7 PER BLOCK p h n m q w v u - one norm over the record would hide ``Bse``, which lives in n, m, q, w at 2e-6 .. 6e-6 -
and every status 0.  fp32: tips 1e-5, stored states 1e-4 per block.  An fp32 run holds ``Bbt`` and NOT its companion
``Bse``: tests/test_full_matrices_cpu.py proves both, by running the oracle on the four mutants of the set
(``test_mutants_are_seen``: each is at least ten bounds away in fp64, the ``Bbt`` ones in fp32, the ``Bse`` ones provably
below the fp32 bound with the network off).

The control.  Every case runs a second time with the diagonal twin (the diagonals of both matrices only) through the
``DIAG = true`` instantiation of the same kernel, under the same bounds: a bound the twin cannot meet would be a wrong
bound, not a finding.  Every call asserts the kernel that ran: ``(last_sim_path, last_waves_per_rod, last_overlap)``;
for the twin that is the overlapped kernel where the full set falls back from one.

Consistency that needs no oracle: the tips of a 3-slot ring call and of the driver's form (ring calls of 5 steps with
``keep_predictor`` and ``prev_init`` in the ring) are bit-identical to the full-trajectory call's - on every kernel that
serves full matrices; the twin's driver calls on an overlapped kernel are held to the tip bound instead, see
``test_step_kernels`` - and on K2b and K2c rod b's result is bit-identical to that of its own B = 1 call.

Scope: Euler sweeps.  RK4 sweeps, with full and with diagonal matrices, are held by tests/test_gpu_rk4_sweeps.py, which
runs them through ``run`` and ``check`` below.  Measured errors: LABBOOK.md (full material
matrices)."""
import numpy as np
import pytest

import full_matrix_cases as fm
import ode_derivative_cases as dc
from conftest import rel_l2
from gpu_helpers import inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 5  # steps per call of the driver's form: T = 16 makes four calls, the last of one step

# kernel -> (mode of gpu_helpers.set_mode_env, waves_per_rod, handle options,
#            (path, waves per rod, overlap) that must have run with "full-asym", the same with the diagonal twin)
KERNELS = {
    "K2a": ("single", 1, {}, (0, 1, 0), (0, 1, 0)),
    "K2b": ("multi", 1, {}, (1, 1, 0), (1, 1, 0)),
    "K2c": ("persistent", 1, {}, (2, 1, 0), (2, 1, 0)),
    "K2c-fallback": ("overlap", 1, {"overlap": 1}, (2, 1, 0), (2, 1, 1)),       # (the twin: K2e)
    "K2d-step-W2": ("multi", 2, {}, (1, 2, 0), (1, 2, 0)),
    "K2d-step-W4": ("multi", 4, {}, (1, 4, 0), (1, 4, 0)),
    "msw-W2": ("persistent", 2, {}, (2, 2, 0), (2, 2, 1)),                      # msw_overlap left at 1 (the twin: K2f)
    "msw-W4": ("persistent", 4, {}, (2, 4, 0), (2, 4, 1)),
    # MLP on.  Matrix-core network, default modes: full matrices take one launch per step, the twin stays persistent
    "mlp-default": ("overlap", 0, {}, (1, 1, 0), (2, 1, 0)),
    "mlp-single": ("single", 1, {}, (0, 1, 0), (0, 1, 0)),                      # incl. the history network
}
FULL, ALL = ("full",), ("full", "ring", "driver")
# (kernel, N, T, controls, rods, call forms); every (N, T, controls) is one of fm.SIM_CASES
ROWS = [
    ("K2a", 12, 16, "sine", 9, FULL), ("K2a", 40, 16, "sine", 9, FULL), ("K2a", 40, 16, "jump", 9, FULL),
    ("K2a", 400, 5, "sine", 9, FULL),  # history in the global workspace (hist_kernel)
    ("K2b", 9, 16, "sine", 5, FULL), ("K2b", 40, 16, "sine", 5, FULL), ("K2b", 40, 16, "jump", 5, FULL),
    ("K2b", 131, 6, "sine", 5, FULL),
    ("K2c", 9, 16, "sine", 5, ALL), ("K2c", 40, 16, "sine", 5, ALL), ("K2c", 40, 16, "jump", 5, ALL),
    ("K2c", 112, 6, "sine", 5, ALL),  # the upper edge of K2c in fp64: four rods' histories of 30 N + 1760 doubles in 160 KiB
    ("K2c", 128, 6, "sine", 5, ALL),  # the upper edge of one_wave_range; fp32 only, see F32_ONLY
    ("K2c-fallback", 40, 16, "sine", 5, ("full", "ring")),
    ("K2d-step-W2", 27, 16, "sine", 5, FULL), ("K2d-step-W2", 131, 6, "sine", 5, FULL), ("K2d-step-W2", 400, 5, "sine", 5, FULL),
    ("K2d-step-W4", 27, 16, "sine", 5, FULL), ("K2d-step-W4", 131, 6, "sine", 5, FULL), ("K2d-step-W4", 400, 5, "sine", 5, FULL),
    ("msw-W2", 60, 16, "sine", 5, ALL), ("msw-W2", 100, 8, "sine", 5, ALL), ("msw-W2", 400, 5, "sine", 5, ("full", "ring")),
    ("msw-W4", 60, 16, "sine", 5, ALL), ("msw-W4", 100, 8, "sine", 5, ALL), ("msw-W4", 400, 5, "sine", 5, ("full", "ring")),
]
assert all(r[1:4] in fm.SIM_CASES for r in ROWS)
# In fp64 the LDS history of a rod of more than 112 points does not fit four to a workgroup (ms_lds_bytes, kr_ms_impl.hpp),
# and the plan gives such a rod one launch per step - K2b, which has its own rows - with either set of matrices.
F32_ONLY = {("K2c", 128)}
ROW_PARAMS = [pytest.param(*r, dt, id=f"{r[0]}-N{r[1]}-{r[3]}-{dt}") for r in ROWS for dt in ("f64", "f32")
              if dt == "f32" or (r[0], r[1]) not in F32_ONLY]
NN_ROWS = [("mlp-default", "elu64"), ("mlp-default", "elu6464"), ("mlp-single", "elu64"), ("mlp-single", "hist64")]
B1_KERNELS = ("K2b", "K2c")  # rod b against its own B = 1 call
VARIANTS = ("full-asym", "twin")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _handle(monkeypatch, kernel, N, variant, net=None):
    mode, W, options = KERNELS[kernel][:3]
    set_mode_env(monkeypatch, mode, waves_per_rod=W)
    r = fm.apply_to_rod(make_robot(None, N), variant)
    if net is not None:
        inject(r, fm.network(net))
    h = r._native()
    for k, v in options.items():
        h.set_option(k, v)
    return h


def run(torch, h, ctl_np, form, dtype, ran, use_nn=False, scheme=0):
    """One run of ctl[B, T, 4] from the straight rod -> (tips [B, T, 3], status [B, T], {entry: states [B, 25, N]} of
    every entry the form leaves behind: all of them, or T - 2 .. T of a ring); asserts the kernel after every call.
    ``scheme``: KR_EULER (0) or KR_RK4 of every sweep."""
    B, T = ctl_np.shape[:2]
    dt = torch.float64 if dtype == "f64" else torch.float32
    tol = 1e-12 if dtype == "f64" else 0.0
    ctl = torch.as_tensor(np.ascontiguousarray(ctl_np), device=DEV).to(dt).contiguous()

    def check_kernel():
        got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
        assert got == ran, f"(path, waves per rod, overlap) = {got}, the test is meant to exercise {ran}"

    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), float("nan"), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    st = h.new_state(B, dt, n_slots=T + 1 if form == "full" else 3)
    h.init_straight(st[0])
    try:
        if form != "driver":
            h.simulate(ctl, st, G, ring=form == "ring", tip=tip, status=status, tol=tol, use_nn=use_nn, scheme=scheme)
            torch.cuda.synchronize()
            check_kernel()
            slot = (lambda e: e) if form == "full" else (lambda e: e % 3)
        else:
            h.set_option("keep_predictor", 0)  # (drops a stored image)
            h.set_option("keep_predictor", 1)
            prev, a = None, 0
            while a < T:
                n = min(CHUNK, T - a)
                tp = torch.full((B, n, 3), float("nan"), dtype=dt, device=DEV)
                sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
                h.simulate(ctl[:, a:a + n].contiguous(), st, G, ring=True, tip=tp, status=sx, prev_init=prev, tol=tol,
                           use_nn=use_nn, scheme=scheme)
                torch.cuda.synchronize()
                check_kernel()
                tip[:, a:a + n], status[:, a:a + n] = tp, sx
                a += n
                if a < T:
                    # the call left the newest state in slot n % 3 and the one before it in slot (n - 1) % 3; the next call
                    # starts from slot 0 again, with the older state in slot 2 of the ring itself (knode_rod.h: prev_init
                    # may point into the ring)
                    newest, older = st[n % 3].clone(), st[(n - 1) % 3].clone()
                    st[0].copy_(newest)
                    st[2].copy_(older)
                    prev = st[2]
            slot = lambda e: (e - (T - n)) % 3
        stored = {}
        for e in (range(1, T + 1) if form == "full" else range(max(1, T - 2), T + 1)):
            y, z = h.unpack(st[slot(e)])
            stored[e] = torch.cat([y, z], dim=1).double().cpu().numpy()
    finally:
        h.set_option("keep_predictor", 0)
    return tip.double().cpu().numpy(), status.cpu().numpy(), stored


def check(label, dtype, tips, status, stored, ref_tips, ref_states, fixture=None):
    """The bounds of the module docstring on every rod against the oracle's ``ref_tips[B, T + 1, 3]`` /
    ``ref_states[B, T + 1, 25, N]``, and on rod 0 against the reference's run; prints every figure before it asserts."""
    tip_tol, state_tol = fm.TOL[dtype]
    B, T = tips.shape[:2]
    entries = sorted(stored)
    lines = []
    for b in range(B):
        te = fm.tip_error(tips[b], ref_tips[b, 1:])
        be = fm.block_errors(np.array([stored[e][b] for e in entries]), ref_states[b][entries])
        lines.append((f"rod {b}", te, be))
    if fixture is not None:  # the reference drops its last solve: entries 0 .. T - 1, a kernel's tip[t] is entry t + 1
        te = fm.tip_error(tips[0, :T - 1], fixture["tips"][1:])
        both = [e for e in entries if e in fixture["states"]]
        assert both, (entries, sorted(fixture["states"]))
        be = fm.block_errors(np.array([stored[e][0] for e in both]), np.array([fixture["states"][e] for e in both]))
        lines.append(("rod 0 / reference", te, be))
    for who, te, be in lines:
        print(f"{label} {who}: tips {te:.1e} | {fm.fmt_blocks(be)}")
    bad = np.argwhere(status != 0)
    assert bad.size == 0, f"{label}: status {status[status != 0].tolist()[:8]} at (rod, step) {bad.tolist()[:8]}"
    assert np.all(np.isfinite(tips))
    for who, te, be in lines:
        assert te < tip_tol, f"{label} {who}: tips {te:.2e}"
        over = {k: v for k, v in be.items() if not v < state_tol}
        assert not over, f"{label} {who}: blocks over {state_tol:g}: {over}"


def _answers(oracle, N, T, kind, variant, B, **kw):
    ref_tips, ref_states = oracle(N, T, kind, variant, B=B, **kw)
    fixture = fm.fixture_run(N, kind) if variant == "full-asym" and not kw else None
    assert fixture is None or fixture["T"] == T
    return ref_tips, ref_states, fixture


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kernel,N,T,kind,B,forms,dtype", ROW_PARAMS)
def test_step_kernels(torch_cuda, monkeypatch, kernel, N, T, kind, B, forms, dtype, variant):
    torch = torch_cuda
    ran = KERNELS[kernel][3 if variant == "full-asym" else 4]
    h = _handle(monkeypatch, kernel, N, variant)
    ctl = fm.batch_controls(T, kind, B)
    ref_tips, ref_states, fixture = _answers(fm.oracle_run, N, T, kind, variant, B)
    full_tips = None
    for form in forms:
        tips, status, stored = run(torch, h, ctl, form, dtype, ran)
        check(f"{kernel} N={N} {kind} {form} {dtype} {variant}", dtype, tips, status, stored, ref_tips, ref_states, fixture)
        if form == "full":
            full_tips, full_stored = tips, stored
        else:
            d = float(np.max(np.abs(tips - full_tips)))
            print(f"{kernel} N={N} {form} {dtype} {variant}: tips differ from the full call's by at most {d:.1e}")
            if form == "driver" and ran[2]:
                # The twin on an overlapped kernel: the verifying sweep of a step rides on the next step's Jacobian sweep,
                # and the last step of a call has no next step - where a call ends changes the sweeps a step takes.  Both
                # calls accept roots of the same step inside the stopping tolerance; held to the tip bound (measured: fp32
                # 1.2e-7 .. 3.0e-7 absolute on K2f, fp64 equal).
                assert fm.tip_error(tips, full_tips) < fm.TOL[dtype][0]
            else:  # the same kernel, the same arithmetic: the same bits
                assert np.array_equal(tips, full_tips), f"{form}: tips differ from the full call's by up to {d:.2e}"
    if kernel in B1_KERNELS:
        for b in range(B):
            t1, s1, st1 = run(torch, h, ctl[b:b + 1], "full", dtype, ran)
            assert np.array_equal(t1[0], full_tips[b]), f"rod {b}: tips depend on the batch"
            assert np.array_equal(st1[T][0], full_stored[T][b]), f"rod {b}: last state depends on the batch"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,net", NN_ROWS)
def test_step_kernels_with_the_mlp_on(torch_cuda, monkeypatch, kernel, net, dtype, variant):
    """The network in every sweep: with full matrices the plan leaves the persistent MLP kernels for one launch per step
    (kr_ms_impl.hpp with the matrix-core evaluator); single shooting also serves the network with history inputs."""
    N, T, kind = fm.NN_CASE
    B = 5
    ran = KERNELS[kernel][3 if variant == "full-asym" else 4]
    h = _handle(monkeypatch, kernel, N, variant, net=net)
    ref_tips, ref_states, _ = _answers(fm.numpy_oracle_run, N, T, kind, variant, B, net=net)
    tips, status, stored = run(torch_cuda, h, fm.batch_controls(T, kind, B), "full", dtype, ran, use_nn=True)
    check(f"{kernel} {net} N={N} {dtype} {variant}", dtype, tips, status, stored, ref_tips, ref_states)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode,W", [("single", 1), ("multi", 1), ("multi", 2)])
def test_step_batch(torch_cuda, monkeypatch, mode, W, dtype, variant):
    """kr_step_batch: one step from entries 7, 8 of the oracle's N = 40 run (pinned to the reference's by
    test_full_matrices_cpu.py) against the oracle's own step from the same two states."""
    torch = torch_cuda
    B = 5
    N = fm.STEP_CASE[0]
    prev, cur, tens, nxt = fm.step_case(variant, B)
    set_mode_env(monkeypatch, mode, waves_per_rod=W)
    h = fm.apply_to_rod(make_robot(None, N), variant)._native()
    dt = torch.float64 if dtype == "f64" else torch.float32
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()
    s_prev, s_cur = (h.pack(t(s[:, :19]), t(s[:, 19:])) for s in (prev, cur))
    s_next = h.new_state(B, dt)
    G = t(cur[:, 7:13, 0])  # start values: n, m at the base of the state before (what a time loop carries over)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    h.step(s_prev, s_cur, s_next, G, t(tens), tol=1e-12 if dtype == "f64" else 0.0, status=status)
    torch.cuda.synchronize()
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"))
    assert got == ((0, 1) if mode == "single" else (1, W)), got
    assert int((status != 0).sum()) == 0, status
    y, z = h.unpack(s_next)
    out = torch.cat([y, z], dim=1).double().cpu().numpy()
    state_tol = fm.TOL[dtype][1]
    for b in range(B):
        be = fm.block_errors(out[b], nxt[b])
        print(f"step {mode} W={W} {dtype} {variant} rod {b}: {fm.fmt_blocks(be)}")
    for b in range(B):
        be = fm.block_errors(out[b], nxt[b])
        assert all(v < state_tol for v in be.values()), (b, be)


# ---------------------------------------------------------------------------
# the kernels below the step kernels: kr_ode_batch, kr_residual_batch (Euler)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ode_batch(torch_cuda, variant, dtype):
    """kr_ode_batch on the four rows of ode_derivative_cases.py (two physical, two with every component O(1)) against
    ``cosserat_oracle.ode``.  fp64: the bounds of test_gpu_forward.py::test_ode_batch_presets_f64.  fp32: those of
    ::test_ode_batch_f32_vs_torch_twin, against the fp64 oracle at the kernel's own (rounded) inputs."""
    torch = torch_cuda
    import cosserat_oracle as orc
    dt = torch.float64 if dtype == "f64" else torch.float32
    y, yh, zh, tf = dc.rows()
    if dtype == "f32":
        y, yh, zh, tf = (np.asarray(a, np.float32).astype(np.float64) for a in (y, yh, zh, tf))
    h = fm.apply_to_rod(make_robot(None, 10), variant)._native()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()
    dys, z = h.ode_batch(t(y), t(yh), t(zh), t(tf))
    got = torch.cat([dys, z], 1).double().cpu().numpy()
    D = fm.rod_params(10, variant).derived()
    ref = np.array([np.concatenate(orc.ode(D, y[i], yh[i], zh[i], tf[i])) for i in range(len(y))])
    e_l2 = rel_l2(got, ref)
    if dtype == "f64":
        e_max = float(np.max(np.abs(got - ref) / (np.abs(ref) + 1e-9 * np.abs(ref).max())))
        print(f"ode_batch {dtype} {variant}: rel L2 {e_l2:.1e}, entry-wise {e_max:.1e}")
        assert e_l2 < 1e-13 and e_max < 1e-8
    else:
        e_max = float(np.max(np.abs(got - ref) / np.abs(ref).max(axis=0, keepdims=True)))
        print(f"ode_batch {dtype} {variant}: rel L2 {e_l2:.1e}, per column scale {e_max:.1e}")
        assert e_l2 < 2e-6 and e_max < 5e-5


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residual_batch(torch_cuda, variant, dtype):
    """kr_residual_batch (Euler) at entries 7, 8 of the N = 40 run, from the root's G and from two G away from it, against
    ``cosserat_oracle.residual_euler``: the swept state and the 6-vector.  fp64: the bounds of
    test_gpu_forward.py::test_residual_methods.  fp32 (no bound of the project's): the oracle sweeps the kernel's own
    rounded inputs; a sweep is N - 1 dependent Euler steps whose roundings add up to N u = 2.4e-6 at N = 40 (u = 6e-8),
    held to four times that, 1e-5, on y and z, and the 6-vector to ten times 1e-5 of the largest n, m."""
    torch = torch_cuda
    import cosserat_oracle as orc
    B = 3
    N = fm.STEP_CASE[0]
    prev, cur, tens, nxt = fm.step_case(variant, B)
    dt = torch.float64 if dtype == "f64" else torch.float32
    rnd = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: np.asarray(a, np.float64))
    G = np.array([nxt[b][7:13, 0] * s for b, s in zip(range(B), (1.0, 1.05, 0.9))])
    prev, cur, tens, G = rnd(prev), rnd(cur), rnd(tens), rnd(G)
    h = fm.apply_to_rod(make_robot(None, N), variant)._native()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()
    s_prev, s_cur = (h.pack(t(s[:, :19]), t(s[:, 19:])) for s in (prev, cur))
    s_next = s_cur.clone()
    res = h.residual(t(G), s_prev, s_cur, s_next, t(tens)).double().cpu().numpy()
    y, z = h.unpack(s_next)
    y, z = y.double().cpu().numpy(), z.double().cpu().numpy()
    D = fm.rod_params(N, variant).derived()
    tol_s, rtol, atol = (1e-10, 1e-8, 1e-10) if dtype == "f64" else (1e-5, 0.0, 1e-4)
    for b in range(B):
        ry, rz = cur[b, :19].copy(), cur[b, 19:].copy()
        yh, zh = D.c1 * cur[b, :19] + D.c2 * prev[b, :19], D.c1 * cur[b, 19:] + D.c2 * prev[b, 19:]
        rr = orc.residual_euler(D, G[b], ry, rz, yh, zh, tens[b])
        ey, ez = rel_l2(y[b], ry), rel_l2(z[b, :, :N - 1], rz[:, :N - 1])   # (column N - 1 of z is never written)
        scale = np.abs(ry[7:13]).max()
        print(f"residual {dtype} {variant} rod {b}: y {ey:.1e} z {ez:.1e} r {np.abs(res[b] - rr).max() / scale:.1e} of max |n, m|"
              f" (|r| {np.abs(rr).max():.1e})")
        assert ey < tol_s and ez < tol_s
        assert np.allclose(res[b], rr, rtol=rtol, atol=atol * scale)
