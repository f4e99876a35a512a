"""RK4 sweeps (``scheme = KR_RK4``) on every step kernel that serves them (``-m gpu``, through the C ABI), over time steps.

Three kernel families carry an RK4 sweep: single shooting (K2a, kr_sim_impl.hpp; eight rods per wavefront, the history in
LDS or, for long rods, in the workspace; MLP off or on), multiple shooting with one launch per step
(K2b, kr_ms_impl.hpp; MLP off or on) and its persistent form (K2c; MLP off).  Each runs in fp64 and fp32 the parameter set
"full-asym" (``DIAG = false``) and its diagonal twin (``DIAG = true``; the control of every comparison) - never the None
preset, which the reference itself does not solve under RK4 on a coarse grid (tests/rk4_cases.py) - and is compared with

  * the unmodified reference under RK4 (tests/golden/rk4_sweeps.npz), rod 0, where the fixture holds the run;
  * the C oracle's RK4 sweep, every rod (B = 5: rod b runs rod 0's controls scaled by 1 + 0.01 b; B = 9 on K2a, where the
    ninth rod starts a second wavefront);
  * with the MLP on, the NumPy oracle (N = 12, three rods; the only oracle with a network).

``run`` and ``check`` are those of tests/test_gpu_full_matrices.py, and so are the bounds: fp64 (``tol = 1e-12``) tips 1e-8,
stored states 1e-7 per block p h n m q w v u; fp32 tips 1e-5, states 1e-4 per block; every status 0.  What these bounds
hold is proven by tests/test_rk4_sweeps_cpu.py::test_mutants_are_seen on seven wrong sweeps (histories of the wrong column
in stages 2, 3 or 4, stage 3 started from k1, the weights of another rule, ``v``, ``u`` stored from stage 4, an Euler sweep):
in fp64 each is at least ten bounds away at every N here up to 131; in fp32 all of them at N = 9, and on the finer grids
the history, ``v``/``u`` and Euler mutants only - an fp32 run at N >= 40 does NOT hold stage 3 or the weights.

Every call asserts the kernel that ran, ``(last_sim_path, last_waves_per_rod, last_overlap)``: with RK4 the mode
"overlap" must give the plain persistent kernel and an MLP in the sweeps one launch per step, with either set.

Consistency that needs no oracle: on K2c the tips of a 3-slot ring call and of the driver's form (ring calls of 5 steps
with ``keep_predictor`` and ``prev_init`` in the ring) are bit-identical to the full call's; on K2b and K2c rod b's result
is bit-identical to that of its own B = 1 call.

Below the simulate calls: ``kr_step_batch`` with RK4 from two entries of the oracle's run to the next, and
``kr_residual_batch`` with RK4 against ``cosserat_oracle.residual_rk4``.  Measured errors: LABBOOK.md (RK4 sweeps)."""
import numpy as np
import pytest

import full_matrix_cases as fm
import rk4_cases as rk
import test_gpu_full_matrices as gfm
from conftest import rel_l2
from gpu_helpers import inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = gfm.DEV
KR_RK4 = 1

# kernel -> (mode of gpu_helpers.set_mode_env, waves_per_rod, handle options, (path, waves per rod, overlap) that must have
# run - with RK4 the same for both parameter sets)
KERNELS = {
    "K2a": ("single", 1, {}, (0, 1, 0)),
    "K2b": ("multi", 1, {}, (1, 1, 0)),
    "K2c": ("persistent", 1, {}, (2, 1, 0)),
    "K2c-not-overlapped": ("overlap", 1, {"overlap": 1}, (2, 1, 0)),   # the overlapped kernel has no RK4 sweep
    "mlp-default": ("overlap", 0, {}, (1, 1, 0)),                      # K2b, NN = true: the persistent MLP kernels are Euler's
    "mlp-single": ("single", 1, {}, (0, 1, 0)),                        # K2a
}
FULL, ALL = ("full",), ("full", "ring", "driver")
# (kernel, N, T, controls, rods, call forms); every (N, T, controls) is one of rk.SIM_CASES
ROWS = [
    ("K2a", 9, 16, "sine", 9, FULL), ("K2a", 40, 16, "sine", 9, FULL), ("K2a", 40, 16, "jump", 9, FULL),
    ("K2a", 400, 5, "sine", 9, FULL),  # history in the global workspace
    ("K2b", 9, 16, "sine", 5, FULL), ("K2b", 27, 16, "sine", 5, FULL), ("K2b", 40, 16, "sine", 5, FULL),
    ("K2b", 40, 16, "jump", 5, FULL), ("K2b", 131, 6, "sine", 5, FULL),
    ("K2c", 9, 16, "sine", 5, ALL), ("K2c", 27, 16, "sine", 5, ALL), ("K2c", 40, 16, "sine", 5, ALL),
    ("K2c", 40, 16, "jump", 5, ALL),
    ("K2c", 112, 6, "sine", 5, ALL),  # the upper edge of K2c in fp64 (its LDS)
    ("K2c", 128, 6, "sine", 5, ALL),  # the upper edge of one_wave_range; fp32 only, as in test_gpu_full_matrices.F32_ONLY
    ("K2c-not-overlapped", 40, 16, "sine", 5, ("full", "ring")),
]
assert all(r[1:4] in rk.SIM_CASES for r in ROWS)
ROW_PARAMS = [pytest.param(*r, dt, id=f"{r[0]}-N{r[1]}-{r[3]}-{dt}") for r in ROWS for dt in ("f64", "f32")
              if dt == "f32" or (r[0], r[1]) not in gfm.F32_ONLY]
# NOT here: K2a with the history-input network (hist64, ``HS_NNH``) under RK4.  Its fp64 ``DIAG = true`` instantiation ended in a
# memory fault on the device at N = 12, B = 3 (LABBOOK.md, RK4 sweeps); until the cause is known no RK4 run of that network is
# part of the suite.
NN_ROWS = [("mlp-default", "elu64"), ("mlp-default", "elu6464"), ("mlp-single", "elu64")]
NN_RODS = 3
B1_KERNELS = ("K2b", "K2c")  # rod b against its own B = 1 call


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


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("kernel,N,T,kind,B,forms,dtype", ROW_PARAMS)
def test_step_kernels(torch_cuda, monkeypatch, kernel, N, T, kind, B, forms, dtype, variant):
    torch = torch_cuda
    ran = KERNELS[kernel][3]
    h = _handle(monkeypatch, kernel, N, variant)
    ctl = fm.batch_controls(T, kind, B)
    ref_tips, ref_states = rk.oracle_run(N, T, kind, variant, B=B)
    fixture = rk.fixture_run(N, kind, variant)
    assert fixture is None or fixture["T"] == T
    full_tips = None
    for form in forms:
        tips, status, stored = gfm.run(torch, h, ctl, form, dtype, ran, scheme=KR_RK4)
        gfm.check(f"rk4 {kernel} N={N} {kind} {form} {dtype} {variant}", dtype, tips, status, stored, ref_tips, ref_states, fixture)
        if form == "full":
            full_tips, full_stored = tips, stored
        else:  # the same kernel, the same arithmetic: the same bits
            d = float(np.max(np.abs(tips - full_tips)))
            assert np.array_equal(tips, full_tips), f"{form}: tips differ from the full call's by up to {d:.2e}"
    if kernel in B1_KERNELS:
        for b in range(B):
            t1, s1, st1 = gfm.run(torch, h, ctl[b:b + 1], "full", dtype, ran, scheme=KR_RK4)
            assert np.array_equal(t1[0], full_tips[b]), f"rod {b}: tips depend on the batch"
            assert np.array_equal(st1[T][0], full_stored[T][b]), f"rod {b}: last state depends on the batch"


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel,net", NN_ROWS)
def test_step_kernels_with_the_mlp_on(torch_cuda, monkeypatch, kernel, net, dtype, variant):
    """The network in all four stages of every sweep.  In the default modes RK4 takes one launch per step with either set of
    matrices (the ``NN = true`` RK4 instantiation of K2b); single shooting runs the same network lane by lane."""
    N, T, kind = rk.NN_CASE
    ran = KERNELS[kernel][3]
    h = _handle(monkeypatch, kernel, N, variant, net=net)
    ref_tips, ref_states = rk.numpy_oracle_run(N, T, kind, variant, B=NN_RODS, net=net)
    tips, status, stored = gfm.run(torch_cuda, h, fm.batch_controls(T, kind, NN_RODS), "full", dtype, ran, use_nn=True,
                                   scheme=KR_RK4)
    gfm.check(f"rk4 {kernel} {net} N={N} {dtype} {variant}", dtype, tips, status, stored, ref_tips, ref_states)


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", ["single", "multi"])
def test_step_batch(torch_cuda, monkeypatch, mode, dtype, variant):
    """kr_step_batch with RK4: from entries 7, 8 of the oracle's N = 40 run (pinned to the reference's by
    test_rk4_sweeps_cpu.py) and the controls of step 8 to the oracle's entry 9."""
    torch = torch_cuda
    B = 5
    N = rk.STEP_CASE[0]
    prev, cur, tens, nxt = rk.step_case(variant, B)
    set_mode_env(monkeypatch, mode, waves_per_rod=1)
    h = fm.apply_to_rod(make_robot(None, N), variant)._native()
    dt = torch.float64 if dtype == "f64" else torch.float32
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()
    s_prev, s_cur = (h.pack(t(s[:, :19]), t(s[:, 19:])) for s in (prev, cur))
    s_next = h.new_state(B, dt)
    G = t(cur[:, 7:13, 0])  # start values: n, m at the base of the state before (what a time loop carries over)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    h.step(s_prev, s_cur, s_next, G, t(tens), scheme=KR_RK4, tol=1e-12 if dtype == "f64" else 0.0, status=status)
    torch.cuda.synchronize()
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"))
    assert got == ((0, 1) if mode == "single" else (1, 1)), got
    assert int((status != 0).sum()) == 0, status
    y, z = h.unpack(s_next)
    out = torch.cat([y, z], dim=1).double().cpu().numpy()
    state_tol = fm.TOL[dtype][1]
    errs = [fm.block_errors(out[b], nxt[b]) for b in range(B)]
    for b in range(B):
        print(f"rk4 step {mode} {dtype} {variant} rod {b}: {fm.fmt_blocks(errs[b])}")
    for b in range(B):
        assert all(v < state_tol for v in errs[b].values()), (b, errs[b])


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_residual_batch(torch_cuda, variant, dtype):
    """kr_residual_batch with RK4 at entries 7, 8 of the N = 40 run, from the root's G (entry 9's) and from two G away from
    it, against ``cosserat_oracle.residual_rk4`` with the midpoint histories of the time loop: the swept state and the
    6-vector, under the bounds of test_gpu_full_matrices.py::test_residual_batch (fp32: the oracle sweeps the kernel's
    own rounded inputs)."""
    torch = torch_cuda
    import cosserat_oracle as orc
    B = 3
    N = rk.STEP_CASE[0]
    prev, cur, tens, nxt = rk.step_case(variant, B)
    dt = torch.float64 if dtype == "f64" else torch.float32
    rnd = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if dtype == "f32" else (lambda a: np.asarray(a, np.float64))
    G = np.array([nxt[b][7:13, 0] * s for b, s in zip(range(B), (1.0, 1.05, 0.9))])
    prev, cur, tens, G = rnd(prev), rnd(cur), rnd(tens), rnd(G)
    h = fm.apply_to_rod(make_robot(None, N), variant)._native()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()
    s_prev, s_cur = (h.pack(t(s[:, :19]), t(s[:, 19:])) for s in (prev, cur))
    s_next = s_cur.clone()
    res = h.residual(t(G), s_prev, s_cur, s_next, t(tens), scheme=KR_RK4).double().cpu().numpy()
    y, z = h.unpack(s_next)
    y, z = y.double().cpu().numpy(), z.double().cpu().numpy()
    D = fm.rod_params(N, variant).derived()
    tol_s, rtol, atol = (1e-10, 1e-8, 1e-10) if dtype == "f64" else (1e-5, 0.0, 1e-4)
    worst = []
    for b in range(B):
        ry, rz = cur[b, :19].copy(), cur[b, 19:].copy()
        yh, zh = D.c1 * cur[b, :19] + D.c2 * prev[b, :19], D.c1 * cur[b, 19:] + D.c2 * prev[b, 19:]
        rr = orc.residual_rk4(D, G[b], ry, rz, yh, 0.5 * (yh[:, :-1] + yh[:, 1:]), zh, 0.5 * (zh[:, :-1] + zh[:, 1:]), tens[b])
        ey, ez = rel_l2(y[b], ry), rel_l2(z[b, :, :N - 1], rz[:, :N - 1])   # (column N - 1 of z is never written)
        scale = np.abs(ry[7:13]).max()
        print(f"rk4 residual {dtype} {variant} rod {b}: y {ey:.1e} z {ez:.1e} r {np.abs(res[b] - rr).max() / scale:.1e} of max |n, m|"
              f" (|r| {np.abs(rr).max():.1e})")
        worst.append((ey, ez, np.allclose(res[b], rr, rtol=rtol, atol=atol * scale)))
    for b, (ey, ez, close) in enumerate(worst):
        assert ey < tol_s and ez < tol_s, (b, ey, ez)
        assert close, b
