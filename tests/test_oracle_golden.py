"""Pins the NumPy oracle against golden vectors produced by the reference
(tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest

import cosserat_oracle as orc
from conftest import load_golden, rel_l2

MODS = ["default", None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]
NN = ["elu64", "hist64", "tanh6464", "softplus6464", "relu6464", "elu6464"]


def _ode_rows(D, g, mlp=None):
    Q = g["y"].shape[0]
    out = np.zeros((Q, 25))
    for i in range(Q):
        tf = orc.tendon_force(D, g["tensions"][i])
        ys, z = orc.ode(D, g["y"][i], g["yh"][i], g["zh"][i], tf, mlp)
        out[i] = np.concatenate([ys, z])
    return out


@pytest.mark.parametrize("mod", MODS)
def test_ode_physics_presets(mod):
    g = load_golden("ode_kat")
    D = orc.params_for(mod, 10).derived()
    got = _ode_rows(D, g)
    ref = g[f"phys_{mod}"]
    assert np.max(np.abs(got - ref) / (np.abs(ref) + 1e-9 * np.abs(ref).max())) < 1e-9
    assert rel_l2(got, ref) < 1e-13


@pytest.mark.parametrize("name", NN)
def test_ode_with_mlp(name):
    g = load_golden("ode_kat")
    D = orc.params_for(None, 10).derived()
    mlp = orc.mlp_from_arrays(g, f"mlp_{name}")
    got = _ode_rows(D, g, mlp)
    ref = g[f"nn_{name}"]
    assert rel_l2(got, ref) < 1e-13
    # the correction must actually matter in this fixture
    assert rel_l2(g["phys_None"], ref) > 1e-6


@pytest.mark.parametrize("tag", ["N10_None", "N20_None", "N100_None", "N10_default", "N40_default"])
@pytest.mark.parametrize("scheme", ["euler", "rk4"])
def test_residuals(tag, scheme):
    g = load_golden("residual_kat")
    N = int(tag.split("_")[0][1:])
    mod = tag.split("_")[1]
    D = orc.params_for(mod, N).derived()
    y0, z0, yp, zp = g[f"{tag}_y"], g[f"{tag}_z"], g[f"{tag}_yp"], g[f"{tag}_zp"]
    yh = D.c1 * y0 + D.c2 * yp
    zh = D.c1 * z0 + D.c2 * zp
    for k, G in enumerate(g[f"{tag}_G"]):
        y, z = y0.copy(), z0.copy()
        with np.errstate(all="ignore"):
            if scheme == "euler":
                r = orc.residual_euler(D, G, y, z, yh, zh, g[f"{tag}_tens"])
            else:
                r = orc.residual_rk4(D, G, y, z, yh, 0.5 * (yh[:, :-1] + yh[:, 1:]), zh,
                                     0.5 * (zh[:, :-1] + zh[:, 1:]), g[f"{tag}_tens"])
        ref_r, ref_y, ref_z = g[f"{tag}_{scheme}_r"][k], g[f"{tag}_{scheme}_y"][k], g[f"{tag}_{scheme}_z"][k]
        if not np.all(np.isfinite(ref_r)):
            # the reference itself blows up here (RK4 at coarse N); nothing to pin
            continue
        assert rel_l2(y, ref_y) < 1e-11
        assert rel_l2(z, ref_z) < 1e-11
        assert np.allclose(r, ref_r, rtol=1e-9, atol=1e-11 * np.abs(ref_y[7:13]).max())
        # the last z column is never written by the sweep
        assert np.array_equal(z[:, -1], z0[:, -1])


def test_simulate_cfg1_fsolve_and_newton():
    """BASELINE config 1.  fsolve path = same algorithm as the reference;
    Newton path = what the HIP kernels implement."""
    g = load_golden("sim_cfg1")
    D = orc.params_for(None, 20).derived()
    assert np.all(g["ier"] == 1)
    traj, info = orc.simulate(D, g["ctl"], solver="fsolve", return_info=True)
    assert np.all(info["ier"] == 1)
    # hybrd's evaluation count is rounding-sensitive at a handful of steps; the path is otherwise identical
    assert np.mean(info["nfev"] == g["nfev"]) > 0.95
    assert rel_l2(traj[:, :3, -1], g["tip"]) < 1e-12
    assert rel_l2(traj[::10, :25], g["every10"]) < 1e-11
    assert rel_l2(traj[-1], g["last"]) < 1e-11
    trn = orc.simulate(D, g["ctl"], solver="newton")
    assert rel_l2(trn[:, :3, -1], g["tip"]) < 1e-9
    assert rel_l2(trn[::10, :25], g["every10"]) < 1e-7


def test_simulate_full50_layout():
    g = load_golden("sim_misc")
    D = orc.params_for(None, 10).derived()
    traj = orc.simulate(D, g["full50_ctl"])
    assert traj.shape == g["full50_traj"].shape == (8, 50, 10)
    assert rel_l2(traj, g["full50_traj"]) < 1e-9  # hybrd stops at xtol=1.5e-8; rounding-level path differences show at 1e-10


@pytest.mark.parametrize("mod", MODS[2:] + ["default"])
def test_simulate_presets(mod):
    g = load_golden("sim_misc")
    D = orc.params_for(mod, 10).derived()
    assert np.all(g[f"mod_{mod}_ier"] == 1)
    traj = orc.simulate(D, g[f"mod_{mod}_ctl"])
    assert rel_l2(traj[:, :25], g[f"mod_{mod}_traj"]) < 1e-9


@pytest.mark.parametrize("kind", ["step", "random"])
def test_simulate_inputs(kind):
    g = load_golden("sim_misc")
    D = orc.params_for(None, 10).derived()
    traj = orc.simulate(D, g[f"{kind}_ctl"])
    assert rel_l2(traj[:, :25], g[f"{kind}_traj"]) < 1e-10


def test_simulate_rk4():
    g = load_golden("sim_misc")
    D = orc.params_for(None, 40).derived()
    assert np.all(g["rk4_ier"] == 1) and np.all(np.isfinite(g["rk4_traj"]))
    traj = orc.simulate(D, g["rk4_ctl"], scheme="rk4")
    assert rel_l2(traj[:, :25], g["rk4_traj"]) < 1e-9


@pytest.mark.parametrize("name", ["elu64", "elu6464", "hist64"])
def test_simulate_with_mlp(name):
    g = load_golden("sim_nn")
    D = orc.params_for(None, int(g[f"{name}_N"])).derived()
    mlp = orc.mlp_from_arrays(g, f"mlp_{name}")
    assert np.all(g[f"{name}_ier"] == 1)
    traj = orc.simulate(D, g[f"{name}_ctl"], mlp=mlp)
    assert rel_l2(traj[:, :25], g[f"{name}_traj"]) < 1e-9
    # the network must move the trajectory visibly, otherwise this pins nothing
    assert rel_l2(orc.simulate(D, g[f"{name}_ctl"])[:, :3, -1], g[f"{name}_traj"][:, :3, -1]) > 1e-5


@pytest.mark.parametrize("name", ["elu512", "elu512n24"])
def test_simulate_default_network(name):
    """The reference's default network 28 -> 512 -> 25 inside simulate (sim_more fixture).  "elu512" carries the
    untrained initialisation as is; the reference's own fsolve gives up (ier = 5) at its 19th solve, so the pinned
    part ends there.  The damped Newton of the oracle - what the tests use as checker - reaches the same states."""
    g = load_golden("sim_more")
    D = orc.params_for(None, int(g[f"{name}_N"])).derived()
    mlp = orc.mlp_from_arrays(g, f"mlp_{name}")
    ier = g[f"{name}_ier"]
    good = len(ier) - 1 if np.all(ier == 1) else int(np.argmax(ier != 1))  # solves 0..good-1 -> entries 0..good
    assert good >= 11
    ref = g[f"{name}_traj"][: good + 1]
    traj = orc.simulate(D, g[f"{name}_ctl"], mlp=mlp)[: good + 1]
    assert rel_l2(traj[:, :25], ref) < 1e-9
    tn = orc.simulate(D, g[f"{name}_ctl"][: good + 1], mlp=mlp, solver="newton")
    assert max(rel_l2(tn[t, :25], ref[t]) for t in range(1, good + 1)) < 1e-8
    assert rel_l2(orc.simulate(D, g[f"{name}_ctl"][:8])[:, :3, -1], ref[:8, :3, -1]) > 1e-3  # the network matters


def test_simulate_lbfgs_branch():
    """knode.py:91-94 (use_fsolve=False): the oracle's restatement equals the reference's run; the root-finding
    branch agrees with it to the accuracy L-BFGS-B reaches (2.7e-6 on the tip)."""
    g = load_golden("sim_more")
    D = orc.params_for(None, 10).derived()
    ref = g["lbfgs_traj"]
    got = orc.simulate(D, g["lbfgs_ctl"], solver="lbfgs")
    assert rel_l2(got, ref) < 1e-9
    root = orc.simulate(D, g["lbfgs_ctl"], solver="newton")
    assert rel_l2(root[:, :3, -1], ref[:, :3, -1]) < 1e-5


@pytest.mark.parametrize("P", ["0_5", "2_0", "3_0"])
def test_n400_cfg5_inputs(P):
    """BASELINE cfg5 inputs (N = 400, calc_controls('sine', P)): the C restatement against the reference's tips."""
    import cosserat_oracle_c as oc
    g = load_golden("sim_more")
    assert np.all(g[f"n400_P{P}_ier"] == 1)
    ctl = g[f"n400_P{P}_ctl"]
    assert np.array_equal(ctl, np.array(orc.calc_controls("sine", float(P.replace("_", ".")), 0.05, 8)))
    tip, tr, bad = oc.simulate(orc.params_for(None, 400), ctl)
    ref = g[f"n400_P{P}_tip"]
    got = np.concatenate([tr[0, :3, -1][None], tip])[: len(ref)]
    assert bad == 0 and rel_l2(got, ref) < 1e-8
    assert rel_l2(tr[len(ref) - 1], g[f"n400_P{P}_last"]) < 1e-7


@pytest.mark.parametrize("use_nn", [0, 1])
def test_torch_full_sweep(use_nn):
    """cosserat_ode_torch.py:325-367 (fp32 torch) against the fp64 oracle sweep: value, full_rod layout
    (column 0 = [y0; z[:, 0] of the caller], column j+1 = [y_{j+1}; z_j]) and the y it leaves behind."""
    g = load_golden("sim_more")
    D = orc.params_for(None, 10).derived()
    mlp = orc.mlp_from_arrays(g, "mlp_tres") if use_nn else None
    y0, z0, yp, zp = g["tres_y"], g["tres_z"], g["tres_yp"], g["tres_zp"]
    yh, zh = D.c1 * y0 + D.c2 * yp, D.c1 * z0 + D.c2 * zp
    for k, G in enumerate(g["tres_G"]):
        y, z = y0.copy(), z0.copy()
        r = orc.residual_euler(D, G, y, z, yh, zh, g["tres_tens"], mlp)
        full = np.vstack([np.hstack([y[:, :1], y[:, 1:]]), np.hstack([z0[:, :1], z[:, :-1]])])
        assert abs(np.sum(r * r) - g[f"tres_val_{use_nn}"][k]) < 2e-4 * g[f"tres_val_{use_nn}"][k]
        assert rel_l2(full, g[f"tres_full_{use_nn}"][k]) < 1e-5
        assert rel_l2(y, g[f"tres_yafter_{use_nn}"][k]) < 1e-5
        if k == 1:
            # inputs of the gradient fixture (tres_grad.npz: reference autograd through the same sweep): its loss value
            # from the oracle, and dL/dG against central differences of the oracle with the network off - where the
            # reference's graph (cosserat_ode_torch.py:185-189 cuts u out of the quaternion rate) loses only the
            # rotation's response to the base moment: same sign and size, not the same number
            gg = load_golden("tres_grad")
            L = np.sum(r * r) + np.sum(full * gg["Wgt"])
            assert abs(L - gg[f"L_{use_nn}"]) < 2e-4 * abs(gg[f"L_{use_nn}"])
            if not use_nn:
                fd = np.zeros(6)
                for c in range(6):
                    vals = []
                    for sgn in (1.0, -1.0):
                        Gp = G.astype(np.float64).copy()
                        Gp[c] += sgn * 1e-6
                        yy, zz = y0.copy(), z0.copy()
                        rr = orc.residual_euler(D, Gp, yy, zz, yh, zh, g["tres_tens"], None)
                        ff = np.vstack([yy, np.hstack([z0[:, :1], zz[:, :-1]])])
                        vals.append(np.sum(rr * rr) + np.sum(ff * gg["Wgt"]))
                    fd[c] = (vals[0] - vals[1]) / 2e-6
                assert rel_l2(gg["dG_0"], fd) < 0.1 and rel_l2(gg["dG_0"][:3], fd[:3]) < 0.02


def test_controls_and_euler():
    g = load_golden("small")
    for key in g.files:
        if key.startswith("ctl_"):
            _, kind, arg, dt, T = key.split("_")
            got = np.array(orc.calc_controls(kind, float(arg), float(dt), int(T)))
            assert np.array_equal(got, g[key]), key
    e = orc.quaternion_to_euler(g["quat"].astype(np.float32))  # the reference casts to float32 first
    assert e.dtype == np.float32
    far = np.r_[0:40, 80:400]
    assert np.allclose(e[:, far], g["euler"][:, far], atol=2e-6)
    # columns 40:80 sit on the asin clamp where float32 rounding is amplified without bound;
    # compare the sine of the pitch there and the other two angles loosely
    near = np.r_[40:80]
    assert np.allclose(np.sin(e[1, near]), np.sin(g["euler"][1, near]), atol=1e-6)
    assert np.allclose(e[[0, 2]][:, near], g["euler"][[0, 2]][:, near], atol=1e-3)
    with pytest.raises(Exception):
        orc.calc_controls("ramp", 1.0, 0.05, 3)
    with pytest.raises(Exception):
        orc.setup_params("bogus")


# ---------------------------------------------------------------------------
# the scalar C restatement (oracle/cosserat_oracle_c.c) against the same reference trajectories
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,tol", [("sim_cfg1", 20, 1e-10), ("sim_n100", 100, 1e-9), ("sim_n400", 400, 1e-8)])
def test_c_oracle_tips_vs_reference(name, N, tol):
    """orc_simulate (Newton to 1e-12) reproduces the tip paths the REFERENCE produced with fsolve."""
    import cosserat_oracle_c as oc
    g = load_golden(name)
    P = orc.params_for(None, N)
    tip, tr, bad = oc.simulate(P, g["ctl"])
    assert bad == 0
    ref = g["tip"]  # entry 0 = initial tip, last solve dropped (knode.py:96-102)
    got = np.concatenate([tr[0, :3, -1][None], tip])[: len(ref)]
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < tol


@pytest.mark.parametrize("mod", [None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"])
def test_c_oracle_vs_numpy_oracle(mod):
    """Full states (all 25 rows) of the C and the NumPy restatement agree for every preset."""
    import cosserat_oracle_c as oc
    P = orc.params_for(mod, 13)
    ctl = np.array(orc.calc_controls("sine", 0.7, P.del_t, 12))
    want = orc.simulate(P.derived(), np.vstack([ctl, ctl[-1:]]), solver="newton")
    tip, tr, bad = oc.simulate(P, ctl)
    assert bad == 0
    assert np.linalg.norm(tr - want[:13, :25]) / np.linalg.norm(want[:13, :25]) < 1e-10


# ---------------------------------------------------------------------------
# round 3 fixtures (tests/golden/round3.npz)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mid_N40_default", "mid_N100_None"])
def test_rk4_residual_with_callers_midpoints(tag):
    """getResidualRK4 reads the midpoint histories the caller passes (cosserat_ode.py:225,233-234); the fixture's
    are NOT the linear interpolation of yh, zh."""
    g = load_golden("round3")
    N = int(tag.split("_")[1][1:])
    mod = tag.split("_")[2]
    D = orc.params_for(mod, N).derived()
    y0, z0, yp, zp = g[f"{tag}_y"], g[f"{tag}_z"], g[f"{tag}_yp"], g[f"{tag}_zp"]
    yh = D.c1 * y0 + D.c2 * yp
    zh = D.c1 * z0 + D.c2 * zp
    lin = 0.5 * (yh[:, :-1] + yh[:, 1:])
    assert rel_l2(g[f"{tag}_yh_int"], lin) > 1e-2  # the midpoints really differ from the interpolation
    for k, G in enumerate(g[f"{tag}_G"]):
        y, z = y0.copy(), z0.copy()
        r = orc.residual_rk4(D, G, y, z, yh, g[f"{tag}_yh_int"], zh, g[f"{tag}_zh_int"], g[f"{tag}_tens"])
        assert rel_l2(y, g[f"{tag}_yout"][k]) < 1e-12
        assert rel_l2(z, g[f"{tag}_zout"][k]) < 1e-12
        assert np.allclose(r, g[f"{tag}_r"][k], rtol=1e-9, atol=1e-11 * np.abs(y[7:13]).max())


def test_cfg2_rods_of_the_256_draw():
    """BASELINE cfg2: rod 0 of the default_rng(1234) draw for B = 256 (N = 100), first 12 steps, against the
    reference's tips - pins the oracle's control generator for the full batch size and the fixture's rod order."""
    g = load_golden("round3")
    assert list(g["cfg2_rods"]) == [0, 1, 3, 4, 6, 7, 8, 10] and int(g["cfg2_B"]) == 256
    D = orc.params_for(None, 100).derived()
    T = 12
    ctl = orc.batch_sine_controls(256, int(g["cfg2_T"]), D.P.del_t, int(g["cfg2_seed"]))
    with np.errstate(all="ignore"):
        traj = orc.simulate(D, ctl[0][:T], solver="fsolve")
    assert rel_l2(traj[:, :3, -1], g["cfg2_tip"][0][:T]) < 1e-9


# ---------------------------------------------------------------------------
# round 4: the reference's full parameter surface (fixture bc.npz: tip wrench, tilted non-unit h0, p0, moving base,
# asymmetric tendon directions with a z component - cosserat_ode.py:28-29,37-41,44-47 entering :194-195,206-207)
# ---------------------------------------------------------------------------
def bc_params(g, N, mod=None):
    P = orc.params_for(mod, N)
    for k in ("F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
        setattr(P, k, np.array(g[f"par_{k}"], dtype=np.float64))
    return P


def test_bc_fixture_is_off_default():
    g = load_golden("bc")
    P0 = orc.RodParams()
    for k in ("F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs"):
        assert not np.allclose(g[f"par_{k}"], getattr(P0, k)), k
    assert abs(np.linalg.norm(g["par_h0"]) - 1.0) > 0.05
    assert np.all(np.abs(g["par_tendon_dirs"][:, 2]) > 0.05)


@pytest.mark.parametrize("N", [20, 100])
def test_bc_simulate(N):
    g = load_golden("bc")
    assert np.all(g[f"sim_N{N}_ier"] == 1)
    D = bc_params(g, N).derived()
    traj = orc.simulate(D, g[f"sim_N{N}_ctl"])
    assert rel_l2(traj[:, :3, -1], g[f"sim_N{N}_tip"]) < 1e-10
    assert rel_l2(traj[-1], g[f"sim_N{N}_last"]) < 1e-9
    if N == 20:
        assert rel_l2(traj[:, :25], g["sim_N20_traj"]) < 1e-9
        trn = orc.simulate(D, g["sim_N20_ctl"], solver="newton")
        assert rel_l2(trn[:, :25], g["sim_N20_traj"]) < 1e-7
        # the boundary column is what the parameters say (cosserat_ode.py:194)
        assert np.allclose(traj[5, 0:3, 0], g["par_p0"]) and np.allclose(traj[5, 3:7, 0], g["par_h0"])
        assert np.allclose(traj[5, 13:16, 0], g["par_q0"]) and np.allclose(traj[5, 16:19, 0], g["par_w0"])
    else:
        assert rel_l2(traj[::10, :25], g["sim_N100_every10"]) < 1e-9


def test_bc_step_input():
    g = load_golden("bc")
    assert np.all(g["step_N40_ier"] == 1)
    traj = orc.simulate(bc_params(g, 40).derived(), g["step_N40_ctl"])
    assert rel_l2(traj[:, :25], g["step_N40_traj"]) < 1e-9


@pytest.mark.parametrize("N", [20, 100])
@pytest.mark.parametrize("scheme", ["euler", "rk4"])
def test_bc_residuals(N, scheme):
    g = load_golden("bc")
    D = bc_params(g, N).derived()
    tag = f"res_N{N}"
    y0, z0, yp, zp = g[f"{tag}_y"], g[f"{tag}_z"], g[f"{tag}_yp"], g[f"{tag}_zp"]
    yh = D.c1 * y0 + D.c2 * yp
    zh = D.c1 * z0 + D.c2 * zp
    for k, G in enumerate(g[f"{tag}_G"]):
        ref_r, ref_y, ref_z = g[f"{tag}_{scheme}_r"][k], g[f"{tag}_{scheme}_y"][k], g[f"{tag}_{scheme}_z"][k]
        if not np.all(np.isfinite(ref_r)):
            continue
        y, z = y0.copy(), z0.copy()
        with np.errstate(all="ignore"):
            if scheme == "euler":
                r = orc.residual_euler(D, G, y, z, yh, zh, g[f"{tag}_tens"])
            else:
                r = orc.residual_rk4(D, G, y, z, yh, 0.5 * (yh[:, :-1] + yh[:, 1:]), zh,
                                     0.5 * (zh[:, :-1] + zh[:, 1:]), g[f"{tag}_tens"])
        assert rel_l2(y, ref_y) < 1e-11 and rel_l2(z, ref_z) < 1e-11
        assert np.allclose(r, ref_r, rtol=1e-9, atol=1e-11 * np.abs(ref_y[7:13]).max())


@pytest.mark.parametrize("name", ["elu6464", "elu64"])
def test_bc_simulate_with_mlp(name):
    g = load_golden("bc")
    assert np.all(g[f"nn_{name}_ier"] == 1)
    mlp = orc.mlp_from_arrays(g, f"mlp_{name}")
    D = bc_params(g, int(g[f"nn_{name}_N"])).derived()
    traj = orc.simulate(D, g[f"nn_{name}_ctl"], mlp=mlp)
    assert rel_l2(traj[:, :25], g[f"nn_{name}_traj"]) < 1e-9


def test_c_oracle_under_sanitizers():
    """`make -C oracle asan`: the C restatement as a standalone program under AddressSanitizer + UBSan,
    N = 10 / 20 / 100 / 400 with and without the trajectory buffer.  CPU build only (GPU sanitizers are not available on
    this pool)."""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.run(["make", "-C", here, "asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "lib", "oracle_c_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count("unconverged=0") == 8, r.stdout


# ---------------------------------------------------------------------------
# the reference at the lengths the BASELINE configurations run (tests/golden/sim_long_*.npz, tests/long_run_cases.py)
# ---------------------------------------------------------------------------
def _c_oracle_long(case, b, c2_scale=1.0):
    import cosserat_oracle_c as oc
    T = case["T"]
    tip, tr, bad = oc.simulate(orc.params_for(None, case["N"]), case["ctl"][b][: T - 1], c2_scale=c2_scale)
    return np.concatenate([tr[0, :3, -1][None], tip]), tr, bad


@pytest.mark.parametrize("name,b", [("n100", 0), ("n100", 1), ("n400", 0)])
def test_c_oracle_long_runs_vs_reference(name, b):
    """The C oracle against the reference over cfg2's 200 steps (rod A smooth, rod B with two late tension jumps) and cfg5's
    100 steps at N = 400: tips per 50-step window and over the whole run to 1e-9, the stored states to 1e-8.  Measured:
    LABBOOK.md (long runs)."""
    import long_run_cases as lc
    case = lc.long_case(name)
    if name == "n100":
        assert case["B"] == 2 and case["jump_a"] == 0.5  # rod B is there, with the largest of the three jumps
    got, tr, bad = _c_oracle_long(case, b)
    assert bad == 0
    errs = lc.window_errors(got, case["tip"][b], case["window"])
    print(f"C oracle {name} rod {b}: tip windows {['%.1e' % e for e in errs]}")
    assert max(errs) < 1e-9, errs
    serr = {k: rel_l2(tr[k], v[b]) for k, v in case["states"].items() if k > 0}
    print(f"C oracle {name} rod {b}: states {{{', '.join('%d: %.1e' % kv for kv in serr.items())}}}")
    assert max(serr.values()) < 1e-8, serr


def test_long_run_windows_resolve_a_history_error():
    """The test of the tests: the C oracle with the BDF2 history coefficient c2 scaled by 1 + 1e-6 must MISS 1e-8 in the last
    50-step window of rod A - an error of that size in what a step carries over from two steps back is visible there."""
    import long_run_cases as lc
    case = lc.long_case("n100")
    got, _, bad = _c_oracle_long(case, 0, c2_scale=1.0 + 1e-6)
    assert bad == 0
    errs = lc.window_errors(got, case["tip"][0], case["window"])
    print(f"c2 (1 + 1e-6): tip windows {['%.1e' % e for e in errs]}")
    assert errs[-2] > 1e-8, errs
    clean, _, _ = _c_oracle_long(case, 0)
    assert lc.window_errors(clean, case["tip"][0], case["window"])[-2] < 1e-9  # (the hook is off again)


@pytest.mark.parametrize("solver", ["newton", "fsolve"])
@pytest.mark.parametrize("b", [0, 1])
def test_numpy_oracle_long_run_with_mlp(solver, b):
    """cfg3's network (28 -> 64 -> 64 -> 25, elu, seed 7) in every sweep over cfg3's 64 steps at N = 100, rods 3 and 1000 of
    its draw: tips per 16-step window and the stored states to 1e-8, the bound of the short MLP fixtures."""
    import long_run_cases as lc
    case = lc.long_case("nn")
    assert case["rods"] == [3, 1000]
    D = orc.params_for(None, case["N"]).derived()
    with np.errstate(all="ignore"):
        traj = orc.simulate(D, case["ctl"][b], mlp=case["mlp"], solver=solver)
    errs = lc.window_errors(traj[:, :3, -1], case["tip"][b], case["window"])
    print(f"NumPy oracle ({solver}) nn rod {b}: tip windows {['%.1e' % e for e in errs]}")
    assert max(errs) < 1e-8, errs
    serr = {k: rel_l2(traj[k, :25], v[b]) for k, v in case["states"].items() if k > 0}
    print(f"NumPy oracle ({solver}) nn rod {b}: states {{{', '.join('%d: %.1e' % kv for kv in serr.items())}}}")
    assert max(serr.values()) < 1e-8, serr


@pytest.mark.parametrize("N", [100, 400])
def test_rough_batch_is_mostly_solved_by_the_oracle(N):
    """tests/test_gpu_long_runs.py holds the kernels against the C oracle on the rods it converged on at every step: at
    least ten of the twelve, and the rough ones must really differ from their smooth base late in the run."""
    import long_run_cases as lc
    case = lc.rough_case(N)
    assert int(case["good"].sum()) >= lc.ROUGH_MIN_GOOD, case["good"].tolist()
    base = orc.batch_sine_controls(256, case["T"], lc.DEL_T, 1234)[: lc.ROUGH_B]
    first = [int(np.argmax(np.any(case["ctl"][b] != base[b], axis=1))) for b in range(4, 12)]
    assert np.array_equal(case["ctl"][:4], base[:4]) and all(f >= min(case["T"] - case["T"] // 3, case["T"] - 30) for f in first), first
    assert all(np.any(case["ctl"][b] != base[b]) for b in range(4, 12))
    assert np.abs(case["tip"][4:]).max() < 1.0
