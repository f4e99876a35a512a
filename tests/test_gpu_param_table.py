"""Heterogeneous batches (per-rod parameter tables, kr_simulate_batch_table) on the MI355X.

Rod b of one simulate call runs with row b of a table instead of the handle's parameters.  The reference side of every
comparison is either a fixture written by the unmodified reference (tests/golden/*.npz, entry 0 = the straight rod,
entry t = the state after step t, the last solve dropped - so ``traj[b, :T_fix]`` lines up with a fixture of ``T_fix``
entries), the oracle's tightly converged Newton solver, or the plain ``kr_simulate_batch`` on the same inputs.
Tolerances are the project's own: fp64 ``rel_l2 < 1e-8`` against reference-held trajectories, fp32 tips ``< 1e-5``;
kernel against kernel at the same root: states ``< 1e-8``, tips ``< 1e-9`` (tests/test_gpu_overlap.py).

Every test asserts what ran: one persistent launch (``last_sim_path == 2``), one wavefront per rod, the overlapped
kernel or not as asked, and ``status == 0`` on every step of every rod."""
import copy

import numpy as np
import pytest

from conftest import load_golden, rel_l2
from gpu_helpers import expected_path, inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODS7 = ["noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]
BC_KEYS = ("F_tip", "M_tip", "p0", "h0", "q0", "w0", "tendon_dirs")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def bc_robot(g, N, mod=None):
    r = make_robot(mod, N)
    for k in BC_KEYS:
        setattr(r, k, np.array(g[f"par_{k}"], dtype=np.float64))
    return r


def assert_table_ran(h, overlap):
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
    assert got == (2, 1, overlap), f"(path, waves per rod, overlap) = {got}, expected (2, 1, {overlap})"


def check(label, value, bound):
    print(f"{label}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, f"{label}: {value:.3e} >= {bound:.0e}"


def eight_mods():
    """The reference's experiment (knode.setup_robot's mods, knode.py:6-53) as one batch: robots, controls, fixtures."""
    g = load_golden("sim_misc")
    robots = [make_robot(m, 10) for m in MODS7] + [make_robot(None, 10)]
    ctl = np.stack([g[f"mod_{m}_ctl"] for m in MODS7] + [g["random_ctl"][:16]])
    ref = [g[f"mod_{m}_traj"] for m in MODS7] + [g["random_traj"][:16]]
    return robots, ctl, ref


# ---------------------------------------------------------------------------
# 1. the eight mods in one launch, against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eight_mods_in_one_launch(torch_cuda, monkeypatch, overlap, dtype):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    robots, ctl, ref = eight_mods()
    carrier = make_robot(None, 10)
    h = carrier._native()
    h.set_option("overlap", overlap)
    out = simulate_batch(carrier, ctl, dtype=dtype, robots=robots)
    assert_table_ran(h, overlap)
    assert np.all(out["status"] == 0), np.argwhere(out["status"] != 0)[:8]
    assert out["traj"].shape == (8, 17, 25, 10)
    for b in range(8):
        name = (MODS7 + ["None"])[b]
        if dtype == "f64":
            check(f"rod {b} ({name}) trajectory", rel_l2(out["traj"][b, :16], ref[b]), 1e-8)
        else:
            check(f"rod {b} ({name}) fp32 tip path", rel_l2(out["traj"][b, :16, :3, -1], ref[b][:, :3, -1]), 1e-5)
    # the initial rod takes its length from its own row
    assert out["traj"][2, 0, 2, -1] == 0.4 and out["traj"][0, 0, 2, -1] == 0.635


# ---------------------------------------------------------------------------
# 2. the full parameter surface next to a plain rod
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 100])
def test_full_parameter_surface_next_to_plain_rod(torch_cuda, monkeypatch, N):
    """Rod 0 carries everything a row can carry (tip wrench, tilted non-unit h0, p0, moving base, asymmetric tendon
    directions: bc.npz), rod 1 is the plain preset; N = 100 is the headline kernel's shape."""
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("bc")
    p = load_golden("sim_cfg1" if N == 20 else "sim_n100")
    carrier = make_robot(None, N)
    robots = [bc_robot(g, N), make_robot(None, N)]
    ctl = np.stack([g[f"sim_N{N}_ctl"], p["ctl"][:30]])
    out = simulate_batch(carrier, ctl, robots=robots)
    assert_table_ran(carrier._handle, 1)
    assert np.all(out["status"] == 0)
    tr = out["traj"]
    check("rod 0 tip path", rel_l2(tr[0, :30, :3, -1], g[f"sim_N{N}_tip"]), 1e-8)
    check("rod 1 tip path", rel_l2(tr[1, :30, :3, -1], p["tip"][:30]), 1e-8)
    if N == 20:
        check("rod 0 trajectory", rel_l2(tr[0, :30], g["sim_N20_traj"]), 1e-8)
        check("rod 1 every 10th state", rel_l2(tr[1, :30:10], p["every10"][:3]), 1e-8)
        assert np.allclose(tr[0, 7, 0:3, 0], g["par_p0"], rtol=0, atol=1e-15)
        assert np.allclose(tr[0, 7, 3:7, 0], g["par_h0"], rtol=0, atol=1e-15)
        assert np.allclose(tr[1, 7, 3:7, 0], [1, 0, 0, 0], rtol=0, atol=0)
    else:
        check("rod 0 every 10th state", rel_l2(tr[0, :30:10], g["sim_N100_every10"]), 1e-8)
        check("rod 1 every 10th state", rel_l2(tr[1, :30:10], p["every10"][:3]), 1e-8)


# ---------------------------------------------------------------------------
# 3. MLP on: one network for all rods
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn_oracle():
    import cosserat_oracle as orc
    g = load_golden("bc")
    mlp = orc.mlp_from_arrays(g, "mlp_elu64")
    ctl = g["nn_elu64_ctl"]
    refs = []
    for m in (None, "damping", "short"):
        traj, info = orc.simulate(orc.setup_params(m, 20).derived(), ctl, mlp=mlp, solver="newton", return_info=True)
        assert np.all(info["ier"] == 1)
        refs.append(traj[:, :25])
    return mlp, ctl, refs


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mlp_on_one_network_for_all_rods(torch_cuda, monkeypatch, nn_oracle, dtype):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("bc")
    mlp, ctl1, refs = nn_oracle
    assert expected_path("persistent", 20, mlp) == 2
    carrier = make_robot(None, 20)
    inject(carrier, mlp)
    robots = [bc_robot(g, 20)] + [make_robot(m, 20) for m in (None, "damping", "short")]
    ctl = np.stack([ctl1] * 4)
    out = simulate_batch(carrier, ctl, dtype=dtype, robots=robots)
    assert_table_ran(carrier._handle, 0)
    assert np.all(out["status"] == 0)
    want = [g["nn_elu64_traj"]] + refs
    for b in range(4):
        if dtype == "f64":
            check(f"rod {b} trajectory", rel_l2(out["traj"][b, :20], want[b]), 1e-8)
        else:
            check(f"rod {b} fp32 tip path", rel_l2(out["traj"][b, :20, :3, -1], want[b][:, :3, -1]), 1e-5)


# ---------------------------------------------------------------------------
# 4. a table of identical rows is the plain call
# ---------------------------------------------------------------------------
def _run(torch, h, ctl, dtype, table=None, ring=False, chunks=None, scheme=0):
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dtype, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dtype, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dtype, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    if chunks is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, scheme=scheme)
    else:
        t0 = 0
        for n in chunks:
            tp = torch.empty((B, n, 3), dtype=dtype, device=DEV)
            sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + n].contiguous(), st[t0:], G, tip=tp, status=sx,
                       prev_init=st[t0 - 1] if t0 else None, table=table)
            tip[:, t0:t0 + n] = tp
            status[:, t0:t0 + n] = sx
            t0 += n
    torch.cuda.synchronize()
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def test_table_of_identical_rows_is_the_plain_call(torch_cuda, monkeypatch):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    r = make_robot(None, 100)
    h = r._native()
    B, T = 64, 40
    ctl = torch.as_tensor(orc.batch_sine_controls(B, T, r.del_t, 1235), device=DEV).to(dt).contiguous()
    s_tol, t_tol = 1e-8, 1e-9  # kernel against kernel at the same root (tests/test_gpu_overlap.py)
    with h.param_table([r._params()] * B) as tab:
        for ring in (False, True):
            plain = _run(torch, h, ctl, dt, ring=ring)
            assert h.get_option("last_overlap") == 1 and h.get_option("last_sim_path") == 2
            tabd = _run(torch, h, ctl, dt, table=tab, ring=ring)
            assert_table_ran(h, 1)
            assert np.all(plain["status"] == 0) and np.array_equal(plain["status"], tabd["status"])
            print(f"ring={ring}: bit-identical tips {np.array_equal(plain['tip'], tabd['tip'])}, "
                  f"states {np.array_equal(plain['states'], tabd['states'])}")
            check(f"ring={ring} tips", rel_l2(tabd["tip"], plain["tip"]), t_tol)
            slots = [T % 3, (T - 1) % 3, (T - 2) % 3] if ring else range(T + 1)
            for k in slots:
                assert rel_l2(tabd["states"][k], plain["states"][k]) < s_tol, k
        one = _run(torch, h, ctl, dt, table=tab)
        h.set_option("keep_predictor", 1)
        try:
            ch = _run(torch, h, ctl, dt, table=tab, chunks=[10, 10, 10, 10])
        finally:
            h.set_option("keep_predictor", 0)
        assert_table_ran(h, 1)
        assert np.all(ch["status"] == 0)
        check("keep_predictor chunks, last state", rel_l2(ch["states"][T][..., :25], one["states"][T][..., :25]), 1e-7)
        check("keep_predictor chunks, tips", rel_l2(ch["tip"], one["tip"]), 1e-7)


# ---------------------------------------------------------------------------
# 5. batch independence: permuting rows and controls permutes the outputs bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
def test_permuted_rows_permute_the_outputs_bitwise(torch_cuda, monkeypatch, overlap):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    robots, ctl, _ = eight_mods()
    carrier = make_robot(None, 10)
    h = carrier._native()
    h.set_option("overlap", overlap)
    a = simulate_batch(carrier, ctl, robots=robots)
    assert_table_ran(h, overlap)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    b = simulate_batch(carrier, ctl[perm], robots=[robots[i] for i in perm])
    assert_table_ran(h, overlap)
    assert np.all(a["status"] == 0) and np.all(b["status"] == 0)
    for k in ("traj", "tip", "G"):
        assert np.array_equal(b[k], a[k][perm]), k


# ---------------------------------------------------------------------------
# 6. a random draw against the oracle
# ---------------------------------------------------------------------------
def random_draw():
    """B = 16 rods around ``setup_params(None, 40)``.  One generator, ``default_rng(2026)``, walked rod by rod: six
    factors ``exp(U(-0.3, 0.3))`` for E, r, rho, L, Bbt, C (in that order), then F_tip ~ N(0, 0.05)^3, then
    M_tip ~ N(0, 0.002)^3."""
    import cosserat_oracle as orc
    rng = np.random.default_rng(2026)
    base = orc.setup_params(None, 40)
    out = []
    for b in range(16):
        f = np.exp(rng.uniform(-0.3, 0.3, 6))
        P = copy.deepcopy(base)
        P.E, P.r, P.rho, P.L = base.E * f[0], base.r * f[1], base.rho * f[2], base.L * f[3]
        P.Bbt, P.C = base.Bbt * f[4], base.C * f[5]
        P.F_tip, P.M_tip = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3)
        out.append(P)
    return out


@pytest.fixture(scope="module")
def draw_oracle():
    import cosserat_oracle as orc
    Ps = random_draw()
    ctl = orc.batch_sine_controls(16, 24, 0.05, 77)
    refs = []
    for b, P in enumerate(Ps):
        traj, info = orc.simulate(P.derived(), ctl[b], solver="newton", return_info=True)
        assert np.all(info["ier"] == 1), b
        refs.append(traj[:, :25])
    return Ps, ctl, refs


def test_random_draw_against_the_oracle(torch_cuda, monkeypatch, draw_oracle):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    Ps, ctl, refs = draw_oracle
    robots = []
    for P in Ps:
        r = make_robot(None, 40)
        for k in ("E", "r", "rho", "L", "Bbt", "C", "F_tip", "M_tip"):
            setattr(r, k, copy.deepcopy(getattr(P, k)))
        r.compute_intermediate_terms()
        robots.append(r)
    carrier = make_robot(None, 40)
    out = simulate_batch(carrier, ctl, robots=robots)
    assert_table_ran(carrier._handle, 1)
    assert np.all(out["status"] == 0), np.argwhere(out["status"] != 0)[:8]
    tipx = out["traj"][:, :24, 0, -1]
    print(f"tip x over the batch: {tipx.min():+.3f} .. {tipx.max():+.3f} m")
    assert tipx.max() - tipx.min() > 0.5  # the rods differ visibly
    for b in range(16):
        check(f"rod {b} tip path", rel_l2(out["traj"][b, :24, :3, -1], refs[b][:, :3, -1]), 1e-8)
        check(f"rod {b} trajectory", rel_l2(out["traj"][b, :24], refs[b]), 1e-8)


# ---------------------------------------------------------------------------
# 7. refusals: never a silent fallback to the handle's parameters
# ---------------------------------------------------------------------------
def test_refusals(torch_cuda, monkeypatch):
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    r = make_robot(None, 40)
    h = r._native()
    rows = [make_robot(m, 40)._params() for m in (None, "short", "damping")]
    ctl = torch.full((3, 6, 4), 5.0, dtype=dt, device=DEV)

    def refused(fn, code):
        with pytest.raises(kn.KrError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert len(str(e.value)) > 30
        return str(e.value)

    with h.param_table(rows) as tab:
        ok = _run(torch, h, ctl, dt, table=tab)
        assert_table_ran(h, 1)
        assert np.all(ok["status"] == 0)
        assert "Euler" in refused(lambda: _run(torch, h, ctl, dt, table=tab, scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED)
        h.set_option("waves_per_rod", 4)
        assert "waves_per_rod" in refused(lambda: _run(torch, h, ctl, dt, table=tab), kn.KR_E_UNSUPPORTED)
        assert h.get_option("last_waves_per_rod") == 1
        h.set_option("waves_per_rod", 1)
        again = _run(torch, h, ctl, dt, table=tab)
        assert_table_ran(h, 1)
        assert np.array_equal(again["tip"], ok["tip"])
        # a table made on one handle, used with a handle of another N
        other = make_robot(None, 20)._native()
        st = other.new_state(3, dt, n_slots=7)
        refused(lambda: other.init_straight(st[0], table=tab), kn.KR_E_ARG)
        msg = refused(lambda: other.simulate(ctl, st, torch.zeros((3, 6), dtype=dt, device=DEV), table=tab), kn.KR_E_ARG)
        assert "N" in msg
        # batch size of the call = the table's
        with pytest.raises(kn.KrError):
            _run(torch, h, ctl[:2].contiguous(), dt, table=tab)
    # a non-diagonal row
    full = make_robot("youngs", 40)
    full.Bbt = full.Bbt + 1e-3
    assert "Bbt" in refused(lambda: h.param_table(rows + [full._params()]), kn.KR_E_UNSUPPORTED)
    # a long rod: the several-wavefront kernels have no table form
    long_rod = make_robot(None, 400)
    assert "N" in refused(lambda: long_rod._native().param_table([long_rod._params()] * 2), kn.KR_E_UNSUPPORTED)


# ---------------------------------------------------------------------------
# 8. argument errors of the five C entry points of the table family: the (rc, kr_last_error()) pair of each, and which of
#    two mistakes a caller hears of first.  Nothing is launched.
# ---------------------------------------------------------------------------
ARG_ENTRIES = ("table", "loads", "boundary", "keypoints", "bank")
BAD = "bad"  # (a value the case replaces by something wrong of its kind; see arg_error_call)


def arg_error_cases():
    """[(label, entry, overrides)]: one argument wrong, then the pairs whose outcome depends on the order of the checks."""
    cases = []
    for e in ARG_ENTRIES:
        add = lambda label, **over: cases.append((f"{e}: {label}", e, over))
        add("null table", t=None)
        for p in ("ctl", "states", "G"):
            add(f"null {p}", **{p: None})
        add("T < 0", T=-1)
        add("table of another N", t="other_N")
        add("table of another del_t", t="other_del_t")
        add("null table, T < 0", t=None, T=-1)
        add("table of another N, T < 0", t="other_N", T=-1)
        add("table of another N, T = 0", t="other_N", T=0)
        add("T < 0, null ctl", T=-1, ctl=None)
        add("T = 0, null ctl", T=0, ctl=None)
        add("null ctl, null states, null G", ctl=None, states=None, G=None)
        add("null states, null G", states=None, G=None)
        if e in ("loads", "boundary", "keypoints"):
            add("null history", hist=None)
            add("null table, null history", t=None, hist=None)
            add("null history, T < 0", hist=None, T=-1)
            add("null history, table of another N", hist=None, t="other_N")
        if e == "keypoints":
            add("null kp", kp=None)
            add("misaligned kp", kp=BAD)
            add("point out of range", idx=[3, 5, 10])
            add("points not increasing", idx=[3, 7, 5])
            add("no points", idx=[])
            add("null kp, point out of range", kp=None, idx=[3, 5, 10])
            add("misaligned kp, point out of range", kp=BAD, idx=[3, 5, 10])
            add("point out of range, T < 0", idx=[3, 5, 10], T=-1)
            add("misaligned kp, table of another N", kp=BAD, t="other_N")
            add("misaligned kp, T < 0", kp=BAD, T=-1)
            add("point of the other table's range, table of another N", idx=[3, 5, 20], t="other_N")
        if e == "bank":
            add("null bank", bank=None)
            add("null index array", nets=None)
            add("index out of range", nets=[0, 1, 2, 0, 1, 0])
            add("negative index", nets=[0, -1, 0, 0, 0, 0])
            add("null table, null bank", t=None, bank=None)
            add("index out of range, T < 0", nets=[0, 1, 2, 0, 1, 0], T=-1)
            add("index out of range, T = 0", nets=[0, 1, 2, 0, 1, 0], T=0)
            add("table of another N, index out of range", t="other_N", nets=[0, 1, 2, 0, 1, 0])
            add("index out of range, null ctl", nets=[0, 1, 2, 0, 1, 0], ctl=None)
    return cases


def arg_error_pairs(torch):
    """{label: (rc, message or None)} of arg_error_cases() on B = 6, N = 10, T = 2, fp64; None where rc = 0."""
    import ctypes as C

    import cosserat_oracle as orc
    import krod_native as kn
    B, N, T, dt = 6, 10, 2, torch.float64
    r = make_robot(None, N)
    h = r._native()
    slow = make_robot(None, N)
    slow.del_t = 2 * slow.del_t
    slow.compute_intermediate_terms()
    ctl = torch.full((B, T, 4), 5.0, dtype=dt, device=DEV)
    hist = {"table": None, "bank": None, "loads": torch.zeros((B, T, 6), dtype=dt, device=DEV)}
    hist["boundary"] = hist["keypoints"] = torch.zeros((B, T, kn.KR_BND), dtype=dt, device=DEV)
    kp = torch.zeros((T, B, 3, kn.KR_SLOTS), dtype=dt, device=DEV)
    st = h.new_state(B, dt, n_slots=T + 1)
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    net = orc.make_mlp([28, 64, 64, 25], "elu", seed=15)
    out = {}
    with h.param_table([r._params()] * B) as tab, make_robot(None, 23)._native().param_table([make_robot(None, 23)._params()] * B) as tab23, \
            slow._native().param_table([slow._params()] * B) as tab_slow, h.mlp_bank([(net.weights, net.biases, net.acts)] * 2) as bank:
        h.init_straight(st[0], table=tab)
        before = st.clone()
        ptr = lambda x: None if x is None else x if isinstance(x, int) else C.c_void_p(x.data_ptr())
        for label, entry, over in arg_error_cases():
            a = dict(t=tab._t, T=T, ctl=ctl, hist=hist[entry], idx=[3, 5, 7], kp=kp, states=st, G=G, bank=bank._b, nets=[0, 1, 0, 1, 0, 1])
            a.update(over)
            if isinstance(a["t"], str):
                a["t"] = {"other_N": tab23._t, "other_del_t": tab_slow._t}[a["t"]]
            if a["kp"] is BAD:
                a["kp"] = kp.data_ptr() + 8
            ints = lambda v: None if v is None else (C.c_int32 * max(len(v), 1))(*v)
            own = {"table": (), "bank": (), "loads": (ptr(a["hist"]),), "boundary": (ptr(a["hist"]),),
                   "keypoints": (ptr(a["hist"]), len(a["idx"]), ints(a["idx"]), ptr(a["kp"]))}[entry]
            mid = (ptr(a["states"]), 0, ptr(a["G"]), None, 0.0, 0, None)
            end = (None, kn.dtype_code(dt), None)
            if entry == "bank":
                rc = h.lib.kr_simulate_batch_bank(h._h, a["t"], a["bank"], ints(a["nets"]), a["T"], kn.KR_EULER, ptr(a["ctl"]), *mid, *end)
            else:
                fn = getattr(h.lib, "kr_simulate_batch_" + entry)
                rc = fn(h._h, a["t"], a["T"], kn.KR_EULER, ptr(a["ctl"]), *own, *mid, 0, *end)
            out[label] = (rc, h.lib.kr_last_error().decode() if rc else None)
        torch.cuda.synchronize()
        assert torch.equal(st, before) and bool((G == 0).all()) and bool((kp == 0).all())  # nothing ran
    return out


# recorded with this list on the build of the commit before the six entry points shared one call body
ARG_ERROR_PAIRS = {
    'table: null table': (-1, 'null pointer argument: t'),
    'table: null ctl': (-1, 'null pointer argument: ctl'),
    'table: null states': (-1, 'null pointer argument: states'),
    'table: null G': (-1, 'null pointer argument: G'),
    'table: T < 0': (-1, 'T < 0'),
    'table: table of another N': (-1, "parameter table: N of the table differs from the handle's"),
    'table: table of another del_t': (-1, "parameter table: del_t of the table differs from the handle's"),
    'table: null table, T < 0': (-1, 'null pointer argument: t'),
    'table: table of another N, T < 0': (-1, "parameter table: N of the table differs from the handle's"),
    'table: table of another N, T = 0': (-1, "parameter table: N of the table differs from the handle's"),
    'table: T < 0, null ctl': (-1, 'T < 0'),
    'table: T = 0, null ctl': (0, None),
    'table: null ctl, null states, null G': (-1, 'null pointer argument: ctl'),
    'table: null states, null G': (-1, 'null pointer argument: states'),
    'loads: null table': (-1, 'null pointer argument: t'),
    'loads: null ctl': (-1, 'null pointer argument: ctl'),
    'loads: null states': (-1, 'null pointer argument: states'),
    'loads: null G': (-1, 'null pointer argument: G'),
    'loads: T < 0': (-1, 'T < 0'),
    'loads: table of another N': (-1, "parameter table: N of the table differs from the handle's"),
    'loads: table of another del_t': (-1, "parameter table: del_t of the table differs from the handle's"),
    'loads: null table, T < 0': (-1, 'null pointer argument: t'),
    'loads: table of another N, T < 0': (-1, "parameter table: N of the table differs from the handle's"),
    'loads: table of another N, T = 0': (-1, "parameter table: N of the table differs from the handle's"),
    'loads: T < 0, null ctl': (-1, 'T < 0'),
    'loads: T = 0, null ctl': (0, None),
    'loads: null ctl, null states, null G': (-1, 'null pointer argument: ctl'),
    'loads: null states, null G': (-1, 'null pointer argument: states'),
    'loads: null history': (-1, 'null pointer argument: loads'),
    'loads: null table, null history': (-1, 'null pointer argument: t'),
    'loads: null history, T < 0': (-1, 'null pointer argument: loads'),
    'loads: null history, table of another N': (-1, 'null pointer argument: loads'),
    'boundary: null table': (-1, 'null pointer argument: t'),
    'boundary: null ctl': (-1, 'null pointer argument: ctl'),
    'boundary: null states': (-1, 'null pointer argument: states'),
    'boundary: null G': (-1, 'null pointer argument: G'),
    'boundary: T < 0': (-1, 'T < 0'),
    'boundary: table of another N': (-1, "parameter table: N of the table differs from the handle's"),
    'boundary: table of another del_t': (-1, "parameter table: del_t of the table differs from the handle's"),
    'boundary: null table, T < 0': (-1, 'null pointer argument: t'),
    'boundary: table of another N, T < 0': (-1, "parameter table: N of the table differs from the handle's"),
    'boundary: table of another N, T = 0': (-1, "parameter table: N of the table differs from the handle's"),
    'boundary: T < 0, null ctl': (-1, 'T < 0'),
    'boundary: T = 0, null ctl': (0, None),
    'boundary: null ctl, null states, null G': (-1, 'null pointer argument: ctl'),
    'boundary: null states, null G': (-1, 'null pointer argument: states'),
    'boundary: null history': (-1, 'null pointer argument: bnd'),
    'boundary: null table, null history': (-1, 'null pointer argument: t'),
    'boundary: null history, T < 0': (-1, 'null pointer argument: bnd'),
    'boundary: null history, table of another N': (-1, 'null pointer argument: bnd'),
    'keypoints: null table': (-1, "kr_simulate_batch_keypoints: null pointer argument: t (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: null ctl': (-1, 'null pointer argument: ctl'),
    'keypoints: null states': (-1, 'null pointer argument: states'),
    'keypoints: null G': (-1, 'null pointer argument: G'),
    'keypoints: T < 0': (-1, 'T < 0'),
    'keypoints: table of another N': (-1, "parameter table: N of the table differs from the handle's"),
    'keypoints: table of another del_t': (-1, "parameter table: del_t of the table differs from the handle's"),
    'keypoints: null table, T < 0': (-1, "kr_simulate_batch_keypoints: null pointer argument: t (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: table of another N, T < 0': (-1, "parameter table: N of the table differs from the handle's"),
    'keypoints: table of another N, T = 0': (-1, "parameter table: N of the table differs from the handle's"),
    'keypoints: T < 0, null ctl': (-1, 'T < 0'),
    'keypoints: T = 0, null ctl': (0, None),
    'keypoints: null ctl, null states, null G': (-1, 'null pointer argument: ctl'),
    'keypoints: null states, null G': (-1, 'null pointer argument: states'),
    'keypoints: null history': (-1, "kr_simulate_batch_keypoints: null pointer argument: bnd (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: null table, null history': (-1, "kr_simulate_batch_keypoints: null pointer argument: t (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: null history, T < 0': (-1, "kr_simulate_batch_keypoints: null pointer argument: bnd (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: null history, table of another N': (-1, "kr_simulate_batch_keypoints: null pointer argument: bnd (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: null kp': (-1, "kr_simulate_batch_keypoints: null pointer argument: kp (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: misaligned kp': (-1, 'kr_simulate_batch_keypoints: kp must be 16-byte aligned'),
    'keypoints: point out of range': (-1, 'kr_simulate_batch_keypoints: idx[2] = 10 lies outside [0, N) = [0, 10)'),
    'keypoints: points not increasing': (-1, 'kr_simulate_batch_keypoints: idx[2] = 5 does not exceed idx[1] = 7 (the key points must be strictly increasing)'),
    'keypoints: no points': (-1, 'kr_simulate_batch_keypoints: K = 0, a call takes 1 <= K <= 16 key points'),
    'keypoints: null kp, point out of range': (-1, "kr_simulate_batch_keypoints: null pointer argument: kp (a caller with a fixed boundary repeats the row's values)"),
    'keypoints: misaligned kp, point out of range': (-1, 'kr_simulate_batch_keypoints: idx[2] = 10 lies outside [0, N) = [0, 10)'),
    'keypoints: point out of range, T < 0': (-1, 'kr_simulate_batch_keypoints: idx[2] = 10 lies outside [0, N) = [0, 10)'),
    'keypoints: misaligned kp, table of another N': (-1, 'kr_simulate_batch_keypoints: kp must be 16-byte aligned'),
    'keypoints: misaligned kp, T < 0': (-1, 'kr_simulate_batch_keypoints: kp must be 16-byte aligned'),
    "keypoints: point of the other table's range, table of another N": (-1, "parameter table: N of the table differs from the handle's"),
    'bank: null table': (-1, 'null pointer argument: t'),
    'bank: null ctl': (-1, 'null pointer argument: ctl'),
    'bank: null states': (-1, 'null pointer argument: states'),
    'bank: null G': (-1, 'null pointer argument: G'),
    'bank: T < 0': (-1, 'T < 0'),
    'bank: table of another N': (-1, "parameter table: N of the table differs from the handle's"),
    'bank: table of another del_t': (-1, "parameter table: del_t of the table differs from the handle's"),
    'bank: null table, T < 0': (-1, 'null pointer argument: t'),
    'bank: table of another N, T < 0': (-1, "parameter table: N of the table differs from the handle's"),
    'bank: table of another N, T = 0': (-1, "parameter table: N of the table differs from the handle's"),
    'bank: T < 0, null ctl': (-1, 'T < 0'),
    'bank: T = 0, null ctl': (0, None),
    'bank: null ctl, null states, null G': (-1, 'null pointer argument: ctl'),
    'bank: null states, null G': (-1, 'null pointer argument: states'),
    'bank: null bank': (-1, 'null pointer argument: bank'),
    'bank: null index array': (-1, 'null pointer argument: net_of_rod_host'),
    'bank: index out of range': (-1, 'network bank: rod 2 asks for network 2, the bank holds 2'),
    'bank: negative index': (-1, 'network bank: rod 1 asks for network -1, the bank holds 2'),
    'bank: null table, null bank': (-1, 'null pointer argument: t'),
    'bank: index out of range, T < 0': (-1, 'network bank: rod 2 asks for network 2, the bank holds 2'),
    'bank: index out of range, T = 0': (-1, 'network bank: rod 2 asks for network 2, the bank holds 2'),
    'bank: table of another N, index out of range': (-1, "parameter table: N of the table differs from the handle's"),
    'bank: index out of range, null ctl': (-1, 'network bank: rod 2 asks for network 2, the bank holds 2'),
}


def test_argument_errors_of_the_c_entry_points(torch_cuda):
    got = arg_error_pairs(torch_cuda)
    assert list(got) == [c[0] for c in arg_error_cases()] and len(got) == len(ARG_ERROR_PAIRS)
    for label, pair in got.items():
        print(label, pair)
    wrong = {k: (v, ARG_ERROR_PAIRS[k]) for k, v in got.items() if v != ARG_ERROR_PAIRS[k]}
    assert not wrong, wrong
