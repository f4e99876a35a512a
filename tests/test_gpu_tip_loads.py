"""Per-step tip loads (kr_simulate_batch_loads) on the MI355X: a wrench history per rod in one simulate call.

Rod b solves step t with ``loads[b, t]`` = F_tip (3), M_tip (3) in place of the wrench of its table row.  The reference
side of a comparison is the fixture tests/golden/tip_loads.npz (the unmodified reference with ``robot.F_tip`` /
``robot.M_tip`` assigned while ``knode.simulate`` draws control t; its last solve is dropped, so T controls give states
0 .. T-1), the oracle's own time loop with the same assignment (tests/tip_loads_cases.py), or the table call on inputs
where both must do the same arithmetic.  Tolerances are the project's own (tests/test_gpu_param_table.py): fp64
``rel_l2 < 1e-8`` against reference-held trajectories, fp32 tips ``< 1e-5``; a wrench taken one step late or early moves
the tips of the ``jump`` / ``alt`` / ``sine`` histories by 4e-3 and more.

Shapes: B = 5 (a partial workgroup of four rods per workgroup), N in {10, 23} (ragged interval lengths), T in {12, 13}
(both step parities at the end of a call).  Every test asserts what ran: one persistent launch, one wavefront per rod,
the overlapped kernel or not as asked."""
import numpy as np
import pytest

from conftest import load_golden, rel_l2
from gpu_helpers import inject, make_robot, set_mode_env
from tip_loads_cases import CASES, SHAPES, load_history, oracle_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODS5 = [None, "damping", "short", "youngs", "noair"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check(label, value, bound):
    print(f"{label}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, f"{label}: {value:.3e} >= {bound:.0e}"


def assert_ran(h, overlap):
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
    assert got == (2, 1, overlap), f"(path, waves per rod, overlap) = {got}, expected (2, 1, {overlap})"


def dev(torch, x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype).contiguous()


def run(torch, h, ctl, dtype, table, loads=None, ring=False, chunks=None, scheme=0, maxit=0, use_nn=False):
    """One call (or one per chunk, the state before handed over) from the straight rod; everything as float64 NumPy."""
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dtype, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dtype, device=DEV)
    tip = torch.empty((B, T, 3), dtype=dtype, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    if chunks is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, loads=loads, scheme=scheme, maxit=maxit,
                   use_nn=use_nn)
    else:
        t0 = 0
        for n in chunks:
            tp = torch.empty((B, n, 3), dtype=dtype, device=DEV)
            sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + n].contiguous(), st[t0:], G, tip=tp, status=sx, prev_init=st[t0 - 1] if t0 else None,
                       table=table, loads=None if loads is None else loads[:, t0:t0 + n].contiguous(), maxit=maxit)
            tip[:, t0:t0 + n] = tp
            status[:, t0:t0 + n] = sx
            t0 += n
    torch.cuda.synchronize()
    return dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
                states=st.double().cpu().numpy())


def unpack(st):
    """packed records [.., N, 28] (q w v u p h n m) -> reference rows [.., 25, N] (p h n m q w v u)"""
    st = np.swapaxes(st, -1, -2)
    return np.concatenate([st[..., 12:25, :], st[..., 0:12, :]], axis=-2)


def sine_ctl(B, T, del_t, seed):
    import cosserat_oracle as orc
    return orc.batch_sine_controls(B, T, del_t, seed)


def wrench_rows(N):
    """five presets, each with a tip wrench of its own"""
    rng = np.random.default_rng(5 + N)
    robots = []
    for m in MODS5:
        r = make_robot(m, N)
        r.F_tip, r.M_tip = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3)
        robots.append(r)
    return robots


# ---------------------------------------------------------------------------
# 1. constant loads are the table call, bit for bit
# ---------------------------------------------------------------------------
def _constant_loads_case(torch, h, robots, dtype, overlap, T, use_nn, seed):
    B = len(robots)
    ctl = dev(torch, sine_ctl(B, T, robots[0].del_t, seed), dtype)
    L = np.stack([np.tile(np.concatenate([r.F_tip, r.M_tip]), (T, 1)) for r in robots])
    with h.param_table([r._params() for r in robots]) as tab:
        for ring in (False, True):
            a = run(torch, h, ctl, dtype, tab, ring=ring, use_nn=use_nn)
            assert_ran(h, overlap)
            b = run(torch, h, ctl, dtype, tab, loads=dev(torch, L, dtype), ring=ring, use_nn=use_nn)
            assert_ran(h, overlap)
            print(f"N={robots[0].N} ring={ring} use_nn={use_nn}: {int((a['status'] != 0).sum())} steps not converged")
            if not use_nn:
                assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            for k in ("status", "tip", "G", "states"):
                assert np.array_equal(a[k], b[k]), f"ring={ring}: {k} differs from the table call"
    # the rows do differ (the comparison is not between five copies of one rod)
    assert rel_l2(a["tip"][1], a["tip"][0]) > 1e-3


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constant_loads_are_the_table_call(torch_cuda, monkeypatch, dtype, overlap):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    for N, T in SHAPES:
        robots = wrench_rows(N)
        h = make_robot(None, N)._native()
        h.set_option("overlap", overlap)
        _constant_loads_case(torch, h, robots, dt, overlap, T, False, 40 + N)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constant_loads_are_the_table_call_mlp_on(torch_cuda, monkeypatch, dtype):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64 if dtype == "f64" else torch.float32
    mlp = orc.mlp_from_arrays(load_golden("bc"), "mlp_elu64")  # (the network of test_gpu_param_table's MLP-on calls)
    for N, T in SHAPES:
        carrier = make_robot(None, N)
        inject(carrier, mlp)
        _constant_loads_case(torch, carrier._native(), wrench_rows(N), dt, 0, T, True, 50 + N)


# ---------------------------------------------------------------------------
# 2. against the reference fixture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("N,T", SHAPES)
def test_against_the_reference_fixture(torch_cuda, monkeypatch, N, T, overlap):
    """The four histories in one batch (rod b gets case b), padded with a zero-load rod that must be the table call."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("tip_loads")
    k = f"_n{N}"
    assert np.all(g["ier" + k] == 1)
    r = make_robot(None, N)
    h = r._native()
    h.set_option("overlap", overlap)
    B = 5
    L = np.concatenate([g["loads" + k], np.zeros((1, T, 6))])
    ctl = np.stack([g["ctl" + k]] * B)
    with h.param_table([r._params()] * B) as tab:
        for dtype in (torch.float64, torch.float32):
            a = run(torch, h, dev(torch, ctl, dtype), dtype, tab, loads=dev(torch, L, dtype))
            assert_ran(h, overlap)
            assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            plain = run(torch, h, dev(torch, ctl, dtype), dtype, tab)
            assert_ran(h, overlap)
            for key in ("tip", "status", "G"):
                assert np.array_equal(a[key][4], plain[key][4]), f"zero-load rod: {key} differs from the table call"
            assert np.array_equal(a["states"][:, 4], plain["states"][:, 4])
            # tip after step t = tip of state t + 1; the fixture holds states 0 .. T-1
            for c, case in enumerate(CASES):
                tips = unpack(a["states"][:T, c])[:, :3, -1]
                if dtype == torch.float64:
                    check(f"N={N} overlap={overlap} {case} tips", rel_l2(tips, g["tips" + k][c]), 1e-8)
                    check(f"N={N} overlap={overlap} {case} tip output", rel_l2(a["tip"][c, :T - 1], g["tips" + k][c][1:]), 1e-8)
                    check(f"N={N} overlap={overlap} {case} state T-1", rel_l2(unpack(a["states"][T - 1, c]), g["last" + k][c]), 1e-8)
                    if N == 10:
                        check(f"N={N} overlap={overlap} {case} trajectory", rel_l2(unpack(a["states"][:T, c]), g["traj" + k][c]), 1e-8)
                else:
                    check(f"N={N} overlap={overlap} {case} fp32 tips", rel_l2(tips, g["tips" + k][c]), 1e-5)


# ---------------------------------------------------------------------------
# 3. against the oracle loop, per-rod constants and loads together
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_oracle():
    import cosserat_oracle as orc
    N, T = 23, 13
    mods = [None, "damping", None, "damping", "damping"]
    cases = ["const", "jump", "alt", "sine", "alt"]
    ctl = orc.batch_sine_controls(5, T, 0.05, 311)
    L = np.stack([load_history(c, T) for c in cases])
    refs = []
    for b in range(5):
        states, ok, _ = oracle_loop(orc.params_for(mods[b], N), ctl[b], L[b])
        assert ok.all(), b
        refs.append(states)
    return N, T, mods, ctl, L, refs


def test_against_the_oracle_with_per_rod_constants(torch_cuda, monkeypatch, mixed_oracle):
    from knode import simulate_batch
    set_mode_env(monkeypatch, "overlap")
    N, T, mods, ctl, L, refs = mixed_oracle
    carrier = make_robot(None, N)
    out = simulate_batch(carrier, ctl, robots=[make_robot(m, N) for m in mods], tip_loads=L)
    assert_ran(carrier._handle, 1)
    assert np.all(out["status"] == 0), np.argwhere(out["status"] != 0)[:8]
    for b in range(5):
        check(f"rod {b} ({mods[b]}) tips", rel_l2(out["tip"][b], refs[b][1:, :3, -1]), 1e-8)
        check(f"rod {b} ({mods[b]}) state T", rel_l2(out["traj"][b, T], refs[b][T]), 1e-8)
    assert rel_l2(out["tip"][4], out["tip"][2]) > 1e-3  # same history, another rod


# ---------------------------------------------------------------------------
# 4. hand-over to the take-over launch
# ---------------------------------------------------------------------------
def test_hand_over_to_second_launch(torch_cuda, monkeypatch):
    """An iteration cap of 2 from the straight rod (tests/test_gpu_overlap.py::test_hand_over_to_second_launch): the
    overlapped kernel gives rods up and the plain persistent kernel takes over at their resume step, where it must load
    that step's wrench."""
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 5
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 77), dt)
    L = dev(torch, np.stack([load_history("alt", T) * (1 + 0.25 * b) for b in range(B)]), dt)
    with h.param_table([r._params()] * B) as tab:
        h.set_option("overlap", 1)
        a = run(torch, h, ctl, dt, tab, loads=L, maxit=2)
        assert_ran(h, 1)
        ar = run(torch, h, ctl, dt, tab, loads=L, maxit=2, ring=True)
        assert_ran(h, 1)
        h.set_option("overlap", 0)
        b = run(torch, h, ctl, dt, tab, loads=L, maxit=2)
        assert_ran(h, 0)
        h.set_option("overlap", 1)
        c = run(torch, h, ctl, dt, tab, loads=L)
    print(f"steps not converged at the cap: {int((a['status'] != 0).sum())} of {B * T}")
    assert np.all(a["status"] >= 0) and np.all(a["status"] <= 2)
    assert np.array_equal(a["status"] != 0, b["status"] != 0)
    assert np.all(np.isfinite(a["tip"]))
    check("overlapped + take-over against the plain kernel, tips", rel_l2(a["tip"], b["tip"]), 1e-6)
    assert np.array_equal(ar["status"], a["status"])
    check("ring against full history, tips", rel_l2(ar["tip"], a["tip"]), 1e-9)
    assert np.all(c["status"] == 0)  # with the default cap everything converges again on the same handle


# ---------------------------------------------------------------------------
# 5. calls in pieces
# ---------------------------------------------------------------------------
def test_calls_in_pieces(torch_cuda, monkeypatch):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 13, 5
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 21), dt)
    cases = ["const", "jump", "alt", "sine", "alt"]
    L = dev(torch, np.stack([load_history(c, T) for c in cases]), dt)
    with h.param_table([r._params()] * B) as tab:
        one = run(torch, h, ctl, dt, tab, loads=L)
        assert_ran(h, 1)
        assert np.all(one["status"] == 0)
        for keep in (0, 1):
            h.set_option("keep_predictor", 0)
            h.set_option("keep_predictor", keep)
            try:
                ch = run(torch, h, ctl, dt, tab, loads=L, chunks=[1, 1, 5, 1, 5])
            finally:
                h.set_option("keep_predictor", 0)
            assert_ran(h, 1)
            assert np.all(ch["status"] == 0)
            check(f"keep_predictor={keep} chunks, last state", rel_l2(ch["states"][T][..., :25], one["states"][T][..., :25]), 1e-7)
            check(f"keep_predictor={keep} chunks, tips", rel_l2(ch["tip"], one["tip"]), 1e-7)
        ring = run(torch, h, ctl, dt, tab, loads=L, ring=True)
        assert_ran(h, 1)
    assert np.array_equal(ring["tip"], one["tip"])
    for k in (T, T - 1, T - 2):
        assert np.array_equal(ring["states"][k % 3], one["states"][k]), k


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch_cuda, monkeypatch):
    import ctypes as C
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 23, 12, 5
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, sine_ctl(B, T, r.del_t, 9), dt)
    L = dev(torch, np.stack([load_history("sine", T)] * B), dt)
    SENT = -7.0
    st = h.new_state(B, dt, n_slots=T + 1)
    G = torch.full((B, 6), SENT, dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dt, device=DEV)
    status = torch.full((B, T), -7, dtype=torch.int32, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((st[1:] == 0).all() and (G == SENT).all() and (tip == SENT).all() and (status == -7).all())

    def raw(table, loads, scheme=kn.KR_EULER):
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        return h.lib.kr_simulate_batch_loads(h._h, table, T, scheme, p(ctl), p(loads), p(st), 0, p(G), p(tip), 0.0, 0, p(status),
                                             0, None, kn.dtype_code(dt), None)

    with h.param_table([r._params()] * B) as tab:
        h.init_straight(st[0], table=tab)
        ok = run(torch, h, ctl, dt, tab, loads=L)
        assert_ran(h, 1)
        assert np.all(ok["status"] == 0)
        assert raw(tab._t, None) == kn.KR_E_ARG and "loads" in h.lib.kr_last_error().decode()
        assert raw(None, L) == kn.KR_E_ARG
        assert untouched()
        assert raw(tab._t, L, kn.KR_RK4) == kn.KR_E_UNSUPPORTED
        msg = h.lib.kr_last_error().decode()
        assert "Euler" in msg and "kr_simulate_batch_loads" in msg, msg
        assert untouched()
        h.set_option("waves_per_rod", 4)
        assert raw(tab._t, L) == kn.KR_E_UNSUPPORTED
        msg = h.lib.kr_last_error().decode()
        assert "waves_per_rod" in msg and "kr_simulate_batch_loads" in msg, msg
        assert untouched() and h.get_option("last_waves_per_rod") == 1
        h.set_option("waves_per_rod", 1)
        # the binding: loads need a table, and do not ride with a bank
        with pytest.raises(kn.KrError, match="table"):
            h.simulate(ctl, st, G, loads=L)
        with pytest.raises(kn.KrError, match="bank"):
            h.simulate(ctl, st, G, table=tab, bank=object(), net_of_rod=[0] * B, loads=L)
        assert untouched()
        again = run(torch, h, ctl, dt, tab, loads=L)
        assert_ran(h, 1)
        assert np.array_equal(again["tip"], ok["tip"])


# ---------------------------------------------------------------------------
# 7. Python front end
# ---------------------------------------------------------------------------
def test_simulate_batch_tip_loads(torch_cuda, monkeypatch):
    from knode import simulate_batch
    from krod_eval import dtw_distance, pos_euler_mse
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    N, T, B = 10, 12, 5
    r = make_robot(None, N)
    ctl = sine_ctl(B, T, r.del_t, 5)
    cases = ["const", "jump", "alt", "sine", "alt"]
    L = np.stack([load_history(c, T) for c in cases])
    out = simulate_batch(r, ctl, tip_loads=L)
    h = r._handle
    assert_ran(h, 1)
    assert np.all(out["status"] == 0)
    with h.param_table([r._params()] * B) as tab:
        direct = run(torch, h, dev(torch, ctl, dt), dt, tab, loads=dev(torch, L, dt))
    assert np.array_equal(out["tip"], direct["tip"]) and np.array_equal(out["G"], direct["G"])
    check("trajectory against the direct call's states", rel_l2(out["traj"], unpack(direct["states"]).transpose(1, 0, 2, 3)) + 1e-300, 1e-14)
    # [T, 6] is shared by all rods
    shared = simulate_batch(r, ctl, tip_loads=L[2])
    both = simulate_batch(r, ctl, tip_loads=np.stack([L[2]] * B))
    assert np.array_equal(shared["tip"], both["tip"]) and np.array_equal(shared["traj"], both["traj"])
    assert np.array_equal(shared["tip"][2], out["tip"][2]) and not np.array_equal(shared["tip"][0], out["tip"][0])
    # tip_only keeps the tips
    lean = simulate_batch(r, ctl, tip_loads=L, tip_only=True)
    assert np.array_equal(lean["tip"], out["tip"]) and "traj" not in lean
    # robots=[...] and score={...} together: the scores are those of the returned trajectory
    robots = [make_robot(m, N) for m in MODS5]
    ref = out["traj"][0, :T]
    sc = simulate_batch(r, ctl, robots=robots, tip_loads=L, score={"reference": ref})
    assert_ran(h, 1)
    assert np.all(sc["status"] == 0)
    assert np.array_equal(sc["tip"][0], out["tip"][0]) and rel_l2(sc["tip"][1], out["tip"][1]) > 1e-3
    want_dtw = np.array([dtw_distance(sc["traj"][b, :T, :3, N - 1], ref[:, :3, N - 1]) for b in range(B)])
    assert np.array_equal(sc["dtw"], want_dtw), (sc["dtw"], want_dtw)
    want_mse = np.array([pos_euler_mse(sc["traj"][b, :T], ref) for b in range(B)])
    err = np.abs(sc["mse"][1:] - want_mse[1:]) / want_mse[1:]
    print(f"mse max relative error {err.max():.2e} (bound 1e-10, tests/test_gpu_score.py); dtw {sc['dtw']}")
    assert err.max() <= 1e-10 and sc["mse"][0] == 0.0 and sc["dtw"][0] == 0.0
