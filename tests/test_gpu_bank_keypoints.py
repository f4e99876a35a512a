"""Bank calls with per-step boundary data and key-point records (kr_simulate_batch_bank_keypoints, kr_mlp_bank_repack,
knode.simulate_bank, krod_eval.evaluate_bank, KnodeBankTrainer.evaluate) on the MI355X.

Rod b of one launch runs with row b of a parameter table, network ``net_of_rod[b]`` of a bank, ``bnd[b][t]`` on step t, and
writes the records of K marked grid points.  The reference side of a comparison is the CPU oracle's tightly converged
Newton solver with the rod's own parameters, network, base and load history (tests/bank_keypoints_cases.py: every step
converged; two networks of a bank move the tip by 2-5 %, the network-free rod by 5-11 %), the unmodified reference
(tests/golden/bank_motion.npz), or another call of the library where a result has to be the same BIT FOR BIT: the
kernel is the bank kernel with the key-point kernel's source struct, so each half must reproduce its parent exactly.
Tolerances are the project's own: fp64 ``rel_l2 < 1e-8`` against trajectories, fp32 tip paths ``< 1e-5``
(tests/test_gpu_mlp_bank.py), calls in pieces ``< 1e-7`` and the MSE over key points ``1e-13`` relative
(tests/test_gpu_keypoints.py).

Shapes: B = 6 (two workgroups of four rods, the second partial), N = 20 with sixteen points, N = 100 with both mask words,
T = 13 (lean ring steps and both step parities).  Every served call asserts what ran: one persistent launch, one
wavefront per rod, no overlapped kernel."""
import ctypes as C

import numpy as np
import pytest

import bank_keypoints_cases as cases
from conftest import load_golden, rel_l2
from gpu_helpers import inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
NAME = "kr_simulate_batch_bank_keypoints"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check(label, value, bound):
    print(f"{label}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, f"{label}: {value:.3e} >= {bound:.0e}"


def assert_ran(h):
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
    assert got == (2, 1, 0), f"(path, waves per rod, overlap) = {got}, expected (2, 1, 0)"


def tdtype(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def dev(torch, x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype).contiguous()


def same_bits(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def as_network(mlp):
    return (mlp.weights, mlp.biases, mlp.acts)


def unpack(st):
    """packed records [.., P, 28] (q w v u p h n m) -> reference rows [.., 25, P] (p h n m q w v u)"""
    st = np.swapaxes(st.astype(np.float64), -1, -2)
    return np.concatenate([st[..., 12:25, :], st[..., 0:12, :]], axis=-2)


def run(torch, h, ctl, dtype, table, bnd=None, bank=None, nets=None, idx=None, ring=False, chunks=None, use_nn=False):
    """One call from the straight rod; arrays in the call's dtype.  bank + bnd: the new call (idx None: K = 0); bank alone:
    kr_simulate_batch_bank; bnd + idx without a bank: kr_simulate_batch_keypoints.  chunks: a ring call cut into pieces,
    the last two states of a piece handed to the next (states[0] and state_prev_init), bnd sliced like ctl, kp like tip."""
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dtype, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dtype, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dtype, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    kp = torch.full((T, B, len(idx), 28), SENT, dtype=dtype, device=DEV) if idx is not None else None
    kw = dict(table=table)
    if bank is not None:
        kw.update(bank=bank, net_of_rod=nets)
    else:
        kw.update(use_nn=use_nn)
    pts = lambda k: dict(key_points=idx, kp=k) if idx is not None else {}
    if chunks is None:
        h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, **kw, **({"bnd": bnd} if bnd is not None else {}), **pts(kp))
    else:
        assert ring and sum(chunks) == T
        t0, prev = 0, None
        for n in chunks:
            tp = torch.empty((B, n, 3), dtype=dtype, device=DEV)
            sx = torch.full((B, n), -1, dtype=torch.int32, device=DEV)
            h.simulate(ctl[:, t0:t0 + n].contiguous(), st, G, ring=True, tip=tp, status=sx, prev_init=prev,
                       bnd=bnd[:, t0:t0 + n].contiguous(), **kw, **pts(kp[t0:t0 + n]))
            tip[:, t0:t0 + n] = tp
            status[:, t0:t0 + n] = sx
            last, prev = st[n % 3].clone(), st[(n - 1) % 3].clone()  # the piece's last state and the one before it
            st = h.new_state(B, dtype, n_slots=3)
            st[0] = last
            t0 += n
    torch.cuda.synchronize()
    out = dict(tip=tip.cpu().numpy(), status=status.cpu().numpy(), G=G.cpu().numpy(), states=st.cpu().numpy())
    if kp is not None:
        out["kp"] = kp.cpu().numpy()
        assert not (out["kp"] == SENT).any(), f"{int((out['kp'] == SENT).sum())} sentinel values left in kp"
    return out


def case_inputs(torch, case, dt):
    N, T = case["N"], case["T"]
    carrier = make_robot(None, N)
    rows = [make_robot(r[0], N)._params() for r in case["rows"]]
    ctl = dev(torch, np.stack([cases.banks.controls(T)] * len(rows)), dt)
    return carrier, rows, ctl, dev(torch, cases.bnd_of(case), dt)


def own_rows(N, mods):
    """presets, each with a tilted (non-unit) base, a base velocity and a tip wrench of its own"""
    rng = np.random.default_rng(17 + N)
    robots = []
    for m in mods:
        r = make_robot(m, N)
        r.p0 = rng.normal(0, 0.02, 3)
        r.h0 = np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.08, 4)
        r.q0, r.w0 = rng.normal(0, 0.02, 3), rng.normal(0, 0.05, 3)
        r.F_tip, r.M_tip = rng.normal(0, 0.05, 3), rng.normal(0, 0.002, 3)
        robots.append(r)
    return robots


def rows_bnd(robots, T):
    return np.stack([np.tile(np.concatenate([r.p0, r.h0, r.q0, r.w0, r.F_tip, r.M_tip]).astype(np.float64), (T, 1)) for r in robots])


MODS6 = [r[0] for r in cases.ROWS]


# ---------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------
def against_the_oracle(torch, monkeypatch, case, which, dtype):
    set_mode_env(monkeypatch, "overlap")
    dt = tdtype(torch, dtype)
    N, T = case["N"], case["T"]
    idx = cases.POINTS[N]
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    h = carrier._native()
    nets = cases.nets_of(case, which)
    refs = cases.oracle_case(case, which)
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        full = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx)
        assert_ran(h)
        ring = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=True)
        assert_ran(h)
    assert np.all(full["status"] == 0), np.argwhere(full["status"] != 0)[:8]
    traj = unpack(full["states"]).transpose(1, 0, 2, 3)  # [B, T + 1, 25, N]
    for b, ref in enumerate(refs):  # every rod, none left out
        label = f"{which}-layer bank N={N} {dtype} rod {b} {case['rows'][b]} network {nets[b]}"
        if dtype == "f64":
            check(f"{label} trajectory", rel_l2(traj[b], ref), 1e-8)
        else:
            check(f"{label} fp32 tip path", rel_l2(traj[b, :, :3, -1], ref[:, :3, -1]), 1e-5)
    assert same_bits(full["kp"], full["states"][1:][:, :, idx]), "kp differs from the marked records of the states"
    assert np.all(full["kp"][..., 25:] == 0)  # the pad slots
    for k in ("kp", "tip", "status"):
        assert same_bits(ring[k], full[k]), f"{k} of the ring call differs from the full call's"
    assert same_bits(full["kp"][:, :, -1, 12:15].transpose(1, 0, 2), full["tip"]), "the tip's key point is not the tip"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", [3, 2])
def test_against_the_oracle(torch_cuda, monkeypatch, which, dtype):
    against_the_oracle(torch_cuda, monkeypatch, cases.CASE_SMALL, which, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_against_the_oracle_n100_both_mask_words(torch_cuda, monkeypatch, dtype):
    against_the_oracle(torch_cuda, monkeypatch, cases.CASE_N100, 3, dtype)


# ---------------------------------------------------------------------------
# 2. each half against a merged parent, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constant_rows_without_points_is_the_bank_call(torch_cuda, monkeypatch, dtype, ring):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = tdtype(torch, dtype)
    N, T, which = 20, 13, 3
    robots = own_rows(N, MODS6)
    h = make_robot(None, N)._native()
    nets = [0, 1, 2, 3, 3, 0]
    ctl = dev(torch, np.stack([cases.banks.controls(T)] * 6), dt)
    with h.param_table([r._params() for r in robots]) as tab, h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        parent = run(torch, h, ctl, dt, tab, None, bank, nets, ring=ring)
        assert_ran(h)
        new = run(torch, h, ctl, dt, tab, dev(torch, rows_bnd(robots, T), dt), bank, nets, ring=ring)  # K = 0
        assert_ran(h)
    assert np.all(parent["status"] == 0)
    for k in ("status", "tip", "G", "states"):
        assert same_bits(new[k], parent[k]), f"{k} differs from kr_simulate_batch_bank"


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bank_of_copies_is_the_key_point_call(torch_cuda, monkeypatch, dtype, ring):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = tdtype(torch, dtype)
    case = cases.CASE_SMALL
    N, T, idx = case["N"], case["T"], cases.POINTS[case["N"]]
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    mlp = cases.bank(3)[1]
    inject(carrier, mlp)
    h = carrier._native()  # (the handle's own MLP: the parent's network)
    with h.param_table(rows) as tab, h.mlp_bank([as_network(mlp)] * 3) as bank:
        parent = run(torch, h, ctl, dt, tab, bnd, idx=idx, ring=ring, use_nn=True)
        assert_ran(h)
        new = run(torch, h, ctl, dt, tab, bnd, bank, [2, 0, 1, 1, 0, 2], idx=idx, ring=ring)
        assert_ran(h)
    assert np.all(parent["status"] == 0)
    for k in ("status", "tip", "G", "states", "kp"):
        assert same_bits(new[k], parent[k]), f"{k} differs from kr_simulate_batch_keypoints with the handle's MLP"


# ---------------------------------------------------------------------------
# 3. batch independence
# ---------------------------------------------------------------------------
def test_permuted_and_single_rods(torch_cuda, monkeypatch):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    case, which = cases.CASE_SMALL, 3
    N, T, idx = case["N"], case["T"], cases.POINTS[case["N"]]
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    h = carrier._native()
    nets = cases.nets_of(case, which)
    perm = [4, 2, 0, 5, 1, 3]
    with h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        with h.param_table(rows) as tab:
            want = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=True)
        with h.param_table([rows[p] for p in perm]) as tab:
            got = run(torch, h, ctl[perm].contiguous(), dt, tab, bnd[perm].contiguous(), bank, [nets[p] for p in perm], idx=idx, ring=True)
        assert_ran(h)
        for k in ("status", "tip", "G"):
            assert same_bits(got[k], want[k][perm]), f"{k}: permuting the rods does not permute the output"
        assert same_bits(got["kp"], want["kp"][:, perm]) and same_bits(got["states"], want["states"][:, perm])
        for b in (1, 5):  # a rod alone: another grid, another place in its workgroup
            with h.param_table([rows[b]]) as tab:
                one = run(torch, h, ctl[b:b + 1].contiguous(), dt, tab, bnd[b:b + 1].contiguous(), bank, [nets[b]], idx=idx, ring=True)
            for k in ("status", "tip", "G"):
                assert same_bits(one[k], want[k][b:b + 1]), f"rod {b} alone: {k} differs from its result in the batch"
            assert same_bits(one["kp"], want["kp"][:, b:b + 1])


# ---------------------------------------------------------------------------
# 4. calls in pieces
# ---------------------------------------------------------------------------
def test_calls_in_pieces(torch_cuda, monkeypatch):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    case, which = cases.CASE_SMALL, 3
    N, T, idx = case["N"], case["T"], cases.POINTS[case["N"]]
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    h = carrier._native()
    nets = cases.nets_of(case, which)
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        one = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=True)
        assert_ran(h)
        assert np.all(one["status"] == 0)
        for keep in (0, 1):
            h.set_option("keep_predictor", 0)
            h.set_option("keep_predictor", keep)
            try:
                ch = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=True, chunks=[5, 4, 4])
            finally:
                h.set_option("keep_predictor", 0)
            assert_ran(h)
            assert np.all(ch["status"] == 0)
            check(f"keep_predictor={keep} pieces 5 + 4 + 4, kp", rel_l2(ch["kp"][..., :25], one["kp"][..., :25]), 1e-7)
            check(f"keep_predictor={keep} pieces 5 + 4 + 4, tip", rel_l2(ch["tip"], one["tip"]), 1e-7)
            assert same_bits(ch["kp"][:, :, -1, 12:15].transpose(1, 0, 2), ch["tip"])


# ---------------------------------------------------------------------------
# 5. a failing rod
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
def test_nan_tension_fails_one_rod_from_that_step(torch_cuda, monkeypatch, ring):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    case, which = cases.CASE_SMALL, 3
    N, T, idx = case["N"], case["T"], cases.POINTS[case["N"]]
    B, t0, sick = 6, 5, 1
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    h = carrier._native()
    nets = cases.nets_of(case, which)
    bad = ctl.clone()
    bad[sick, t0, 1] = float("nan")
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        want = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=ring)
        assert np.all(want["status"] == 0)
        got = run(torch, h, bad, dt, tab, bnd, bank, nets, idx=idx, ring=ring)  # (run: no sentinel is left in kp)
        assert_ran(h)
        again = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx, ring=ring)
    print(f"ring={ring}: status of rod {sick}: {got['status'][sick].tolist()}")
    assert np.all(got["status"][sick, :t0] == 0) and got["status"][sick, t0] == 2 and np.all(got["status"][sick, t0 + 1:] != 0)
    others = [b for b in range(B) if b != sick]
    assert same_bits(got["kp"][:, others], want["kp"][:, others]), "kp of another rod differs from the clean call"
    assert same_bits(got["kp"][:t0, sick], want["kp"][:t0, sick]), "kp of the failing rod before t0 differs from the clean call"
    for k in ("status", "tip", "G"):
        assert same_bits(got[k][others], want[k][others]), f"{k} of another rod differs from the clean call"
    assert same_bits(got["states"][:, others], want["states"][:, others]), "states of another rod differ from the clean call"
    for k in ("status", "tip", "G", "states", "kp"):  # nothing of the failure stays behind in the handle
        assert same_bits(again[k], want[k]), f"{k} of the next call differs from the clean call"


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch_cuda, monkeypatch):
    import cosserat_oracle as orc
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    T, B, N = 12, 6, 23
    idx = [3, 5, 7, 9]
    r = make_robot(None, N)
    h = r._native()
    ctl = dev(torch, np.stack([cases.banks.controls(T)] * B), dt)
    bnd = dev(torch, np.stack([np.hstack([cases.base_history("slide", T), cases.load_history("sine", T)])] * B), dt)
    st = h.new_state(B, dt, n_slots=T + 1)
    G = torch.full((B, 6), SENT, dtype=dt, device=DEV)
    tip = torch.full((B, T, 3), SENT, dtype=dt, device=DEV)
    status = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    kp = torch.full((T, B, len(idx), 28), SENT, dtype=dt, device=DEV)
    nets_ok = [0, 1, 2, 3, 3, 0]

    def untouched():
        torch.cuda.synchronize()
        return bool((st[1:] == 0).all() and (G == SENT).all() and (tip == SENT).all() and (status == -7).all() and (kp == SENT).all())

    def raw(table, bank, nets=nets_ok, ctl_=ctl, bnd_=bnd, pts=idx, kp_=kp, st_=st, G_=G, scheme=kn.KR_EULER, K=None):
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        arr = (C.c_int32 * max(len(pts), 1))(*pts) if pts is not None else None
        na = (C.c_int32 * B)(*nets) if nets is not None else None
        return h.lib.kr_simulate_batch_bank_keypoints(h._h, table, bank, na, T, scheme, p(ctl_), p(bnd_), (len(pts) if K is None else K), arr,
                                                      p(kp_), p(st_), 0, p(G_), p(tip), 0.0, 0, p(status), None, kn.dtype_code(dt), None)

    def last():
        return tuple(h.get_option(o) for o in ("last_sim_path", "last_waves_per_rod", "last_overlap"))

    def refused(rc, code, *words, named=True):
        msg = h.lib.kr_last_error().decode()
        assert rc == code, (rc, msg)
        assert (NAME in msg or not named) and all(w in msg for w in words), msg

    with h.param_table([r._params()] * B) as tab, h.mlp_bank([as_network(m) for m in cases.bank(3)]) as bank:
        ok = run(torch, h, ctl, dt, tab, bnd, bank, nets_ok, idx=idx)
        assert_ran(h)
        assert np.all(ok["status"] == 0)
        h.init_straight(st[0], table=tab)
        before = last()
        t_, b_ = tab._t, bank._b
        # each NULL
        refused(raw(None, b_), kn.KR_E_ARG, "null pointer argument: t")
        refused(raw(t_, None), kn.KR_E_ARG, "null pointer argument: bank")
        refused(raw(t_, b_, nets=None), kn.KR_E_ARG, "null pointer argument: net_of_rod_host")
        refused(raw(t_, b_, bnd_=None), kn.KR_E_ARG, "null pointer argument: bnd")
        refused(raw(t_, b_, kp_=None), kn.KR_E_ARG, "null pointer argument: kp")
        refused(raw(t_, b_, pts=None, K=4), kn.KR_E_ARG, "null pointer argument: idx")
        refused(raw(t_, b_, ctl_=None), kn.KR_E_ARG, "ctl", named=False)
        refused(raw(t_, b_, st_=None), kn.KR_E_ARG, "states", named=False)
        refused(raw(t_, b_, G_=None), kn.KR_E_ARG, "G", named=False)
        assert untouched() and last() == before
        # K = 0 takes neither idx nor kp
        refused(raw(t_, b_, pts=[], kp_=kp), kn.KR_E_ARG, "K = 0")
        # a bad network index: the first bad rod named
        refused(raw(t_, b_, nets=[0, 1, 4, 3, -1, 0]), kn.KR_E_ARG, "rod 2 asks for network 4", "the bank holds 4")
        refused(raw(t_, b_, nets=[0, 1, 2, 3, -1, 0]), kn.KR_E_ARG, "rod 4 asks for network -1")
        # the point set: the rule of kr_keypoints_check, the first bad entry named
        refused(raw(t_, b_, pts=list(range(17))), kn.KR_E_ARG, "K = 17")
        refused(raw(t_, b_, pts=[3, 5, 5, 9]), kn.KR_E_ARG, "idx[2] = 5")
        refused(raw(t_, b_, pts=[3, 5, 7, 23]), kn.KR_E_ARG, "idx[3] = 23", "[0, 23)")
        refused(raw(t_, b_, pts=[-1, 5, 7, 9]), kn.KR_E_ARG, "idx[0] = -1")
        assert untouched() and last() == before
        # what the bank call refuses
        refused(raw(t_, b_, scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, "Euler")
        assert untouched() and last() == before
        h.set_option("waves_per_rod", 2)
        refused(raw(t_, b_), kn.KR_E_UNSUPPORTED, "waves_per_rod = 2", "bank key-point calls run one wavefront per rod")
        assert untouched() and last() == before
        h.set_option("waves_per_rod", 1)
        h.set_option("persistent", 0)
        refused(raw(t_, b_), kn.KR_E_UNSUPPORTED, "persistent = 0")
        assert untouched() and last() == before
        h.set_option("persistent", 1)
        # a bank shape the kernel does not evaluate cannot be made (the rule of kr_mlp_bank_create, host arithmetic)
        wide = orc.make_mlp([28, 96, 64, 25], "elu", seed=3)
        with pytest.raises(kn.KrError) as e:
            h.mlp_bank([as_network(wide)])
        assert e.value.code == kn.KR_E_UNSUPPORTED and "at most 64 with three layers" in str(e.value)
        # ... and a bank that exists is refused where the handle cannot evaluate it on the matrix cores
        h.set_option("mfma_mlp", 0)
        refused(raw(t_, b_), kn.KR_E_UNSUPPORTED, "a network shape the persistent one-wavefront kernel does not evaluate")
        assert untouched() and last() == before
        h.set_option("mfma_mlp", 1)
        again = run(torch, h, ctl, dt, tab, bnd, bank, nets_ok, idx=idx)
        assert_ran(h)
        assert same_bits(again["kp"], ok["kp"]) and same_bits(again["tip"], ok["tip"])
        # N - 1 < 8 and N = 129: no table of that N can be made for the call to take (the planner's own refusal of both,
        # worded for this call, is held in tests/test_bank_keypoints_cpu.py), and a table of another N is refused by the handle
        for n_bad in (8, 129):
            rb = make_robot(None, n_bad)
            with pytest.raises(kn.KrError, match=rf"N = {n_bad}.*9 <= N <= 128"):
                rb._native().param_table([rb._params()] * B)
        with make_robot(None, 20)._native().param_table([make_robot(None, 20)._params()] * B) as other:
            rc = raw(other._t, b_)
            assert rc == kn.KR_E_ARG, (rc, h.lib.kr_last_error().decode())
        assert untouched() and last() == before


# ---------------------------------------------------------------------------
# 7. the reference
# ---------------------------------------------------------------------------
def test_against_the_reference_fixture(torch_cuda, monkeypatch):
    """bank_motion.npz: four rods over three networks at N = 10, every grid point marked, on a ring: kp[t] is state t + 1,
    and the fixture holds states 0 .. T-1."""
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("bank_motion")
    N, idx = 10, cases.POINTS[10]
    B, T = g["bnd"].shape[0], g["ctl"].shape[0]
    assert np.all(g["ier"] == 1) and g["traj"].shape == (B, T, 25, N)
    mods = [None if m == "None" else str(m) for m in g["mods"]]
    h = make_robot(None, N)._native()
    nets = [orc.mlp_from_arrays(g, f"net{k}") for k in range(int(g["nets"].max()) + 1)]
    with h.param_table([make_robot(m, N)._params() for m in mods]) as tab, h.mlp_bank([as_network(m) for m in nets]) as bank:
        for dtype in (torch.float64, torch.float32):
            a = run(torch, h, dev(torch, np.stack([g["ctl"]] * B), dtype), dtype, tab, dev(torch, g["bnd"], dtype), bank,
                    g["nets"].tolist(), idx=idx, ring=True)
            assert_ran(h)
            assert np.all(a["status"] == 0), np.argwhere(a["status"] != 0)[:8]
            got = unpack(a["kp"]).transpose(1, 0, 2, 3)  # [B, T, 25, N]
            for b in range(B):
                if dtype == torch.float64:
                    check(f"rod {b} ({mods[b]}, network {g['nets'][b]}) trajectory", rel_l2(got[b, :T - 1], g["traj"][b][1:]), 1e-8)
                else:
                    check(f"rod {b} ({mods[b]}, network {g['nets'][b]}) fp32 tips", rel_l2(got[b, :T - 1, :3, -1], g["tips"][b][1:]), 1e-5)


# ---------------------------------------------------------------------------
# 8. Python
# ---------------------------------------------------------------------------
def python_robots(case, which, zero=()):
    robots = []
    for b, row in enumerate(case["rows"]):
        r = make_robot(row[0], case["N"])
        if b not in zero:
            inject(r, cases.bank(which)[cases.net_index(which, row[3])])
        robots.append(r)
    return robots


def test_simulate_bank_is_the_c_call(torch_cuda, monkeypatch):
    from knode import simulate_bank
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    case, which = cases.CASE_SMALL, 3
    N, T, idx = case["N"], case["T"], cases.POINTS[case["N"]]
    carrier, rows, ctl, bnd = case_inputs(torch, case, dt)
    h = carrier._native()
    nets = cases.nets_of(case, which)
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank(which)]) as bank:
        want = run(torch, h, ctl, dt, tab, bnd, bank, nets, idx=idx)
    robots = python_robots(case, which)
    hist = cases.bnd_of(case)
    out = simulate_bank(carrier, robots, ctl.cpu().numpy(), base_motion=hist[:, :, :13], tip_loads=hist[:, :, 13:], key_points=idx)
    assert_ran(carrier._handle)
    assert out["n_networks"] == 4 and out["key_points"].tolist() == idx
    assert same_bits(out["tip"], want["tip"]) and same_bits(out["status"], want["status"]) and same_bits(out["G"], want["G"])
    assert same_bits(out["traj"], np.ascontiguousarray(unpack(want["states"]).transpose(1, 0, 2, 3)))
    assert same_bits(out["kp"][:, 1:], np.ascontiguousarray(unpack(want["kp"]).transpose(1, 0, 2, 3)))
    # a zero-network rod next to trained ones: the oracle without a network
    zero = (2, 4)
    out0 = simulate_bank(carrier, python_robots(case, which, zero), ctl.cpu().numpy(), base_motion=hist[:, :, :13], tip_loads=hist[:, :, 13:])
    assert_ran(carrier._handle)
    assert np.all(out0["status"] == 0) and out0["n_networks"] == 4  # three of the bank's in use and the zero network
    for b, row in enumerate(case["rows"]):
        ref = cases.oracle_rod(N, T, row[0], row[1], row[2], which, None if b in zero else cases.net_index(which, row[3]))
        check(f"rod {b} {'without a network' if b in zero else 'trained'}", rel_l2(out0["traj"][b], ref), 1e-8)
        if b not in zero:
            assert same_bits(out0["traj"][b], out["traj"][b])


def test_simulate_bank_scores_on_the_device(torch_cuda, monkeypatch):
    from knode import simulate_bank
    from krod_eval import dtw_distance, evaluate_bank, pos_euler_mse
    set_mode_env(monkeypatch, "overlap")
    case, which = cases.CASE_SMALL, 3
    N, T = case["N"], case["T"]
    pts = [2, 6, 9, -1]
    carrier = make_robot(None, N)
    robots = python_robots(case, which)
    ctl = np.stack([cases.banks.controls(T)] * len(robots))
    hist = cases.bnd_of(case)
    kw = dict(base_motion=hist[:, :, :13], tip_loads=hist[:, :, 13:], key_points=pts)
    full = simulate_bank(carrier, robots, ctl, **kw)
    ref = cases.oracle_rod(N, T, None, "still", "const", which, None)  # a recorded run that is none of the rods'
    lean = simulate_bank(carrier, robots, ctl, tip_only=True, score={"reference": ref, "point": -1}, **kw)
    assert_ran(carrier._handle)
    assert "traj" not in lean and "mse" not in lean
    assert same_bits(lean["kp"], full["kp"]) and same_bits(lean["tip"], full["tip"])
    kp = lean["kp"]  # [B, T + 1, 25, K]
    ref_kp = ref[:, :, lean["key_points"]]
    host_dtw = np.array([dtw_distance(kp[b][:, :3, -1], ref_kp[:, :3, -1]) for b in range(len(robots))])
    assert same_bits(lean["dtw"], host_dtw), (lean["dtw"], host_dtw)
    want = np.array([pos_euler_mse(kp[b], ref_kp) for b in range(len(robots))])
    assert np.all(want >= 1e-2), want  # (squared differences large enough for a relative bound to mean something)
    rel = np.abs(lean["mse_kp"] - want) / want
    print(f"mse_kp against pos_euler_mse on kp, relative errors {rel} (bound 1e-13); mse {want}")
    assert float(np.max(rel)) <= 1e-13, (lean["mse_kp"], want)
    d, m = evaluate_bank(carrier, robots, ctl, ref, pts)  # (its boundary: the rows' own, on every step)
    plain = simulate_bank(carrier, robots, ctl, tip_only=True, key_points=pts, score={"reference": ref, "point": -1})
    assert same_bits(d, plain["dtw"]) and same_bits(m, plain["mse_kp"])


# ---------------------------------------------------------------------------
# 9. the trainer
# ---------------------------------------------------------------------------
def test_bank_trainer_evaluates_its_live_weights(torch_cuda, monkeypatch):
    from cosserat_ode_torch import CosseratRodTorch
    from knode import setup_robot, simulate_bank
    from krod_train import KnodeBankTrainer
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    g = load_golden("train_step")
    traj, ctl = torch.tensor(g["traj"], device=DEV), torch.tensor(g["controls"], device=DEV)
    mods = ("nsw", "short")
    robots = []
    for k, mod in enumerate(mods):
        torch.manual_seed(40 + k)
        rob = CosseratRodTorch(DEV, 64)
        setup_robot(rob, mod)
        rob.N = 10
        rob.compute_intermediate_terms()
        robots.append(rob)
    trainer = KnodeBankTrainer(robots, [traj[None]] * 2, [ctl[None]] * 2, [3, 5, 7, 9])
    trainer.run(3)
    T, pts = 12, [3, 5, 7, 9]
    controls = np.stack([g["controls"][:T].astype(np.float64)] * 2)
    reference = g["traj"][:T + 1].astype(np.float64)

    def by_simulate_bank():
        """the same rods with the weights read back from the robots, through a freshly created bank"""
        for rob in robots:
            rob.nn_model = rob.nn_models
            rob.param_ls = [t.detach().cpu().numpy() for _, t in rob.nn_models.state_dict().items()]
            rob.nn_path = "whatever"
        out = simulate_bank(robots[0], robots, controls, tip_only=True, key_points=pts, score={"reference": reference, "point": -1})
        print(f"steps not converged: {int((out['status'] != 0).sum())}")
        return out["dtw"], out["mse_kp"]

    first = trainer.evaluate(controls, reference, pts)
    assert_ran(trainer.h)
    want = by_simulate_bank()
    assert same_bits(first[0], want[0]) and same_bits(first[1], want[1]), (first, want)
    assert first[0].shape == (2,) and np.all(np.isfinite(first[0])) and np.all(first[1] > 0)
    bank_object = trainer._eval_bank
    trainer.run(3)
    second = trainer.evaluate(controls, reference, pts)  # the repacked bank
    assert trainer._eval_bank is bank_object
    want = by_simulate_bank()  # a freshly created one
    assert same_bits(second[0], want[0]) and same_bits(second[1], want[1]), (second, want)
    print(f"dtw {first[0]} -> {second[0]}, mse_kp {first[1]} -> {second[1]}")
    assert not np.array_equal(first[0], second[0]) and not np.array_equal(first[1], second[1])  # the repack is seen
    trainer.close()
