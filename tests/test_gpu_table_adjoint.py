"""The step adjoint of a heterogeneous batch on the MI355X (kr_step_vjp_table_batch, kr_simulate_vjp_table_batch, krod_grad's
table forms): rod b with row b of a parameter table, the boundary gradient per step.

Steps are held to the EXISTING fixtures - step_adjoint.npz and param_adjoint.npz, finite differences of the oracle's step - with
rods of different parameter sets in ONE table call on a carrier handle whose own parameters belong to no row; rollouts to
table_adjoint.npz (tests/golden/make_golden_table_adjoint.py: three rods at N = 9, each with its own controls and boundary
history).  Every comparison is per block under the project's rule (ten times the H / 2 H disagreement plus the quotient's
floor); every figure is printed before it is asserted.  Forward states are produced on the device with tol = 1e-12.
Measured (MI355X, this file): largest error / tolerance 0.30 over the step blocks and 0.34 over the rollout blocks; a table of
identical rows against kr_step_vjp_par_batch on that handle (`bc`, N = 10): every output bit for bit the same."""
import ctypes as C

import numpy as np
import pytest

import param_adjoint_cases as pc
import step_adjoint_cases as sc
import table_adjoint_cases as tc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OTHERS = ("g_cur", "g_prev", "g_tensions", "g_bnd", "resid", "status")
ALL = OTHERS + ("g_par",)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fx():
    return load_golden("step_adjoint")


@pytest.fixture(scope="module")
def fp():
    return load_golden("param_adjoint")


@pytest.fixture(scope="module")
def ft():
    return load_golden("table_adjoint")


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype or torch.float64).contiguous()


def same_bits(torch, a, b, names=OTHERS):
    return all(torch.equal(a[k], b[k]) for k in names)


def pick(out, idx, names=ALL):
    return {k: out[k][idx] for k in names if out.get(k) is not None}


_steps = {}


def het_step_batch(torch, fx, rods, N):
    """One heterogeneous batch: rods = [(set, fixture rod, state)].  Each set's OWN handle produces the forward step of its rods
    (tol 1e-12, held to the oracle's); the table holds one row per rod and is made on the carrier's handle.
    -> (carrier handle, table, fixture keys, prev, cur, nxt, tens, the rods' robots)"""
    key = (tuple(rods), N)
    if key in _steps:
        return _steps[key]
    keys = [pc.step_key(ps, N, rod, state) for ps, rod, state in rods]
    prev = _dev(torch, np.stack([fx[k + "prev"] for k in keys]))
    cur = _dev(torch, np.stack([fx[k + ("prev" if st == "straight" else "cur")] for k, (_, _, st) in zip(keys, rods)]))
    tens = _dev(torch, np.stack([fx[k + "tens"] for k in keys]))
    nxt = torch.zeros_like(prev)
    for b, (ps, rod, state) in enumerate(rods):
        h = tc.robot_for(ps, N)._native()
        G = torch.zeros((1, 6), dtype=torch.float64, device=DEV)
        status = torch.ones((1,), dtype=torch.int32, device=DEV)
        one = torch.zeros_like(prev[b:b + 1])
        h.step(prev[b:b + 1].contiguous(), cur[b:b + 1].contiguous(), one, G, tens[b:b + 1].contiguous(), tol=1e-12, status=status)
        assert int(status[0]) == 0 and np.max(np.abs(one[0].cpu().numpy() - fx[keys[b] + "next"])) < 1e-9
        nxt[b] = one[0]
    robots = [tc.robot_for(ps, N) for ps, _, _ in rods]
    hc = tc.carrier_for(N)._native()
    table = hc.param_table([r._params() for r in robots])
    _steps[key] = (hc, table, keys, prev, cur, nxt, tens, robots)
    return _steps[key]


def got_vector(out, b):
    return np.concatenate([out["g_cur"][b, :, :12].cpu().numpy().ravel(), out["g_prev"][b, :, :12].cpu().numpy().ravel(),
                           out["g_tensions"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy()])


def assert_step_blocks(fx, fp, out, keys, nxt, gbar, c, N, label, worst):
    """every rod of a table step call against its own fixture entries: the input blocks under sc.block_report, g_par (the
    first two cotangents) under pc.assert_blocks"""
    for b, k in enumerate(keys):
        floor = sc.fd_floor(gbar[b], nxt[b].cpu().numpy())
        for name, err, tol, size in sc.block_report(got_vector(out, b), fx[k + "fd_h"][c], fx[k + "fd_2h"][c], N, floor):
            print(f"{label} rod {b} cot {c} {name:14s} err {err:.3e} tol {tol:.3e} size {size:.3e} ratio {err / tol:.3f}")
            worst["step"] = max(worst.get("step", 0.0), err / tol)
            assert err <= tol, (label, b, c, name, err, tol)
        if c < pc.N_COT:
            wp = {}
            pc.assert_blocks(out["g_par"][b].cpu().numpy(), fp[k + "fd_h"][c], fp[k + "fd_2h"][c], fp[k + "floor"][c], f"{label} rod {b} cot {c}", wp)
            worst["step"] = max([worst.get("step", 0.0)] + list(wp.values()))


_worst = {}
HET10 = [("plain", 0, "sine30"), ("bc", 1, "sine30"), ("noair", 2, "sine30"), ("plain", 0, "straight")]
HET33 = [("plain", 0, "sine30"), ("bc", 1, "sine30")]


@pytest.mark.parametrize("N,rods", [(10, HET10), (33, HET33)])
def test_step_table_against_the_existing_fixtures(torch_cuda, fx, fp, N, rods):
    """1. Rods of `plain`, `bc`, `noair` (and `plain` from the straight rod) in ONE table call on a carrier handle: every rod's
    g_cur, g_prev, g_tensions, g_bnd against its own entries of step_adjoint.npz, its g_par against param_adjoint.npz."""
    torch = torch_cuda
    hc, table, keys, prev, cur, nxt, tens, _ = het_step_batch(torch, fx, rods, N)
    for c in range(3):
        gbar = np.stack([fx[k + "gbar"][c] for k in keys])
        out = hc.step_vjp_table(table, prev, cur, nxt, tens, _dev(torch, gbar), need_par=True)
        assert (out["status"] == 0).all() and tuple(out["g_par"].shape) == (len(rods), pc.KR_PAR)
        assert float(out["resid"].max()) <= 1e-9
        assert_step_blocks(fx, fp, out, keys, nxt, gbar, c, N, f"N={N}", _worst)
    print("largest error / tolerance so far:", {k: round(v, 3) for k, v in _worst.items()})


def test_position_independence(torch_cuda, fx):
    """2. B = 3 against the same rods inside B = 5 (four rods per workgroup: the last workgroup is ragged, and the table holds
    exactly B rows - none beyond may be read); the same with rods and rows permuted together; B = 70 cycling the three sets.
    Every output of a rod is the same bits wherever it rides."""
    torch = torch_cuda
    hc, table5, keys, prev, cur, nxt, tens, robots = het_step_batch(torch, fx, HET10 + [("bc", 0, "sine30")], 10)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    args = (prev, cur, nxt, tens, g_next)
    out5 = hc.step_vjp_table(table5, *args, need_par=True)
    assert (out5["status"] == 0).all()
    with hc.param_table([r._params() for r in robots[:3]]) as table3:
        out3 = hc.step_vjp_table(table3, *[a[:3].contiguous() for a in args], need_par=True)
        assert same_bits(torch, out3, pick(out5, slice(0, 3)), ALL)
    perm = [3, 0, 4, 2, 1]
    with hc.param_table([robots[i]._params() for i in perm]) as tablep:
        outp = hc.step_vjp_table(tablep, *[a[perm].contiguous() for a in args], need_par=True)
        assert same_bits(torch, outp, pick(out5, perm), ALL)
    idx = [b % 3 for b in range(70)]
    with hc.param_table([robots[i]._params() for i in idx]) as table70:
        out70 = hc.step_vjp_table(table70, *[a[idx].contiguous() for a in args], need_par=True)
        assert (out70["status"] == 0).all() and same_bits(torch, out70, pick(out5, idx), ALL)
        torch.cuda.synchronize()


def test_form_equivalences(torch_cuda, fx, fp):
    """3. With g_par against without it: the other outputs bit for bit.  fp32 is the fp64 call on the upcast inputs, rounded.
    A table of identical rows equal to a handle's parameters against kr_step_vjp_par_batch on that handle: each held to the
    finite differences; their largest difference is printed (bit identity is hoped for, not asserted)."""
    torch = torch_cuda
    hc, table, keys, prev, cur, nxt, tens, robots = het_step_batch(torch, fx, HET10, 10)
    gbar = np.stack([fx[k + "gbar"][0] for k in keys])
    args = (prev, cur, nxt, tens, _dev(torch, gbar))
    with_par, without = hc.step_vjp_table(table, *args, need_par=True), hc.step_vjp_table(table, *args)
    assert "g_par" not in without and same_bits(torch, with_par, without)
    f32 = [a.float().contiguous() for a in args]
    lo = hc.step_vjp_table(table, *f32, need_par=True)
    hi = hc.step_vjp_table(table, *[a.double().contiguous() for a in f32], need_par=True)
    assert (lo["status"] == 0).all() and lo["g_par"].dtype == torch.float32
    for k in ("g_cur", "g_prev", "g_tensions", "g_bnd", "g_par"):
        assert torch.equal(lo[k], hi[k].float()), k
    assert torch.equal(lo["resid"], hi["resid"]) and torch.equal(lo["status"], hi["status"])
    assert same_bits(torch, lo, hc.step_vjp_table(table, *f32))
    # identical rows = the handle's own parameters
    same = [("bc", r, "sine30") for r in range(3)]
    _, _, keys3, p3, c3, n3, t3, _ = het_step_batch(torch, fx, same, 10)
    hb = tc.robot_for("bc", 10)._native()
    gbar3 = np.stack([fx[k + "gbar"][0] for k in keys3])
    g3 = _dev(torch, gbar3)
    with hb.param_table([tc.robot_for("bc", 10)._params()] * 3) as t_same:
        a = hb.step_vjp_table(t_same, p3, c3, n3, t3, g3, need_par=True)
    b = hb.step_vjp(p3, c3, n3, t3, g3, need_par=True)
    w = {}
    assert_step_blocks(fx, fp, a, keys3, n3, gbar3, 0, 10, "identical rows, table", w)
    assert_step_blocks(fx, fp, b, keys3, n3, gbar3, 0, 10, "identical rows, handle", w)
    diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in ALL}
    rel = {k: diff[k] / max(float(b[k].double().abs().max()), 1e-300) for k in ALL}
    print("table of identical rows against kr_step_vjp_par_batch: largest |difference| per output", diff, "relative", rel,
          "bit for bit:", same_bits(torch, a, b, ALL))


_rolls = {}


def rollout_batch(torch, ft, case):
    """The fixture's three rods of `case` in one table call: the forward run is the boundary call on the device from the
    fixture's states[0] (and prev_init), held to the oracle's states."""
    if case in _rolls:
        return _rolls[case]
    T, with_prev = tc.CASES[case]
    ks = [tc.key(b, case) for b in range(3)]
    robots = [tc.robot_for(ps, tc.N_FIX) for ps in tc.SETS]
    hc = tc.carrier_for(tc.N_FIX)._native()
    table = hc.param_table([r._params() for r in robots])
    ctl = _dev(torch, np.stack([ft[k + "ctl"] for k in ks]))
    bnd = _dev(torch, np.stack([ft[k + "bnd"] for k in ks]))
    prev_init = _dev(torch, np.stack([ft[k + "prev_init"] for k in ks])) if with_prev else None
    states = hc.new_state(3, torch.float64, n_slots=T + 1)
    states[0] = _dev(torch, np.stack([ft[k + "state0"] for k in ks]))
    G = torch.zeros((3, 6), dtype=torch.float64, device=DEV)
    status = torch.ones((3, T), dtype=torch.int32, device=DEV)
    hc.simulate(ctl, states, G, ring=False, status=status, tol=1e-12, table=table, bnd=bnd, prev_init=prev_init)
    assert (status == 0).all(), status
    for b, k in enumerate(ks):
        miss = float(np.max(np.abs(states[:, b].cpu().numpy() - ft[k + "states"])))
        print(f"{k} device forward against the oracle's states: {miss:.2e}")
        assert miss < 1e-9
    _rolls[case] = (hc, table, ks, ctl, bnd, states, prev_init, robots)
    return _rolls[case]


def composition(torch, h, table, ctl, states, g, prev_init=None):
    """kr_simulate_vjp_table_batch as the header defines it: the loop of kr_step_vjp_table_batch calls; g_bnd kept per step"""
    B, T = ctl.shape[0], ctl.shape[1]
    g = g.clone()
    g_ctl = torch.zeros((B, T, 4), dtype=ctl.dtype, device=DEV)
    g_bnd = torch.zeros((B, T, 19), dtype=ctl.dtype, device=DEV)
    g_par = torch.zeros((B, pc.KR_PAR), dtype=ctl.dtype, device=DEV)
    resid = torch.zeros((B, T), dtype=torch.float64, device=DEV)
    status = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    g_prev_init = None
    for t in range(T - 1, -1, -1):
        prev = states[t - 1] if t > 0 else (prev_init if prev_init is not None else states[0])
        o = h.step_vjp_table(table, prev, states[t], states[t + 1], ctl[:, t].contiguous(), g[t + 1], need_par=True)
        g[t] += o["g_cur"]
        if t > 0 or prev_init is None:
            g[max(t - 1, 0)] += o["g_prev"]
        else:
            g_prev_init = o["g_prev"]
        g_ctl[:, t], g_bnd[:, t] = o["g_tensions"], o["g_bnd"]
        g_par += o["g_par"]
        resid[:, t], status[:, t] = o["resid"], o["status"]
    return dict(g_states=g, g_ctl=g_ctl, g_bnd=g_bnd, g_par=g_par, resid=resid, status=status, g_prev_init=g_prev_init)


@pytest.mark.parametrize("case", list(tc.CASES))
def test_rollout_table_against_the_fixture_and_the_step_calls(torch_cuda, ft, case):
    """4. bnd_per_step = 1: g_ctl, g_bnd[b][t] (six blocks per step), the entries of g_states[0] (and of g_prev_init) and g_par,
    block by block against the fixture, for both cotangents and every rod; the call is bit for bit the loop of step calls;
    bnd_per_step = 0 is the sum of the per-step values from zero, t = T - 1 first, bit for bit."""
    torch = torch_cuda
    T, with_prev = tc.CASES[case]
    hc, table, ks, ctl, bnd, states, prev_init, _ = rollout_batch(torch, ft, case)
    for c in range(2):
        g0 = _dev(torch, np.stack([ft[k + "gbar"][c] for k in ks], axis=1))
        g = g0.clone()
        out = hc.simulate_vjp_table(table, ctl, states, g, prev_init=prev_init, bnd_per_step=True, need_par=True)
        assert (out["status"] == 0).all() and tuple(out["g_bnd"].shape) == (3, T, 19) and float(out["resid"].max()) <= 1e-9
        ref = composition(torch, hc, table, ctl, states, g0, prev_init)
        assert torch.equal(g, ref["g_states"]) and all(torch.equal(out[n], ref[n]) for n in ("g_ctl", "g_bnd", "g_par", "resid", "status"))
        if with_prev:
            assert torch.equal(out["g_prev_init"], ref["g_prev_init"])
        g2 = g0.clone()
        summed = hc.simulate_vjp_table(table, ctl, states, g2, prev_init=prev_init, need_par=True)
        acc = torch.zeros((3, 19), dtype=torch.float64, device=DEV)
        for t in range(T - 1, -1, -1):
            acc = acc + out["g_bnd"][:, t]
        assert tuple(summed["g_bnd"].shape) == (3, 19) and torch.equal(summed["g_bnd"], acc) and torch.equal(g2, g)
        assert all(torch.equal(summed[n], out[n]) for n in ("g_ctl", "g_par", "resid", "status"))
        nobnd = hc.simulate_vjp_table(table, ctl, states, g0.clone(), prev_init=prev_init, need_bnd=False)
        assert nobnd["g_bnd"] is None and "g_par" not in nobnd and torch.equal(nobnd["g_ctl"], out["g_ctl"])
        for b, k in enumerate(ks):
            got = tc.x_got(out["g_ctl"][b].cpu().numpy(), out["g_bnd"][b].cpu().numpy(), g[0, b].cpu().numpy(),
                           out["g_prev_init"][b].cpu().numpy() if with_prev else None)
            wx, wp = {}, {}
            tc.assert_x_blocks(got, ft[k + "x_fd_h"][c], ft[k + "x_fd_2h"][c], ft[k + "x_floor"][c], T, with_prev, f"{k} cot {c}", wx)
            pc.assert_blocks(out["g_par"][b].cpu().numpy(), ft[k + "par_fd_h"][c], ft[k + "par_fd_2h"][c], ft[k + "par_floor"][c],
                             f"{k} cot {c}", wp)
            _worst["rollout"] = max([_worst.get("rollout", 0.0)] + list(wx.values()) + list(wp.values()))
    print("largest error / tolerance so far:", {k: round(v, 3) for k, v in _worst.items()})


def test_failing_rod(torch_cuda, fx, ft):
    """5. One rod's state_next holds a NaN: its status is KR_ST_NONFINITE and its gradients NaN; every other rod is bit for bit
    the clean call; the next call on the handle is clean.  Through the rollout: NaN in that rod's g_bnd[b][t0] and back."""
    torch = torch_cuda
    import krod_native as kn
    hc, table, keys, prev, cur, nxt, tens, _ = het_step_batch(torch, fx, HET10 + [("bc", 0, "sine30")], 10)
    g_next = _dev(torch, np.stack([fx[k + "gbar"][0] for k in keys]))
    clean = hc.step_vjp_table(table, prev, cur, nxt, tens, g_next, need_par=True)
    assert (clean["status"] == 0).all() and bool(torch.isfinite(clean["g_par"]).all())
    bad_next = nxt.clone()
    bad_next[2, 4, 19] = float("nan")
    out = hc.step_vjp_table(table, prev, cur, bad_next, tens, g_next, need_par=True)
    assert out["status"].tolist() == [0, 0, kn.ST_NONFINITE, 0, 0]
    for k in ("g_par", "g_tensions", "g_bnd"):
        assert bool(torch.isnan(out[k][2]).all()), k
    assert bool(torch.isnan(out["g_cur"][2, :, :12]).all()) and torch.count_nonzero(out["g_cur"][2, :, 12:]) == 0
    keep = [0, 1, 3, 4]
    assert same_bits(torch, pick(out, keep), pick(clean, keep), ALL)
    assert same_bits(torch, hc.step_vjp_table(table, prev, cur, nxt, tens, g_next, need_par=True), clean, ALL)
    hr, tab, ks, ctl, bnd, states, _, _ = rollout_batch(torch, ft, "T3")
    g0 = _dev(torch, np.stack([ft[k + "gbar"][0] for k in ks], axis=1))
    o_clean = hr.simulate_vjp_table(tab, ctl, states, g0.clone(), bnd_per_step=True, need_par=True)
    bad = states.clone()
    bad[2, 1, 3, 20] = float("nan")  # states[2] is state_next of step 1 and state_cur of step 2 (slot 20 is read as next only)
    o_bad = hr.simulate_vjp_table(tab, ctl, bad, g0.clone(), bnd_per_step=True, need_par=True)
    assert o_bad["status"][1].tolist() == [kn.ST_NONFINITE, kn.ST_NONFINITE, 0]
    assert bool(torch.isnan(o_bad["g_bnd"][1, :2]).all()) and torch.equal(o_bad["g_bnd"][1, 2], o_clean["g_bnd"][1, 2])
    assert bool(torch.isnan(o_bad["g_par"][1]).all())
    for b in (0, 2):
        assert all(torch.equal(o_bad[n][b], o_clean[n][b]) for n in ("g_ctl", "g_bnd", "g_par"))


def test_refusals_leave_every_output_byte(torch_cuda, fx):
    """6. Each refusal of the header: the (rc, message) pair, nothing launched, and output buffers pre-filled with a pattern
    come back unchanged."""
    torch = torch_cuda
    import krod_native as kn
    hc, table, keys, prev, cur, nxt, tens, robots = het_step_batch(torch, fx, HET10, 10)
    lib, B, N = hc.lib, 4, 10
    g_next = torch.ones_like(nxt)
    full = lambda *shape, dtype=torch.float64: torch.full(shape, 7, dtype=dtype, device=DEV)
    outs = [full(B, N, 28), full(B, N, 28), full(B, 4), full(B, 19), full(B, pc.KR_PAR), full(B), full(B, dtype=torch.int32)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    h33 = tc.carrier_for(33)._native()               # another N
    from gpu_helpers import make_robot
    other_dt = make_robot("youngs", 10)
    other_dt.del_t = 0.025
    other_dt.compute_intermediate_terms()
    hdt = other_dt._native()                          # another del_t

    def step(h=hc._h, t=table._t, scheme=kn.KR_EULER, g=g_next, dtype=kn.KR_F64, cur_=cur, tens_=tens):
        return lib.kr_step_vjp_table_batch(h, t, scheme, p(prev), p(cur_), p(nxt), p(tens_), p(g), *[p(o) for o in outs], dtype, None)
    step_cases = ((dict(h=None), kn.KR_E_ARG, b"null handle"), (dict(t=None), kn.KR_E_ARG, b"kr_step_vjp_table_batch: null parameter table"),
                  (dict(dtype=5), kn.KR_E_ARG, b"dtype"), (dict(g=None), kn.KR_E_ARG, b"null pointer"), (dict(cur_=None), kn.KR_E_ARG, b"null pointer"),
                  (dict(tens_=None), kn.KR_E_ARG, b"null pointer"), (dict(h=h33._h), kn.KR_E_ARG, b"N of the table differs"),
                  (dict(h=hdt._h), kn.KR_E_ARG, b"del_t of the table differs"),
                  (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"kr_step_vjp_table_batch: the adjoint of the RK4 sweep is not served"),
                  # the order KR_ADJ_ARG fixes: the dtype is heard of before a null pointer, a null pointer before the form's refusal
                  (dict(dtype=5, g=None, scheme=kn.KR_RK4), kn.KR_E_ARG, b"dtype"), (dict(g=None, scheme=kn.KR_RK4), kn.KR_E_ARG, b"null pointer"),
                  (dict(h=h33._h, scheme=kn.KR_RK4), kn.KR_E_ARG, b"N of the table differs"))
    for kw, want, word in step_cases:
        rc = step(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    T = 2
    states = torch.zeros((T + 1, B, N, 28), dtype=torch.float64, device=DEV)
    ctl = torch.zeros((B, T, 4), dtype=torch.float64, device=DEV)
    g_states = full(T + 1, B, N, 28)
    souts = [full(B, N, 28), full(B, T, 4), full(B, T, 19)]
    stail = [full(B, pc.KR_PAR), full(B, T), full(B, T, dtype=torch.int32)]

    def sim(h=hc._h, t=table._t, T=T, scheme=kn.KR_EULER, st=states, dtype=kn.KR_F64, per_step=1):
        return lib.kr_simulate_vjp_table_batch(h, t, T, scheme, p(ctl), p(st), None, p(g_states), *[p(o) for o in souts], per_step,
                                               *[p(o) for o in stail], dtype, None)
    sim_cases = ((dict(h=None), kn.KR_E_ARG, b"null handle"), (dict(t=None), kn.KR_E_ARG, b"kr_simulate_vjp_table_batch: null parameter table"),
                 (dict(per_step=2), kn.KR_E_ARG, b"bnd_per_step"), (dict(dtype=-1), kn.KR_E_ARG, b"dtype"), (dict(T=0), kn.KR_E_ARG, b"T < 1"),
                 (dict(st=None), kn.KR_E_ARG, b"null pointer"), (dict(h=h33._h), kn.KR_E_ARG, b"N of the table differs"),
                 (dict(h=hdt._h), kn.KR_E_ARG, b"del_t of the table differs"), (dict(scheme=kn.KR_RK4), kn.KR_E_UNSUPPORTED, b"RK4"),
                 (dict(T=0, st=None), kn.KR_E_ARG, b"T < 1"))
    for kw, want, word in sim_cases:
        rc = sim(**kw)
        assert rc == want and word in lib.kr_last_error(), (kw, rc, want, lib.kr_last_error())
    torch.cuda.synchronize()
    for o in outs + souts + stail + [g_states]:
        assert bool((o == 7).all())
    with pytest.raises(kn.KrError, match="holds 3 rods, the parameter table 4"):
        hc.step_vjp_table(table, prev[:3], cur[:3], nxt[:3], tens[:3], g_next[:3])
    with pytest.raises(kn.KrError, match="must be a ParamTable"):
        hc.step_vjp_table(None, prev, cur, nxt, tens, g_next)


def test_simulate_tips_batch_backward_against_the_fixture(torch_cuda, ft):
    """7. simulate_tips_batch(...).backward() on the fixture's T = 3 case (the tip cotangent): ctl.grad, the per-rod theta[k].grad
    for E, C, tendon_dirs, base_motion.grad and tip_loads.grad against the same fixture blocks; and rollout_grad(robots=...)
    returns the handle-level results."""
    torch = torch_cuda
    import krod_grad as kg
    import krod_native as kn
    case, T, N = "T3", 3, tc.N_FIX
    hc, table, ks, ctl, bnd, states, _, robots = rollout_batch(torch, ft, case)
    carrier = tc.carrier_for(N)
    val = lambda r, k: np.array(getattr(r, k), dtype=np.float64)
    theta = {k: torch.tensor(np.stack([val(r, k) for r in robots]), dtype=torch.float64, requires_grad=True) for k in ("E", "C", "tendon_dirs")}
    leaf = ctl.clone().requires_grad_(True)
    base = bnd[:, :, :13].clone().requires_grad_(True)
    loads = bnd[:, :, 13:].clone().requires_grad_(True)
    w = _dev(torch, np.stack([ft[k + "gbar"][0][1:, N - 1, 12:15] for k in ks]))  # [B, T, 3]: the tip cotangent of every step
    tips = kg.simulate_tips_batch(carrier, robots, leaf, theta=theta, base_motion=base, tip_loads=loads)
    assert tuple(tips.shape) == (3, T, 3) and torch.equal(tips, states[1:, :, N - 1, 12:15].permute(1, 0, 2))
    (tips * w).sum().backward()
    assert tuple(theta["E"].grad.shape) == (3,) and tuple(theta["tendon_dirs"].grad.shape) == (3, 4, 3)
    for b, k in enumerate(ks):
        got = tc.x_got(leaf.grad[b].cpu().numpy(), torch.cat([base.grad[b], loads.grad[b]], dim=1).cpu().numpy(), np.zeros((N, 28)))
        tc.assert_x_blocks(got, ft[k + "x_fd_h"][0], ft[k + "x_fd_2h"][0], ft[k + "x_floor"][0], T, False, f"{k} autograd", only=("g_ctl", "g_bnd"))
        g_par = np.zeros(pc.KR_PAR)
        g_par[0], g_par[28:31], g_par[31:43] = float(theta["E"].grad[b]), theta["C"].grad[b].numpy(), theta["tendon_dirs"].grad[b].numpy().ravel()
        for name, err, tol, size, zero in pc.block_report(g_par, ft[k + "par_fd_h"][0], ft[k + "par_fd_2h"][0], ft[k + "par_floor"][0]):
            if name in ("E", "C", "tendon_dirs"):
                print(f"{k} autograd {name:12s} err {err:.2e} tol {tol:.2e} size {size:.2e}")
                assert tol <= pc.MAX_REL_TOL * size and err <= tol, (k, name, err, tol)
    g = torch.zeros_like(states)
    g[1:, :, N - 1, 12:15] = w.permute(1, 0, 2)
    direct = hc.simulate_vjp_table(table, ctl, states, g.clone(), bnd_per_step=True, need_par=True)
    res = kg.rollout_grad(carrier, ctl, states, g_tips=w.cpu().numpy(), physical=True, robots=robots, per_step_boundary=True)
    assert np.array_equal(res["ctl"], direct["g_ctl"].cpu().numpy()) and res["boundary"].shape == (3, T, 19)
    assert np.array_equal(res["boundary"], direct["g_bnd"].cpu().numpy())
    by_name = kn.split_par(direct["g_par"].cpu().numpy())
    assert all(np.array_equal(res["physical"][k], by_name[k]) for k in by_name) and res["physical"]["E"].shape == (3,)
    assert torch.equal(leaf.grad, direct["g_ctl"]) and torch.equal(theta["E"].grad.to(DEV), direct["g_par"][:, 0])
    assert torch.equal(base.grad, direct["g_bnd"][:, :, :13]) and torch.equal(loads.grad, direct["g_bnd"][:, :, 13:])
    summed = kg.rollout_grad(carrier, ctl, states, g_tips=w.cpu().numpy(), robots=robots)
    assert summed["boundary"].shape == (3, 19) and "physical" not in summed
