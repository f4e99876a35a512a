"""Per-rod networks (kr_mlp_bank_*, kr_simulate_batch_bank) on the MI355X.

Rod b of one simulate call runs with row b of a parameter table AND network ``net_of_rod[b]`` of a bank - the
reference's model-mismatch experiment loads every model variant's own trained network before it simulates
(physics_multitrain.py:181-199).  The reference side of a comparison is the CPU oracle's tightly converged Newton
solver with the rod's own parameters and network (tests/mlp_bank_cases.py: every step ``ier == 1``; on one parameter
set two of these networks move the tip by 2-5 % relative, so a rod served the wrong network misses by orders of
magnitude), or another call of the library where a result has to be the same bit for bit.
Tolerances are the project's own: fp64 ``rel_l2 < 1e-8`` against oracle trajectories, fp32 tip paths ``< 1e-5``.

Every served call asserts what ran: one persistent launch (``last_sim_path == 2``), one wavefront per rod, no
overlapped kernel, ``status == 0`` on every step of every rod."""
import numpy as np
import pytest

import mlp_bank_cases as cases
from conftest import rel_l2
from gpu_helpers import inject, make_robot, set_mode_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check(label, value, bound):
    print(f"{label}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, f"{label}: {value:.3e} >= {bound:.0e}"


def assert_bank_ran(h):
    got = (h.get_option("last_sim_path"), h.get_option("last_waves_per_rod"), h.get_option("last_overlap"))
    assert got == (2, 1, 0), f"(path, waves per rod, overlap) = {got}, expected (2, 1, 0)"


def as_network(mlp):
    return (mlp.weights, mlp.biases, mlp.acts)


def tdtype(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def run(torch, h, ctl, dt, table, bank=None, net_of_rod=None, ring=False, use_nn=True, scheme=0):
    """One call through Handle.simulate: a bank call, or (bank None) the one-network table call with the handle's MLP."""
    ctl = torch.as_tensor(np.asarray(ctl, dtype=np.float64), device=DEV).to(dt).contiguous()
    B, T = ctl.shape[0], ctl.shape[1]
    st = h.new_state(B, dt, n_slots=3 if ring else T + 1)
    h.init_straight(st[0], table=table)
    G = torch.zeros((B, 6), dtype=dt, device=DEV)
    tip = torch.zeros((B, T, 3), dtype=dt, device=DEV)
    status = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    try:
        if bank is not None:
            h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, bank=bank, net_of_rod=net_of_rod, scheme=scheme)
        else:
            h.simulate(ctl, st, G, ring=ring, tip=tip, status=status, table=table, use_nn=use_nn, scheme=scheme)
    finally:
        torch.cuda.synchronize()
    out = dict(tip=tip.double().cpu().numpy(), status=status.cpu().numpy(), G=G.double().cpu().numpy(),
               states=st.double().cpu().numpy())
    return out


def traj_of(torch, h, states):
    """float64[B, T + 1, 25, N] in the reference's row order from a full state history [T + 1, B, N, slots]."""
    out = []
    for t in range(states.shape[0]):
        y, z = h.unpack(torch.as_tensor(states[t], device=DEV).contiguous())
        out.append(torch.cat([y, z], dim=1).cpu().numpy())
    return np.stack(out, axis=1)


def same(a, b, what):
    for k in ("status", "tip", "G", "states"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs (max |d| = {np.max(np.abs(a[k].astype(np.float64) - b[k]))})"


def compare_with_oracle(torch, h, out, case, dtype):
    refs = cases.oracle_case(case)
    T = case["steps"]
    assert np.all(out["status"] == 0), np.argwhere(out["status"] != 0)[:8]
    traj = traj_of(torch, h, out["states"])
    assert traj.shape == (len(refs), T + 1, 25, case["N"])
    for b, ref in enumerate(refs):  # every rod, none left out
        label = f"rod {b} ({case['mods'][b]}, network {case['nets'][b]})"
        if dtype == "f64":
            check(f"{label} trajectory", rel_l2(traj[b, :T], ref), 1e-8)
        else:
            check(f"{label} fp32 tip path", rel_l2(traj[b, :T, :3, -1], ref[:, :3, -1]), 1e-5)


def case_call(torch, monkeypatch, case, dtype):
    """The bank call of one case of tests/mlp_bank_cases.py; returns (handle, output)."""
    set_mode_env(monkeypatch, "overlap")
    dt = tdtype(torch, dtype)
    N = case["N"]
    carrier = make_robot(None, N)
    h = carrier._native()
    rows = [make_robot(m, N)._params() for m in case["mods"]]
    ctl = np.stack([cases.controls(case["steps"])] * len(rows))
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank_of(case)]) as bank:
        assert bank.K == len(cases.bank_of(case))
        out = run(torch, h, ctl, dt, tab, bank, list(case["nets"]))
    assert_bank_ran(h)
    return carrier, h, out


# ---------------------------------------------------------------------------
# 1. - 3. banks against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_layer_bank_against_the_oracle(torch_cuda, monkeypatch, dtype):
    carrier, h, out = case_call(torch_cuda, monkeypatch, cases.CASE_THREE, dtype)
    compare_with_oracle(torch_cuda, h, out, cases.CASE_THREE, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_layer_bank_against_the_oracle(torch_cuda, monkeypatch, dtype):
    carrier, h, out = case_call(torch_cuda, monkeypatch, cases.CASE_TWO, dtype)
    compare_with_oracle(torch_cuda, h, out, cases.CASE_TWO, dtype)


def test_the_workloads_shape_n100(torch_cuda, monkeypatch):
    carrier, h, out = case_call(torch_cuda, monkeypatch, cases.CASE_N100, "f64")
    compare_with_oracle(torch_cuda, h, out, cases.CASE_N100, "f64")


# ---------------------------------------------------------------------------
# 4. a bank of copies of one network is the one-network table call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bank_of_copies_is_the_one_network_table_call_bit_for_bit(torch_cuda, monkeypatch, dtype):
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = tdtype(torch, dtype)
    mods = cases.CASE_THREE["mods"]
    net = cases.bank_three()[1]
    carrier = make_robot(None, 20)
    h = carrier._native()
    h.set_mlp(*as_network(net))
    rows = [make_robot(m, 20)._params() for m in mods]
    ctl = np.stack([cases.controls(20)] * len(rows))
    with h.param_table(rows) as tab, h.mlp_bank([as_network(net)] * 3) as bank:
        for ring in (False, True):
            plain = run(torch, h, ctl, dt, tab, use_nn=True, ring=ring)
            assert (h.get_option("last_sim_path"), h.get_option("last_overlap")) == (2, 0)
            assert np.all(plain["status"] == 0)
            banked = run(torch, h, ctl, dt, tab, bank, [0, 1, 2, 2, 1, 0], ring=ring)
            assert_bank_ran(h)
            same(plain, banked, f"ring={ring}")


# ---------------------------------------------------------------------------
# 5. permuting (robots, net_of_rod, ctl) together permutes the outputs
# ---------------------------------------------------------------------------
def test_permuting_the_rods_permutes_the_outputs_bitwise(torch_cuda, monkeypatch):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    mods = [None, "damping", "short", "youngs", "noair", "nsw", "dampstiff", "lengthstiff"]
    nets = [0, 1, 2, 3, 3, 2, 1, 0]
    B = len(mods)  # two workgroups of four wavefronts
    carrier = make_robot(None, 20)
    h = carrier._native()
    rows = [make_robot(m, 20)._params() for m in mods]
    ctl = orc.batch_sine_controls(B, 12, carrier.del_t, 77)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    with h.mlp_bank([as_network(m) for m in cases.bank_three()]) as bank:
        with h.param_table(rows) as tab:
            a = run(torch, h, ctl, dt, tab, bank, nets)
        with h.param_table([rows[p] for p in perm]) as tab:
            b = run(torch, h, ctl[perm], dt, tab, bank, [nets[p] for p in perm])
    assert_bank_ran(h)
    assert np.all(a["status"] == 0)
    assert not np.array_equal(a["tip"][0], a["tip"][7])  # (same network, different parameters and controls)
    for k in ("status", "tip", "G"):
        assert np.array_equal(a[k][perm], b[k]), k
    assert np.array_equal(a["states"][:, perm], b["states"])


# ---------------------------------------------------------------------------
# 6. a rod's result does not depend on the batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_rods_result_does_not_depend_on_the_batch(torch_cuda, monkeypatch, dtype):
    torch = torch_cuda
    case = cases.CASE_THREE
    carrier, h, full = case_call(torch, monkeypatch, case, dtype)
    dt = tdtype(torch, dtype)
    for b in (0, 1, 2, 4):  # one rod per network: 0, 1, 2, 3
        k = case["nets"][b]
        with h.param_table([make_robot(case["mods"][b], 20)._params()]) as tab, \
                h.mlp_bank([as_network(cases.bank_three()[k])]) as bank:
            one = run(torch, h, cases.controls(20)[None], dt, tab, bank, [0])
        assert_bank_ran(h)
        for key in ("status", "tip", "G"):
            assert np.array_equal(one[key][0], full[key][b]), (b, key)
        assert np.array_equal(one["states"][:, 0], full["states"][:, b]), b


# ---------------------------------------------------------------------------
# 7. the handle's own MLP survives a bank call
# ---------------------------------------------------------------------------
def test_the_handles_own_mlp_survives_a_bank_call(torch_cuda, monkeypatch):
    import cosserat_oracle as orc
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    case = cases.CASE_THREE
    fifth = orc.make_mlp([28, 64, 64, 25], "elu", seed=15)
    carrier = make_robot(None, 20)
    h = carrier._native()
    h.set_mlp(*as_network(fifth))
    rows = [make_robot(m, 20)._params() for m in case["mods"]]
    ctl = np.stack([cases.controls(20)] * len(rows))
    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank_three()]) as bank:
        before = run(torch, h, ctl, dt, tab, use_nn=True)
        banked = run(torch, h, ctl, dt, tab, bank, list(case["nets"]))
        assert_bank_ran(h)
        after = run(torch, h, ctl, dt, tab, use_nn=True)
    assert np.all(before["status"] == 0) and np.all(banked["status"] == 0)
    same(before, after, "the plain table call after a bank call")
    assert not np.array_equal(before["tip"], banked["tip"])  # (the fifth network is none of the bank's)


# ---------------------------------------------------------------------------
# 8. Python surface
# ---------------------------------------------------------------------------
def test_simulate_batch_per_robot_nn(torch_cuda, monkeypatch):
    import krod_native as kn
    from knode import simulate_batch
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    case = cases.CASE_THREE
    robots = []
    for mod, k in zip(case["mods"], case["nets"]):
        r = make_robot(mod, 20)
        inject(r, cases.bank_three()[k])
        robots.append(r)
    banks = []
    real = kn.Handle.mlp_bank

    def spy(self, networks):
        banks.append(real(self, networks))
        return banks[-1]
    monkeypatch.setattr(kn.Handle, "mlp_bank", spy)
    carrier = make_robot(None, 20)  # (carries no network of its own)
    ctl = np.stack([cases.controls(20)] * 6)
    out = simulate_batch(carrier, ctl, robots=robots, per_robot_nn=True)
    assert_bank_ran(carrier._handle)
    assert len(banks) == 1 and banks[0].K == 4 and banks[0].dims == (28, 64, 64, 25)  # six robots, four uploads
    assert out["n_networks"] == 4 and list(out["net_of_rod"]) == list(case["nets"])
    assert np.all(out["status"] == 0)
    refs = cases.oracle_case(case)
    for b, ref in enumerate(refs):
        check(f"rod {b} trajectory", rel_l2(out["traj"][b, :20], ref), 1e-8)
    # the default leaves every existing call as it was: without per_robot_nn the carrier's (absent) MLP is used
    off = simulate_batch(carrier, ctl, robots=robots)
    assert "n_networks" not in off and len(banks) == 1
    assert not np.array_equal(off["tip"], out["tip"])


# ---------------------------------------------------------------------------
# 9. refusals at run time
# ---------------------------------------------------------------------------
def test_refusals_at_run_time(torch_cuda, monkeypatch):
    import cosserat_oracle as orc
    import krod_native as kn
    torch = torch_cuda
    set_mode_env(monkeypatch, "overlap")
    dt = torch.float64
    carrier = make_robot(None, 20)
    h = carrier._native()
    fifth = orc.make_mlp([28, 64, 64, 25], "elu", seed=15)
    h.set_mlp(*as_network(fifth))  # (a refused bank call must not be served from this one)
    mods = [None, "damping", "short", "youngs"]
    rows = [make_robot(m, 20)._params() for m in mods]
    ctl = np.stack([cases.controls(6)] * 4)

    def refused(code, match, **kw):
        with pytest.raises(kn.KrError, match=match) as e:
            run(torch, h, ctl, dt, kw.pop("table"), kw.pop("bank"), kw.pop("nets"), **kw)
        assert e.value.code == code, (e.value.code, str(e.value))

    with h.param_table(rows) as tab, h.mlp_bank([as_network(m) for m in cases.bank_three()]) as bank:
        refused(kn.KR_E_UNSUPPORTED, "Euler", table=tab, bank=bank, nets=[0, 1, 2, 3], scheme=kn.KR_RK4)
        h.set_option("waves_per_rod", 2)
        refused(kn.KR_E_UNSUPPORTED, "waves_per_rod", table=tab, bank=bank, nets=[0, 1, 2, 3])
        h.set_option("waves_per_rod", 1)
        # an index outside the bank: refused on the host, nothing launched - every output still holds its fill
        for nets, rod in (([0, 1, 4, 3], 2), ([0, -1, 2, 3], 1)):
            ctl_t = torch.as_tensor(ctl, device=DEV).contiguous()
            st = h.new_state(4, dt, n_slots=7)
            h.init_straight(st[0], table=tab)
            G = torch.zeros((4, 6), dtype=dt, device=DEV)
            tip = torch.full((4, 6, 3), -7.0, dtype=dt, device=DEV)
            status = torch.full((4, 6), -1, dtype=torch.int32, device=DEV)
            with pytest.raises(kn.KrError, match=f"rod {rod}") as e:
                h.simulate(ctl_t, st, G, tip=tip, status=status, table=tab, bank=bank, net_of_rod=nets)
            torch.cuda.synchronize()
            assert e.value.code == kn.KR_E_ARG
            assert torch.all(status == -1) and torch.all(tip == -7.0) and torch.all(st[1:] == 0) and torch.all(G == 0)
        # B: a table of another size than the call's, an index array of another length
        with h.param_table(rows[:3]) as tab3:
            with pytest.raises(kn.KrError, match="4 rods"):
                run(torch, h, ctl, dt, tab3, bank, [0, 1, 2])
        with pytest.raises(kn.KrError, match="net_of_rod 3"):
            run(torch, h, ctl, dt, tab, bank, [0, 1, 2])
        # the pieces go together
        with pytest.raises(kn.KrError, match="together"):
            h.simulate(torch.as_tensor(ctl, device=DEV), None, None, bank=bank, net_of_rod=[0, 1, 2, 3])
        # and a served call still works after all of these
        ok = run(torch, h, ctl, dt, tab, bank, [0, 1, 2, 3])
        assert_bank_ran(h)
        assert np.all(ok["status"] == 0)
    # a shape the bank kernels do not serve: refused by the check and by create
    wide = orc.make_mlp([28, 128, 64, 25], "elu", seed=3)
    rc, msg = kn.mlp_bank_check(carrier._params(), 2, [28, 128, 64, 25], wide.acts)
    assert rc == kn.KR_E_UNSUPPORTED and "first hidden layer" in msg
    with pytest.raises(kn.KrError, match="first hidden layer") as e:
        h.mlp_bank([as_network(wide)] * 2)
    assert e.value.code == kn.KR_E_UNSUPPORTED
    with pytest.raises(kn.KrError, match="K must be") as e:
        h.mlp_bank([])
    assert e.value.code == kn.KR_E_ARG
    with pytest.raises(kn.KrError, match="share one shape"):
        h.mlp_bank([as_network(cases.bank_three()[0]), as_network(cases.bank_two()[0])])
