"""The inputs of tests/test_gpu_sick_rod.py, checked on the CPU oracle (no GPU): what the device tests call "clean" converges
at every step, what they call "sick" makes the oracle's own Newton solve (``newton_shoot``, through the time loop of
tests/tip_loads_cases.py) give up at step t0 inside its own cap with ``ok = False`` - and leaves every earlier step alone -
and the sick twin differs from the clean set in the one entry tests/sick_rod_cases.py names.

Physics-only shapes are solved for every rod (N = 400 by the C restatement of the oracle, which the NumPy loop would take
minutes for); with the MLP on (2 s of NumPy per rod) the rods solved are rod 0 and the sick rods."""
import warnings

import numpy as np
import pytest

import sick_rod_cases as sc
from conftest import load_golden
from tip_loads_cases import oracle_loop

ORACLE_CAP = 50  # newton_shoot's own maxit


def own_wrench(P, T):
    return np.tile(np.concatenate([P.F_tip, P.M_tip]), (T, 1))


@pytest.fixture(scope="module")
def clean_runs():
    """{(family, variant): [states[T + 1, 25, N] of every rod]}, every step converged; computed once."""
    import cosserat_oracle as orc
    runs = {}
    for family in ("k2a", "one_wave", "waves"):
        N, B, T, _ = sc.SHAPES[family]
        c = sc.clean_set(family)
        variants = {"plain": lambda b: (orc.params_for(None, N), own_wrench(orc.params_for(None, N), T))}
        if family == "one_wave":
            variants["table"] = lambda b: (orc.params_for(sc.MODS5[b], N), sc.row_loads(c)[b])
            variants["loads"] = lambda b: (orc.params_for(sc.MODS5[b], N), c["loads"][b])
        for name, pick in variants.items():
            out = []
            for b in range(B):
                P, L = pick(b)
                states, ok, its = oracle_loop(P, c["ctl"][b], L)
                assert ok.all() and its.max() < ORACLE_CAP, (family, name, b, ok, its)
                out.append(states)
            runs[family, name] = out
    return runs


def test_clean_inputs_converge(clean_runs):
    for (family, name), states in clean_runs.items():
        N, B, T, _ = sc.SHAPES[family]
        assert len(states) == B and all(s.shape == (T + 1, 25, N) and np.isfinite(s).all() for s in states), (family, name)
    # the table rows and the load histories are not five copies of one rod
    tips = [s[-1, :3, -1] for s in clean_runs["one_wave", "table"]]
    assert np.linalg.norm(tips[1] - tips[0]) > 1e-3 * np.linalg.norm(tips[0])


def test_clean_long_rod_converges():
    import cosserat_oracle as orc
    import cosserat_oracle_c as oc
    N, B, T, _ = sc.SHAPES["long"]
    c = sc.clean_set("long")
    for b in range(B):
        tip, _, bad = oc.simulate(orc.params_for(None, N), c["ctl"][b])
        assert bad == 0 and tip.shape == (T, 3) and np.isfinite(tip).all(), (b, bad)


def test_clean_inputs_converge_with_the_mlp_on():
    import cosserat_oracle as orc
    import mlp_bank_cases as mb
    N, B, T, sick = sc.SHAPES["one_wave"]
    c = sc.clean_set("one_wave")
    D = orc.params_for(None, N).derived()
    golden = orc.mlp_from_arrays(load_golden("bc"), "mlp_elu6464")
    nets = mb.bank_three()[:2]
    for b in (0,) + tuple(sick):
        ctl = np.vstack([c["ctl"][b], c["ctl"][b][-1:]])  # (orc.simulate drops its last solve)
        for mlp in (golden, nets[sc.BANK_NETS[b]]):
            traj, info = orc.simulate(D, ctl, mlp=mlp, solver="newton", return_info=True)
            assert np.all(info["ier"][:T] == 1) and np.isfinite(traj).all(), (b, info["ier"])


@pytest.mark.parametrize("family,kind", [(f, k) for f in ("k2a", "one_wave", "waves") for k in ("nan_ctl", "overflow_ctl")]
                         + [("one_wave", "nan_load")])  # (the loads call is a one-wavefront call)
def test_the_oracle_gives_up_at_the_sick_step(clean_runs, family, kind):
    import cosserat_oracle as orc
    N, B, T, sick = sc.SHAPES[family]
    c = sc.clean_set(family)
    t0 = sc.T0
    for s in sick:
        tw = sc.sick_twin(c, kind, s)
        if kind == "nan_load":
            P, L, ref = orc.params_for(sc.MODS5[s], N), tw["loads"][s], clean_runs[family, "loads"][s]
        else:
            P = orc.params_for(None, N)
            L, ref = own_wrench(P, T), clean_runs[family, "plain"][s]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (NumPy's invalid-value warnings of the sick solve)
            states, ok, its = oracle_loop(P, tw["ctl"][s][:t0 + 1], L[:t0 + 1])
        assert ok[:t0].all() and not ok[t0], (family, kind, s, ok)
        assert 1 <= its[t0] <= ORACLE_CAP, its
        # steps before t0 are untouched: states 0 .. t0 are those of the clean run, bit for bit
        assert np.array_equal(states[:t0 + 1], ref[:t0 + 1]), (family, kind, s)


@pytest.mark.parametrize("family", list(sc.SHAPES))
def test_the_twin_differs_in_one_entry(family):
    N, B, T, sick = sc.SHAPES[family]
    c = sc.clean_set(family)
    assert c["ctl"].shape == (B, T, 4) and c["loads"].shape == (B, T, 6) and c["wrench"].shape == (B, 6)
    assert all(np.isfinite(v).all() for v in c.values())
    assert sc.differing_entries(c, sc.clean_set(family)) == []
    for s in sick:
        for t0 in (0, sc.T0, T - 1):
            want = {"nan_ctl": ("ctl", (s, t0, 1)), "overflow_ctl": ("ctl", (s, t0, 1)), "nan_row": ("wrench", (s, 0)),
                    "nan_load": ("loads", (s, t0, 0))}
            for kind in sc.KINDS:
                tw = sc.sick_twin(c, kind, s, t0)
                assert sc.differing_entries(c, tw) == [want[kind]], (kind, s, t0)
                name, idx = want[kind]
                v = tw[name][idx]
                assert (v == 1e200) if kind == "overflow_ctl" else np.isnan(v)
                assert sc.first_sick_step(kind, t0) == (0 if kind == "nan_row" else t0)
                assert sc.sick_entry(kind, s, t0)[:2] == want[kind]
    with pytest.raises(ValueError):
        sc.sick_twin(c, "nonsense", 0)
