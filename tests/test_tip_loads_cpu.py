"""Per-step tip loads (kr_simulate_batch_loads), host side (no GPU): the C ABI surface, the fixture
tests/golden/tip_loads.npz - the unmodified reference run with ``robot.F_tip`` / ``robot.M_tip`` assigned while
``knode.simulate`` draws control t - against the oracle's own time loop, and the argument validation of
``knode.simulate_batch(..., tip_loads=...)``, which raises before anything touches a device.

Bounds of the oracle comparison are those tests/test_oracle_golden.py uses for the Newton oracle against reference-held
trajectories: tips < 1e-9, trajectory and last state < 1e-7 relative L2 (the reference stops fsolve at xtol 1.5e-8)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_l2
from tip_loads_cases import CASES, SHAPES, load_history, oracle_loop

HEADER = os.path.join(ROOT, "include", "knode_rod.h")


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    return kn


def preset_robot(mod, N=10):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r, mod)
    r.N = N
    r.compute_intermediate_terms()
    return r


def test_loads_symbol_declared_exported_and_bound(kn):
    name = "kr_simulate_batch_loads"
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert proto, f"{name} is not declared in include/knode_rod.h"
    assert hasattr(ctypes.CDLL(kn.LIB_PATH), name), f"{name} is not exported by the library"
    assert name in kn.EXPORTED_SYMBOLS
    fn = getattr(kn.load(), name)
    assert fn.restype is ctypes.c_int
    assert len(fn.argtypes) == len(proto.group(1).split(",")) == 17
    # loads follows ctl, as in the table call with one argument more
    args = [a.split()[-1].lstrip("*") for a in proto.group(1).split(",")]
    assert args[4:7] == ["ctl", "loads", "states"], args


def test_fixture_is_what_the_issue_describes():
    g = load_golden("tip_loads")
    assert tuple(g["cases"]) == CASES
    for N, T in SHAPES:
        k = f"_n{N}"
        assert g["ctl" + k].shape == (T, 4) and g["loads" + k].shape == (4, T, 6)
        assert g["tips" + k].shape == (4, T, 3) and g["last" + k].shape == (4, 25, N)
        for c, case in enumerate(CASES):
            assert np.array_equal(g["loads" + k][c], load_history(case, T)), case
        assert np.all(g["ier" + k] == 1) and np.all(g["ier_zero" + k] == 1)  # fsolve converged on every step
        # not vacuous: the alternating wrench moves the tip path
        d = rel_l2(g["tips" + k][CASES.index("alt")], g["tips_zero" + k])
        print(f"N = {N}: alt against no load, tips rel L2 {d:.2e}")
        assert d > 1e-3
    assert g["traj_n10"].shape == (4, 12, 25, 10) and "traj_n23" not in g.files


@pytest.mark.parametrize("N,T", SHAPES)
def test_oracle_loop_against_the_reference(N, T):
    import cosserat_oracle as orc
    g = load_golden("tip_loads")
    k = f"_n{N}"
    P = orc.params_for(None, N)
    for c, case in enumerate(CASES):
        states, ok, its = oracle_loop(P, g["ctl" + k], g["loads" + k][c])
        assert ok.all() and its.max() <= 5, (case, its)
        e_tip = rel_l2(states[:T, :3, -1], g["tips" + k][c])
        e_last = rel_l2(states[T - 1], g["last" + k][c])
        print(f"N = {N} {case}: tips {e_tip:.2e} (bound 1e-9), state T-1 {e_last:.2e} (bound 1e-7), iterations <= {its.max()}")
        assert e_tip < 1e-9 and e_last < 1e-7
        if N == 10:
            e_traj = rel_l2(states[:T], g["traj" + k][c])
            print(f"N = {N} {case}: trajectory {e_traj:.2e} (bound 1e-7)")
            assert e_traj < 1e-7
    # a wrench one step late is another trajectory: the comparison above tells time levels apart
    late = np.vstack([g["loads" + k][2][:1], g["loads" + k][2][:-1]])
    states, _, _ = oracle_loop(P, g["ctl" + k], late)
    assert rel_l2(states[:T, :3, -1], g["tips" + k][2]) > 1e-3


def test_simulate_batch_validates_tip_loads_on_the_host(kn, monkeypatch):
    import knode
    robot = preset_robot(None)
    monkeypatch.setattr(type(robot), "_native", lambda self: pytest.fail("a device call before validation"))
    B, T = 3, 5
    ctl = np.full((B, T, 4), 5.0)
    good = np.zeros((B, T, 6))

    def refused(word, **kw):
        with pytest.raises(kn.KrError) as e:
            knode.simulate_batch(robot, ctl, **kw)
        assert word in str(e.value), str(e.value)

    refused("[3, 5, 6]", tip_loads=np.zeros((B, T, 5)))          # a wrong shape
    refused("[3, 5, 6]", tip_loads=np.zeros((B, T + 1, 6)))
    refused("[5, 6]", tip_loads=np.zeros((T + 1, 6)))
    refused("tip_loads must be", tip_loads=np.zeros(6))
    refused("holds 2 rods", tip_loads=np.zeros((B - 1, T, 6)))   # a row count other than B
    bad = good.copy()
    bad[1, 3, 2] = np.nan
    refused("not finite at rod 1, step 3", tip_loads=bad)
    # check_finite=False hands it on unchanged: to the library a wrench that is not finite is ordinary input, answered with
    # status 2 for that rod (knode_rod.h, "failed steps"; tests/test_gpu_sick_rod.py)
    passed = knode._tip_loads(bad, B, T, check_finite=False)
    assert passed.shape == (B, T, 6) and np.isnan(passed[1, 3, 2]) and np.isnan(passed).sum() == 1
    refused("not served", tip_loads=good, robots=[robot] * B, per_robot_nn=True)
    refused("not served", tip_loads=good, per_robot_nn=True)
    # ... and the binding refuses loads next to a bank before it calls the library
    with pytest.raises(kn.KrError, match="bank"):
        kn.Handle.simulate(object.__new__(kn.Handle), ctl, None, None, table=object(), bank=object(), net_of_rod=[0] * B, loads=good)
