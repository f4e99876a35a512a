"""Per-step boundary data (kr_simulate_batch_boundary), host side (no GPU): the C ABI surface, the fixture
tests/golden/base_motion.npz - the unmodified reference run with ``robot.p0 / h0 / q0 / w0`` assigned while
``knode.simulate`` draws control t - against the oracle's own time loop, the argument validation of
``knode.simulate_batch(..., base_motion=...)``, which raises before anything touches a device, how the boundary array
is composed, and the planner: a boundary query plans as the loads query does.

Bounds of the oracle comparison are those tests/test_tip_loads_cpu.py uses: tips < 1e-9, trajectory and last state < 1e-7
relative L2 (the reference stops fsolve at xtol 1.5e-8).  Measured with these inputs: tips <= 3.5e-11, trajectory
<= 5.4e-10, at most 5 Newton iterations per solve; a history applied one step late moves the tips by >= 1.7e-2 (``still``
excepted - it is constant), every history moves them by >= 2.3e-2 against the unmoved run."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from base_motion_cases import CASES, SHAPES, UNMOVED, base_history, oracle_loop
from conftest import ROOT, load_golden, rel_l2

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


def test_boundary_symbol_declared_exported_and_bound(kn):
    name = "kr_simulate_batch_boundary"
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert proto, f"{name} is not declared in include/knode_rod.h"
    assert re.search(r"#define\s+KR_BND\s+19\b", text) and kn.KR_BND == 19
    assert hasattr(ctypes.CDLL(kn.LIB_PATH), name), f"{name} is not exported by the library"
    assert name in kn.EXPORTED_SYMBOLS
    fn = getattr(kn.load(), name)
    assert fn.restype is ctypes.c_int
    assert len(fn.argtypes) == len(proto.group(1).split(",")) == 17
    # bnd follows ctl, as loads does in the loads call - whose binding this one's equals
    args = [a.split()[-1].lstrip("*") for a in proto.group(1).split(",")]
    assert args[4:7] == ["ctl", "bnd", "states"], args
    assert list(fn.argtypes) == list(kn.load().kr_simulate_batch_loads.argtypes)


def test_fixture_is_what_the_issue_describes():
    g = load_golden("base_motion")
    assert tuple(g["cases"]) == CASES == ("still", "slide", "tilt", "jump", "alt")
    n = len(CASES)
    for N, T in SHAPES:
        k = f"_n{N}"
        assert g["ctl" + k].shape == (T, 4) and g["base" + k].shape == (n, T, 13)
        assert g["tips" + k].shape == (n, T, 3) and g["last" + k].shape == (n, 25, N)
        assert g["tips_unmoved" + k].shape == (T, 3) and g["last_unmoved" + k].shape == (25, N)
        for c, case in enumerate(CASES):
            assert np.array_equal(g["base" + k][c], base_history(case, T)), case
        assert np.all(g["ier" + k] == 1) and np.all(g["ier_unmoved" + k] == 1)  # fsolve converged on every step
        # not vacuous: every history moves the tip path
        for c, case in enumerate(CASES):
            d = rel_l2(g["tips" + k][c], g["tips_unmoved" + k])
            print(f"N = {N}: {case} against the unmoved run, tips rel L2 {d:.2e}")
            assert d > 1e-2, case
        # record 0 of a state holds the base of the step that produced it: exact in the reference (state t <- step t - 1)
        for c in range(n):
            if N == 10:
                assert np.array_equal(g["traj" + k][c][1:, :7, 0], g["base" + k][c][:T - 1, :7])
                assert np.array_equal(g["traj" + k][c][1:, 13:19, 0], g["base" + k][c][:T - 1, 7:])
            assert np.array_equal(g["last" + k][c][:7, 0], g["base" + k][c][T - 2, :7])
    # the histories are what the issue's table says
    s = base_history("still", 3)
    assert np.array_equal(s[1], [0.01, -0.02, 0.03, 0.98, 0.05, -0.1, 0.02, 0.01, 0, -0.02, 0.05, -0.03, 0.02])
    j = base_history("jump", 12)
    assert np.array_equal(j[5], UNMOVED) and np.array_equal(j[6, :7], [0.01, 0, 0, 1.05, 0, 0.08, 0])
    a = base_history("alt", 4)
    assert np.array_equal(a[:, 0], [0.005, -0.005, 0.005, -0.005]) and np.array_equal(a[:, 4], [0.02, -0.02, 0.02, -0.02])
    assert np.array_equal(a[:, 12], [0.1, -0.1, 0.1, -0.1]) and np.array_equal(a[:, 1], [-0.002, 0.002, -0.002, 0.002])
    sl = base_history("slide", 12)
    om = 2 * np.pi / (8 * 0.05)
    assert np.allclose(sl[:, 0], 0.02 * np.sin(om * np.arange(12) * 0.05), rtol=0, atol=1e-18) and sl[0, 7] == 0.02 * om
    tl = base_history("tilt", 13)
    assert np.allclose(tl[:, 3] ** 2 + tl[:, 5] ** 2, 1.0, rtol=0, atol=1e-15) and tl[0, 11] == 0.2 * 2 * np.pi / (10 * 0.05)
    assert g["traj_n10"].shape == (n, 12, 25, 10) and "traj_n23" not in g.files


@pytest.mark.parametrize("N,T", SHAPES)
def test_oracle_loop_against_the_reference(N, T):
    import cosserat_oracle as orc
    g = load_golden("base_motion")
    k = f"_n{N}"
    P = orc.params_for(None, N)
    assert np.array_equal(np.concatenate([P.p0, P.h0, P.q0, P.w0]), UNMOVED)
    for c, case in enumerate(CASES):
        states, ok, its = oracle_loop(P, g["ctl" + k], g["base" + k][c])
        assert ok.all() and its.max() <= 5, (case, its)
        e_tip = rel_l2(states[:T, :3, -1], g["tips" + k][c])
        e_last = rel_l2(states[T - 1], g["last" + k][c])
        print(f"N = {N} {case}: tips {e_tip:.2e} (bound 1e-9), state T-1 {e_last:.2e} (bound 1e-7), iterations <= {its.max()}")
        assert e_tip < 1e-9 and e_last < 1e-7
        if N == 10:
            e_traj = rel_l2(states[:T], g["traj" + k][c])
            print(f"N = {N} {case}: trajectory {e_traj:.2e} (bound 1e-7)")
            assert e_traj < 1e-7
        # a base one step late is another trajectory: the comparison above tells time levels apart
        if case != "still":
            late = np.vstack([g["base" + k][c][:1], g["base" + k][c][:-1]])
            moved, _, _ = oracle_loop(P, g["ctl" + k], late)
            d = rel_l2(moved[:T, :3, -1], g["tips" + k][c])
            print(f"N = {N} {case}: one step late moves the tips by {d:.2e}")
            assert d > 1e-2, case
    states, ok, _ = oracle_loop(P, g["ctl" + k], np.tile(UNMOVED, (T, 1)))
    assert ok.all() and rel_l2(states[:T, :3, -1], g["tips_unmoved" + k]) < 1e-9


def test_simulate_batch_validates_base_motion_on_the_host(kn, monkeypatch):
    import knode
    robot = preset_robot(None)
    monkeypatch.setattr(type(robot), "_native", lambda self: pytest.fail("a device call before validation"))
    B, T = 3, 5
    ctl = np.full((B, T, 4), 5.0)
    good = np.tile(UNMOVED, (B, T, 1))

    def refused(word, **kw):
        with pytest.raises(kn.KrError) as e:
            knode.simulate_batch(robot, ctl, **kw)
        assert word in str(e.value), str(e.value)

    refused("[3, 5, 13]", base_motion=np.zeros((B, T, 12)))          # a wrong shape
    refused("[3, 5, 13]", base_motion=np.zeros((B, T + 1, 13)))      # a row count other than ctl's
    refused("[5, 13]", base_motion=np.zeros((T + 1, 13)))
    refused("base_motion must be", base_motion=np.zeros(13))
    refused("base_motion must be a numeric array", base_motion=[["p0"] * 13] * T)
    refused("holds 2 rods", base_motion=good[:B - 1])                # another number of rods
    bad = good.copy()
    bad[1, 3, 2] = np.nan
    refused("base_motion is not finite at rod 1, step 3", base_motion=bad)
    bad = good.copy()
    bad[2, 4, 9] = np.inf
    refused("base_motion is not finite at rod 2, step 4", base_motion=bad)
    zero = good.copy()
    zero[2, 1, 3:7] = 0.0
    refused("zero quaternion h0 at rod 2, step 1", base_motion=zero)
    refused("zero quaternion h0 at rod 0, step 1", base_motion=zero[2])  # ([T, 13]: the first rod that gets it)
    # a non-unit h0 is ordinary input (the reference does not normalise it)
    odd = good.copy()
    odd[:, :, 3:7] = [1.05, 0, 0.08, 0]
    assert np.array_equal(knode._base_motion(odd, B, T), odd)
    # check_finite=False hands both on unchanged: to the library they are ordinary input (knode_rod.h, "failed steps")
    bad[1, 3, 2] = np.nan
    passed = knode._base_motion(bad, B, T, check_finite=False)
    assert passed.shape == (B, T, 13) and np.isnan(passed[1, 3, 2]) and np.isinf(passed[2, 4, 9])
    assert np.array_equal(knode._base_motion(zero, B, T, check_finite=False), zero)
    shared = knode._base_motion(good[0], B, T)
    assert shared.shape == (B, T, 13) and shared.flags["C_CONTIGUOUS"] and np.array_equal(shared, good)
    refused("not served", base_motion=good, robots=[robot] * B, per_robot_nn=True)
    refused("not served", base_motion=good, per_robot_nn=True)
    with pytest.raises(kn.KrError, match=r"ctl must be \[B, T, 4\]"):
        knode.simulate_batch(robot, ctl[0], base_motion=good[0])
    # the wrench history next to it is validated as it is alone
    refused("[3, 5, 6]", base_motion=good, tip_loads=np.zeros((B, T, 5)))
    # ... and the binding refuses bnd next to a bank, or next to loads, before it calls the library
    H = kn.Handle
    with pytest.raises(kn.KrError, match="bank"):
        H.simulate(object.__new__(H), ctl, None, None, table=object(), bank=object(), net_of_rod=[0] * B, bnd=good)
    with pytest.raises(kn.KrError, match="loads"):
        H.simulate(object.__new__(H), ctl, None, None, table=object(), loads=good, bnd=good)
    with pytest.raises(kn.KrError, match="table"):
        H.simulate(object.__new__(H), ctl, None, None, bnd=good)


def test_wrench_columns_come_from_the_rows_without_tip_loads(kn):
    import knode
    B, T = 3, 4
    robots = []
    for b, mod in enumerate([None, "damping", "short"]):
        r = preset_robot(mod)
        r.F_tip, r.M_tip = np.array([0.1 * (b + 1), -0.2, 0.3 * b]), np.array([1e-3 * b, 2e-3, -1e-3 * (b + 1)])
        robots.append(r)
    rows = [r._params() for r in robots]
    base = np.stack([base_history(c, T) for c in ("slide", "tilt", "alt")])
    bnd = knode._boundary(base, None, rows)
    assert bnd.shape == (B, T, kn.KR_BND) and bnd.dtype == np.float64
    assert np.array_equal(bnd[:, :, :13], base)
    for b, r in enumerate(robots):
        assert np.array_equal(bnd[b, :, 13:16], np.tile(r.F_tip, (T, 1))) and np.array_equal(bnd[b, :, 16:19], np.tile(r.M_tip, (T, 1)))
    loads = np.arange(B * T * 6, dtype=np.float64).reshape(B, T, 6)
    both = knode._boundary(base, loads, rows)
    assert np.array_equal(both[:, :, :13], base) and np.array_equal(both[:, :, 13:], loads)


def test_boundary_query_plans_as_the_loads_query(tmp_path):
    """tests/base_motion_plan_probe.hip: the planner on a matrix of table queries, as a loads and as a boundary query."""
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found (the library itself is built with it)"
    out = tmp_path / "plan_probe"
    cmd = [hipcc, "-O0", "-std=c++17", "--cuda-host-only", "-rdynamic", "-w",
           "-I", os.path.join(ROOT, "knode-cosserat_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "base_motion_plan_probe.hip"), "-o", str(out), "-ldl", "-Wl,--unresolved-symbols=ignore-all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split(" | ") for l in r.stdout.splitlines()]
    assert len(lines) == 2 * 7 * 2 * 2 * 3 * 7 * 2 and len(lines) % 2 == 0
    served = refusals = 0
    seen = set()
    for (la, fa, pa, wa), (lb, fb, pb, wb) in zip(lines[0::2], lines[1::2]):
        assert la == lb and (fa, fb) == ("loads", "bnd")
        assert pa == pb, (la, pa, pb)  # rc, path, family, W, occ, nn, overlap, LDS bytes of both launches
        rc = int(pa.split()[0])
        if rc == 0:
            served += 1
            assert wa == wb == "" and pa.split()[1] == "2"
            seen.add((la.split(",")[0], pa.split()[2], pa.split()[5]))
        else:
            refusals += 1
            if wa.startswith("kr_simulate_batch_loads: "):  # a rule of the table family: worded for each call
                assert wb.startswith("kr_simulate_batch_boundary: "), wb
                rule = lambda w: w.split(": ", 1)[1].rsplit(" (not served", 1)[0].replace("boundary", "loads")  # ("a loads form", "loads calls run ...")
                assert rule(wa) == rule(wb), (wa, wb)
                assert "per-step boundary data" in wb and "frozen base" in wb
            else:
                assert wa == wb  # (no MLP was set: KR_E_STATE, the same words)
    n8 = [w for (l, f, _, w) in lines if l.startswith("f64,8,6,E,n0,none") and f == "bnd"]
    assert n8 and all("kr_simulate_batch_boundary: N = 8" in w and "9 <= N <= 128" in w for w in n8), n8
    print(f"{served} served and {refusals} refused queries plan alike")
    assert served >= 80 and refusals >= 500
    # both kernel families, with the MLP off and on, in both precisions
    assert len({s[1] for s in seen}) == 2 and {(d, n) for d, _, n in seen} == {("f64", "0"), ("f64", "1"), ("f32", "0"), ("f32", "1")}
