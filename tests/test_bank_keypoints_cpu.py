"""Bank calls with per-step boundary data and key-point records (kr_simulate_batch_bank_keypoints, kr_mlp_bank_repack,
knode.simulate_bank, krod_eval.evaluate_bank, KnodeBankTrainer.evaluate), host side (no GPU): the C ABI surface, the plan
of the new kind next to the bank query's, the validation of the Python entry points - which raise before anything touches
a device or the library - and the oracle's time loop of tests/bank_keypoints_cases.py against the reference's own run
(tests/golden/bank_motion.npz)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bank_keypoints_cases as cases
from conftest import ROOT, load_golden, rel_l2
from gpu_helpers import inject

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


def header_proto(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert proto, f"{name} is not declared in include/knode_rod.h"
    return [a.split()[-1].lstrip("*") for a in proto.group(1).split(",")]


def test_symbols_declared_exported_and_bound(kn):
    lib = kn.load()
    vp, i64, i32p, vpp = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_void_p)
    want = {
        "kr_simulate_batch_bank_keypoints": (
            ["h", "t", "bank", "net_of_rod_host", "T", "scheme", "ctl", "bnd", "K", "idx_host", "kp", "states", "ring", "G", "tip",
             "tol", "maxit", "status", "state_prev_init", "dtype", "stream"],
            [vp, vp, vp, i32p, i64, ctypes.c_int, vp, vp, ctypes.c_int, i32p, vp, vp, ctypes.c_int, vp, vp, ctypes.c_double,
             ctypes.c_int, vp, vp, ctypes.c_int, vp]),
        "kr_mlp_bank_repack": (["h", "bank", "W", "b", "src_on_device", "stream"], [vp, vp, vpp, vpp, ctypes.c_int, vp]),
    }
    for name, (params, argtypes) in want.items():
        assert header_proto(name) == params, (name, header_proto(name))
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    # the documents speak of the calls as served
    text = open(HEADER).read()
    assert "changed only by kr_mlp_bank_repack" in text and "physics_multitrain.py:180-233" in text and "physics_train.py:136-167" in text
    assert "kr_simulate_batch_bank_keypoints" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # kr_keypoints_check itself keeps refusing K = 0
    assert lib.kr_keypoints_check(23, 0, (ctypes.c_int32 * 1)(0)) == kn.KR_E_ARG


def test_bank_keypoints_query_plans_as_the_bank_query(tmp_path):
    """tests/bank_keypoints_plan_probe.hip: the planner on a matrix of bank queries, as a bank and as a bank key-point query."""
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found (the library itself is built with it)"
    out = tmp_path / "plan_probe"
    cmd = [hipcc, "-O0", "-std=c++17", "--cuda-host-only", "-rdynamic", "-w",
           "-I", os.path.join(ROOT, "knode-cosserat_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "bank_keypoints_plan_probe.hip"), "-o", str(out), "-ldl", "-Wl,--unresolved-symbols=ignore-all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split(" | ") for l in r.stdout.splitlines()]
    assert len(lines) == 2 * 8 * 2 * 2 * 3 * 8 * 2
    served = refusals = 0
    seen, rules = set(), set()
    for (la, fa, pa, wa), (lb, fb, pb, wb) in zip(lines[0::2], lines[1::2]):
        assert la == lb and (fa, fb) == ("bank", "bankkp")
        assert pa == pb, (la, pa, pb)  # rc, path, family, W, occ, nn, overlap, LDS bytes
        rc = int(pa.split()[0])
        if rc == 0:
            served += 1
            assert wa == wb == "" and pa.split()[1] == "2" and pa.split()[5] == "1" and pa.split()[6] == "0"  # persistent, MLP on, no overlap
            seen.add((la.split(",")[0], la.split(",")[4]))
        else:
            refusals += 1
            assert wa.startswith("kr_simulate_batch_bank: ") and wb.startswith("kr_simulate_batch_bank_keypoints: "), (wa, wb)
            rule = lambda w: w.split(": ", 1)[1].rsplit(" (not served", 1)[0].replace("bank key-point", "bank")
            assert rule(wa) == rule(wb), (wa, wb)
            assert "a network bank and per-step boundary data" in wb and "frozen boundary" in wb
            rules.add(re.sub(r"\d+", "#", rule(wb)))
    print(f"{served} served and {refusals} refused queries plan alike; {len(rules)} rules")
    assert served >= 80 and refusals >= 1000
    # every served shape in both precisions, three- and two-layer; every refusal of the bank query was met
    assert seen == {(d, n) for d in ("f64", "f32") for n in ("n0", "n1")}
    for word in ("Euler", "# <= N <= #", "persistent = #", "ms_batch_limit", "waves_per_rod = #", "does not evaluate", "does not fit the LDS"):
        assert any(word in r for r in rules), (word, rules)


def test_simulate_bank_validates_on_the_host(kn, monkeypatch):
    import knode
    import krod_eval
    N, B, T = 10, 3, 5
    robot = preset_robot(None, N)
    monkeypatch.setattr(type(robot), "_native", lambda self: pytest.fail("a device call before validation"))
    monkeypatch.setattr(kn.Handle, "__init__", lambda *a, **k: pytest.fail("a handle before validation"))
    bank = cases.bank(3)
    robots = [preset_robot(m, N) for m in (None, "damping", "short")]
    for r, k in zip(robots, (0, 1, 0)):
        inject(r, bank[k])
    ctl = np.full((B, T, 4), 5.0)

    def refused(word, **kw):
        args = dict(robots=robots)
        args.update(kw)
        with pytest.raises(kn.KrError) as e:
            knode.simulate_bank(robot, args.pop("robots"), args.pop("ctl", ctl), **args)
        assert word in str(e.value), str(e.value)
        assert "simulate_batch" not in str(e.value), str(e.value)

    # what needs no rule of the library is refused before the library is so much as loaded
    with monkeypatch.context() as m:
        m.setattr(kn, "load", lambda: pytest.fail("a library call before validation"))
        refused("simulate_bank needs robots", robots=None)
        refused("robots holds 2 rods, ctl 3", robots=robots[:2])
        refused("ctl must be [B, T, 4]", ctl=ctl[0])
        refused("key point -11 outside", key_points=[-11])
        refused("[3, 5, 13]", base_motion=np.zeros((B, T, 12)))
        refused("score point 9 is not one of the key points [3, 5]", tip_only=True, key_points=[3, 5],
                score={"reference": np.zeros((T + 1, 7, N))})
    refused("simulate_bank needs robots", robots=None)
    refused("robots holds 2 rods, ctl 3", robots=robots[:2])
    refused("ctl must be [B, T, 4]", ctl=ctl[0])
    refused("key point 10 outside the rod's 10 grid points", key_points=[3, 10])
    refused("0 key points", key_points=[])
    refused("[3, 5, 13]", base_motion=np.zeros((B, T, 12)))
    refused("[3, 5, 6]", tip_loads=np.zeros((B, T, 5)))
    bad = np.zeros((B, T, 6))
    bad[1, 3, 2] = np.nan
    refused("not finite at rod 1, step 3", tip_loads=bad)
    ref = np.zeros((T + 1, 7, N))
    refused("score needs the state history", tip_only=True, score={"reference": ref})
    refused("score point 9 is not one of the key points [3, 5]", tip_only=True, key_points=[3, 5], score={"reference": ref})
    refused("score reference has 4 grid points", tip_only=True, key_points=[3, 9], score={"reference": np.zeros((T, 7, 4))})
    # the networks: one shape, a zero network for a robot without one, but not for all of them
    other = preset_robot("short", N)
    inject(other, cases.bank(2)[1])
    refused("rod 2", robots=robots[:2] + [other])
    refused("no robot carries a network", robots=[preset_robot(None, N) for _ in range(B)])
    odd = preset_robot(None, 12)
    inject(odd, bank[0])
    refused("field N = 12", robots=robots[:2] + [odd])
    # evaluate_bank: the same, and the key points are required
    for kw, word in ((dict(key_points=None), "key_points is required"), (dict(key_points=[3, 5]), "score point 9 is not one of the key points"),
                     (dict(key_points=[3, 9], point=5), "score point 5"), (dict(key_points=[10]), "key point 10 outside")):
        with pytest.raises(kn.KrError) as e:
            krod_eval.evaluate_bank(robot, robots, ctl, ref, kw.pop("key_points"), **kw)
        assert word in str(e.value), str(e.value)
    # what the validation hands to the device half: a zero network for the baseline rod, the rows' own boundary
    plain = preset_robot("youngs", N)
    plain.F_tip = np.array([0.1, -0.2, 0.3])
    rows, networks, net_of_rod, bnd, kp_idx, score_ref, score_point = knode._bank_call_inputs(
        robot, robots[:2] + [plain], ctl, True, {"reference": ref, "point": -1}, None, None, [9, 3, -1], True)
    assert net_of_rod == [0, 1, 2] and len(networks) == 3 and kp_idx.tolist() == [3, 9] and score_point == 9
    assert all(not np.any(w) for w in networks[2][0] + networks[2][1]) and list(networks[2][2]) == list(networks[0][2])
    assert [w.shape for w in networks[2][0]] == [w.shape for w in networks[0][0]]
    assert bnd.shape == (B, T, kn.KR_BND) and np.array_equal(bnd[2, :, 13:16], np.tile(plain.F_tip, (T, 1))) and np.all(bnd[:, :, 3] == 1.0)
    # simulate_batch keeps refusing the combination, and points here
    with pytest.raises(kn.KrError, match="not served.*simulate_bank"):
        knode.simulate_batch(robot, ctl, robots=robots, per_robot_nn=True, key_points=[3])


def test_binding_routes_and_refuses_before_the_library(kn):
    H = kn.Handle
    B, T = 3, 5
    ctl = np.zeros((B, T, 4))
    me = object.__new__(H)
    # a bank that is none, a bank without its index array, loads next to a bank (the hint: the wrench rides in bnd)
    with pytest.raises(kn.KrError, match="MlpBank"):
        H.simulate(me, ctl, None, None, table=object(), bank=object(), net_of_rod=[0] * B, bnd=ctl)
    with pytest.raises(kn.KrError, match="net_of_rod"):
        H.simulate(me, ctl, None, None, table=object(), net_of_rod=[0] * B, bnd=ctl, key_points=[3], kp=ctl)
    with pytest.raises(kn.KrError, match="last six columns of bnd"):
        H.simulate(me, ctl, None, None, table=object(), bank=object(), net_of_rod=[0] * B, loads=ctl)
    with pytest.raises(kn.KrError, match="last six columns of bnd"):
        H.simulate(me, ctl, None, None, table=object(), bank=object(), net_of_rod=[0] * B, loads=ctl, bnd=ctl)
    # repack: the shape of the bank, checked on the host
    bank = object.__new__(kn.MlpBank)
    bank._b, bank.K, bank.dims, bank.acts = ctypes.c_void_p(1), 2, (28, 64, 25), (kn.ACT_ELU, kn.ACT_NONE)
    two = cases.bank(2)
    net = lambda m: (m.weights, m.biases, m.acts)
    with pytest.raises(kn.KrError, match="repack takes 2 networks"):
        bank.repack([net(two[0])])
    with pytest.raises(kn.KrError, match="repack takes 2 networks of layers"):
        bank.repack([net(m) for m in cases.bank(3)[:2]])
    bank._b = None  # (nothing to free)


def test_oracle_loop_reproduces_the_reference():
    """tests/golden/bank_motion.npz: the unmodified reference with an injected network and p0 / h0 / q0 / w0 / F_tip / M_tip
    assigned before every solve, four rods over three networks of one shape."""
    import cosserat_oracle as orc
    g = load_golden("bank_motion")
    case = cases.FIXTURE
    N, T = case["N"], case["T"]
    assert np.all(g["ier"] == 1) and g["ier"].shape == (4, T) and g["traj"].shape == (4, T, 25, N)
    assert [str(r[0]) for r in case["rows"]] == list(g["mods"]) and g["nets"].tolist() == cases.nets_of(case, case["bank"])
    assert len(set(g["nets"].tolist())) >= 2
    assert np.array_equal(g["bnd"], cases.bnd_of(case))
    # the weights the fixture stores are the bank's
    for k, mlp in enumerate(cases.bank(case["bank"])):
        stored = orc.mlp_from_arrays(g, f"net{k}")
        assert all(np.array_equal(a, b) for a, b in zip(stored.weights + stored.biases, mlp.weights + mlp.biases))
    worst = 0.0
    for b, row in enumerate(case["rows"]):
        mlp = orc.mlp_from_arrays(g, f"net{int(g['nets'][b])}")
        states, ok, it = cases.oracle_loop(orc.setup_params(row[0], N), g["ctl"], g["bnd"][b, :, :13], g["bnd"][b, :, 13:], mlp=mlp)
        assert np.all(ok), (b, ok)
        err = rel_l2(states[:T, :25], g["traj"][b])
        print(f"rod {b} ({row}): oracle loop against the reference {err:.3e} (bound 1e-08)")
        worst = max(worst, err)
        # the network and the histories matter far beyond the bound: without either the rod is another one
        bare, _, _ = cases.oracle_loop(orc.setup_params(row[0], N), g["ctl"], g["bnd"][b, :, :13], g["bnd"][b, :, 13:])
        assert rel_l2(bare[:T, :3, -1], g["tips"][b]) > 1e-3
    assert worst < 1e-8, worst
