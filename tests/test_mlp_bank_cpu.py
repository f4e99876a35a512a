"""Per-rod networks, host side (no GPU): ``kr_mlp_bank_check`` - which bank shapes ``kr_simulate_batch_bank`` serves -
the argument validation of ``knode.simulate_batch(..., robots=[...], per_robot_nn=True)``, which raises before anything
touches a device, and the oracle cases the GPU tests compare against."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mlp_bank_cases as cases
from conftest import ROOT
from gpu_helpers import inject

ELU, NONE, TANH = 4, 0, 1


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    assert (kn.ACT_ELU, kn.ACT_NONE, kn.ACT_TANH) == (ELU, NONE, TANH)
    return kn


def preset_robot(mod, N=20):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r, mod)
    r.N = N
    r.compute_intermediate_terms()
    return r


def test_the_two_bank_shapes_are_served(kn):
    base = preset_robot(None)._params()
    for N in (20, 100):
        base.N = N
        for K in (1, 4, 64):
            assert kn.mlp_bank_check(base, K, [28, 64, 64, 25], [ELU, ELU, NONE]) == (0, "")
            assert kn.mlp_bank_check(base, K, [28, 64, 25], [ELU, NONE]) == (0, "")


def test_refusals_name_the_rule(kn):
    base = preset_robot(None)._params()
    rc, msg = kn.mlp_bank_check(base, 0, [28, 64, 64, 25], [ELU, ELU, NONE])
    assert rc == kn.KR_E_ARG and "K" in msg, msg
    rc, msg = kn.mlp_bank_check(base, -3, [28, 64, 25], [ELU, NONE])
    assert rc == kn.KR_E_ARG and "K" in msg, msg
    # the 53-input history form, by the shape and by the base parameters
    rc, msg = kn.mlp_bank_check(base, 2, [53, 64, 64, 25], [ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "nn_input_history" in msg, msg
    hist = preset_robot(None)._params()
    hist.nn_input_history = 1
    rc, msg = kn.mlp_bank_check(hist, 2, [28, 64, 64, 25], [ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "nn_input_history" in msg, msg
    rc, msg = kn.mlp_bank_check(base, 2, [28, 64, 64, 25], [ELU, TANH, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "mixed activations" in msg, msg
    for H1 in (65, 128):
        rc, msg = kn.mlp_bank_check(base, 2, [28, H1, 64, 25], [ELU, ELU, NONE])
        assert rc == kn.KR_E_UNSUPPORTED and "first hidden layer" in msg and str(H1) in msg, msg
    rc, msg = kn.mlp_bank_check(base, 2, [28, 64, 193, 25], [ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "second hidden layer" in msg, msg
    rc, msg = kn.mlp_bank_check(base, 2, [28, 64, 64, 25], [ELU, ELU, ELU])
    assert rc == kn.KR_E_UNSUPPORTED and "output layer" in msg, msg
    rc, msg = kn.mlp_bank_check(base, 2, [28, 64, 64, 64, 25], [ELU, ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "layers" in msg, msg
    # malformed shapes are argument errors
    assert kn.mlp_bank_check(base, 2, [28, 64, 24], [ELU, NONE])[0] == kn.KR_E_ARG
    assert kn.mlp_bank_check(base, 2, [28, 0, 25], [ELU, NONE])[0] == kn.KR_E_ARG
    assert kn.mlp_bank_check(base, 2, [28, 64, 25], [9, NONE])[0] == kn.KR_E_ARG
    # the grid sizes of the one-wavefront persistent kernel
    for N, want in ((8, kn.KR_E_UNSUPPORTED), (9, 0), (128, 0), (129, kn.KR_E_UNSUPPORTED)):
        base.N = N
        rc, msg = kn.mlp_bank_check(base, 2, [28, 64, 25], [ELU, NONE])
        assert rc == want and (rc == 0 or "N = " in msg), (N, rc, msg)
    lib = kn.load()
    dims = (ctypes.c_int32 * 3)(28, 64, 25)
    acts = (ctypes.c_int32 * 2)(ELU, NONE)
    assert lib.kr_mlp_bank_check(None, 1, 2, dims, acts) == kn.KR_E_ARG
    assert lib.kr_mlp_bank_check(ctypes.byref(base), 1, 2, None, acts) == kn.KR_E_ARG


def test_simulate_batch_validates_networks_before_any_device_call(kn, monkeypatch):
    import cosserat_oracle as orc
    import knode
    from cosserat_ode import CosseratRod

    def no_device(self):
        raise AssertionError("simulate_batch touched the device before validating the robots' networks")
    monkeypatch.setattr(CosseratRod, "_native", no_device)
    nets3, nets2 = cases.bank_three(), cases.bank_two()

    def with_net(mod, mlp):
        r = preset_robot(mod)
        if mlp is not None:
            inject(r, mlp)
        return r
    carrier = preset_robot(None)
    ctl = np.zeros((3, 5, 4))
    with pytest.raises(kn.KrError, match="needs robots"):
        knode.simulate_batch(carrier, ctl, per_robot_nn=True)
    with pytest.raises(kn.KrError, match="2 rods"):  # a length mismatch
        knode.simulate_batch(carrier, ctl, robots=[with_net(None, nets3[0]), with_net("short", nets3[1])], per_robot_nn=True)
    with pytest.raises(kn.KrError, match=r"rod 1.*needs a network"):  # a robot without a network
        knode.simulate_batch(carrier, ctl, per_robot_nn=True,
                             robots=[with_net(None, nets3[0]), with_net("short", None), with_net("nsw", nets3[1])])
    with pytest.raises(kn.KrError, match=r"rod 2.*layers"):  # mismatched layer strings
        knode.simulate_batch(carrier, ctl, per_robot_nn=True,
                             robots=[with_net(None, nets3[0]), with_net("short", nets3[1]), with_net("nsw", nets2[1])])
    tanh = orc.make_mlp([28, 64, 64, 25], "tanh", seed=5)
    with pytest.raises(kn.KrError, match=r"rod 1.*layers"):
        knode.simulate_batch(carrier, ctl, per_robot_nn=True,
                             robots=[with_net(None, nets3[0]), with_net("short", tanh), with_net("nsw", nets3[1])])
    hist = with_net("damping", nets3[2])
    hist.nn_input_history = True
    with pytest.raises(kn.KrError, match=r"rod 2.*nn_input_history"):
        knode.simulate_batch(carrier, ctl, per_robot_nn=True, robots=[with_net(None, nets3[0]), with_net("short", nets3[1]), hist])
    # a shape the bank kernels do not serve: refused by the library's host check, still before any device call
    wide = [orc.make_mlp([28, 128, 64, 25], "elu", seed=s) for s in (1, 2, 1)]
    with pytest.raises(kn.KrError) as e:
        knode.simulate_batch(carrier, ctl, per_robot_nn=True, robots=[with_net(None, w) for w in wide])
    assert e.value.code == kn.KR_E_UNSUPPORTED and "first hidden layer" in str(e.value)


def test_networks_are_deduplicated_by_digest(kn):
    import knode
    nets3 = cases.bank_three()
    carrier = preset_robot(None)
    robots = []
    for mod, k in zip(cases.CASE_THREE["mods"], cases.CASE_THREE["nets"]):
        r = preset_robot(mod)
        inject(r, nets3[k])
        robots.append(r)
    networks, net_of_rod = knode._robots_networks(carrier, robots)
    assert len(networks) == 4 and net_of_rod == list(cases.CASE_THREE["nets"])
    for k in range(4):
        for a, b in zip(networks[k][0], nets3[k].weights):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ["CASE_THREE", "CASE_TWO", "CASE_N100"])
def test_oracle_cases_converge_and_tell_networks_apart(case):
    """The GPU tests compare against these trajectories: every step of every rod has ``ier == 1`` (asserted where the
    reference is computed), and on one parameter set two networks give tips that differ by far more than any tolerance
    - a rod served the wrong network cannot pass.  (The N = 100 case takes a few seconds of oracle time.)"""
    c = getattr(cases, case)
    refs = cases.oracle_case(c)
    assert len(refs) == len(c["mods"]) and all(r.shape == (c["steps"], 25, c["N"]) for r in refs)
    if case == "CASE_THREE":
        a = cases.oracle_rod(20, None, 3, 0, 20)[:, :3, -1]
        for k in (1, 2, 3):
            d = np.linalg.norm(cases.oracle_rod(20, None, 3, k, 20)[:, :3, -1] - a) / np.linalg.norm(a)
            print(f"plain preset, network {k} against network 0: tips differ by {d:.3e} relative")
            assert d > 1e-3
