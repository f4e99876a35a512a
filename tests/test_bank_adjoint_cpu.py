"""CPU tier of the bank adjoint (kr_step_vjp_bank_batch, kr_simulate_vjp_bank_batch, krod_grad.rollout_grad_bank /
simulate_tips_bank): the C ABI surface, the argument checks that need no device, the fixture's self-consistency, and the
composition the calls are defined as - restated in NumPy with per-rod rows AND per-rod networks
(bank_adjoint_cases.numpy_rollout_adjoint) - held to the fixture the GPU tests compare with.  Three mutants of it show that the
fixture tells the networks, the per-network sums and the rows apart.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import bank_adjoint_cases as bc
import nn_adjoint_cases as nc
import step_adjoint_cases as sc
from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = ("kr_step_vjp_bank_batch", "kr_simulate_vjp_bank_batch")
MUTANT_FAMILY = "tanh17"


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


@pytest.fixture(scope="module")
def fx():
    return load_golden("bank_adjoint")


def test_bank_symbols_declared_exported_and_bound(lib):
    """The header declares both calls, cites the reference lines they differentiate and says what they do not serve; the
    library exports them and krod_native binds them with the header's argument count; a null handle, table or bank is
    refused without a device and no output byte is written; nothing in the header still says that a bank has no adjoint."""
    import krod_native as kn
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name in SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert proto, f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == proto.group(1).count(",") + 1, name
        for arg in ("const kr_param_table* t", "const kr_mlp_bank* bank", "const int32_t* net_of_rod_host", "nn_x", "nn_g"):
            assert arg in proto.group(1), (name, arg)
        assert "g_par" not in proto.group(1) and "int64_t B" not in proto.group(1) and "use_nn" not in proto.group(1)
    assert "bnd_per_step" in re.search(r"\bint\s+kr_simulate_vjp_bank_batch\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert "by nothing yet" not in text
    doc = text[text.index("the adjoint of a heterogeneous batch with the MLP on"):]
    for word in ("knode.py:70-100", "cosserat_ode.py:178-184", "physics_multitrain.py:181-199", "g_par with the network on", "RK4",
                 "53-wide", "full matrices", "ROD order", "[0, K)", "bnd_per_step == 1"):
        assert word in doc, word
    out = (ctypes.c_double * 43)(*([7.0] * 43))
    buf = (ctypes.c_double * 64)()
    nets = (ctypes.c_int32 * 4)()
    assert lib.kr_step_vjp_bank_batch(None, None, None, nets, kn.KR_EULER, buf, buf, buf, buf, buf, out, out, out, out, None, None, out,
                                      out, kn.KR_F64, None) == kn.KR_E_ARG and b"handle" in lib.kr_last_error()
    assert lib.kr_simulate_vjp_bank_batch(None, None, None, nets, 1, kn.KR_EULER, buf, buf, None, out, None, out, out, 1, None, None, out,
                                          out, kn.KR_F64, None) == kn.KR_E_ARG and b"handle" in lib.kr_last_error()
    assert list(out) == [7.0] * 43


class _Robot:
    """stands in for a CosseratRod in the checks that come before any library or device work"""
    _use_nn = True

    def _native(self, push_mlp=True):
        raise AssertionError("the argument checks come before the device is touched")

    def _params(self):
        raise AssertionError("the argument checks come before the library's rows are made")


def test_bank_calls_check_their_arguments():
    """wrong shapes, a ragged bank, indices outside [0, K), len(robots) != B: KrError before anything runs"""
    import torch
    import krod_grad as kg
    import krod_native as kn
    r, B, T = _Robot(), 2, 3
    robots = [_Robot(), _Robot()]
    ctl = torch.zeros((B, T, 4))
    net = lambda h=5: [torch.zeros((h, 28)), torch.zeros(h), torch.zeros((25, h)), torch.zeros(25)]
    params = [net(), net()]
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.simulate_tips_bank(r, robots, np.zeros((B, T, 4)), params, [0, 1])
    with pytest.raises(kn.KrError, match=r"\[B, T, 4\]"):
        kg.simulate_tips_bank(r, robots, torch.zeros((B, T, 5)), params, [0, 1])
    with pytest.raises(kn.KrError, match="list of K per-network lists"):
        kg.simulate_tips_bank(r, robots, ctl, net(), [0, 1])
    with pytest.raises(kn.KrError, match="network 1 has another shape than network 0"):
        kg.simulate_tips_bank(r, robots, ctl, [net(), net(6)], [0, 1])
    with pytest.raises(kn.KrError, match=r"network 1: params\[2\] takes 5 inputs, the layer before gives 4"):
        kg.simulate_tips_bank(r, robots, ctl, [net(), [torch.zeros((4, 28)), torch.zeros(4), torch.zeros((25, 5)), torch.zeros(25)]], [0, 1])
    with pytest.raises(kn.KrError, match=r"net_of_rod must hold one integer per rod \(2\)"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0, 1, 0])
    with pytest.raises(kn.KrError, match=r"net_of_rod must hold one integer per rod"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0.0, 1.0])
    with pytest.raises(kn.KrError, match=r"net_of_rod must lie in \[0, 2\); got 0 \.\. 2"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0, 2])
    with pytest.raises(kn.KrError, match=r"net_of_rod must lie in \[0, 2\); got -1 \.\. 1"):
        kg.simulate_tips_bank(r, robots, ctl, params, [-1, 1])
    with pytest.raises(kn.KrError, match=r"base_motion must be \[B, T, 13\] = \[2, 3, 13\]"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0, 1], base_motion=torch.zeros((B, T, 19)))
    with pytest.raises(kn.KrError, match=r"tip_loads must be \[B, T, 6\] = \[2, 3, 6\]"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0, 1], tip_loads=np.zeros((T, 6)))
    with pytest.raises(kn.KrError, match="robots holds 3 rods, ctl 2"):
        kg.simulate_tips_bank(r, robots + [_Robot()], ctl, params, [0, 1])
    with pytest.raises(kn.KrError, match="unsupported dtype"):
        kg.simulate_tips_bank(r, robots, ctl, params, [0, 1], dtype="f16")
    g_tips, states = np.zeros((B, T, 3)), np.zeros((T + 1, B, 5, kn.KR_SLOTS))
    with pytest.raises(kn.KrError, match="give g_states and / or g_tips"):
        kg.rollout_grad_bank(r, robots, np.zeros((B, T, 4)), states, params, [0, 1])
    with pytest.raises(kn.KrError, match="full history"):
        kg.rollout_grad_bank(r, robots, np.zeros((B, T, 4)), states[:3], params, [0, 1], g_tips=g_tips)
    with pytest.raises(kn.KrError, match=r"net_of_rod must lie in \[0, 2\)"):
        kg.rollout_grad_bank(r, robots, np.zeros((B, T, 4)), states, params, [1, 2], g_tips=g_tips)
    with pytest.raises(kn.KrError, match="robots holds 1 rods, ctl 2"):
        kg.rollout_grad_bank(r, [_Robot()], np.zeros((B, T, 4)), states, params, [0, 1], g_tips=g_tips)


def test_fixture_is_self_consistent(fx):
    """The file carries a tolerance for every compared block; each is the rule applied to the file's own two step sizes, is
    positive exactly where a block is not identically zero, and stays within MAX_REL_TOL of its block; the rods, rows and
    networks are the cases'; network 2 has no rod and therefore no weight block."""
    assert list(fx["net_of_rod"]) == list(bc.NET_OF_ROD) == [1, 0, 1, 1, 0] and list(fx["row_of_rod"]) == list(bc.ROW_OF_ROD)
    assert float(fx["H"]) == sc.H and float(fx["H_STATE"]) == bc.H_STATE
    n_blocks = 0
    for fam in bc.FAMILIES:
        nets = bc.fixture_networks(fx, fam)
        for k, (a, b) in enumerate(zip(nets, bc.networks(fam))):
            assert all(np.array_equal(u, v) for u, v in zip(a.weights + a.biases, b.weights + b.biases)), (fam, k)
        assert not np.array_equal(nets[0].weights[0], nets[1].weights[0])
        xb = bc.x_blocks(bc.T_FIX, False)
        for b in range(bc.B_FIX):
            kb, rc = bc.key(fam, b), bc.fixture_case(fx, fam, b, nets)
            assert np.array_equal(rc["bnd"], bc.boundary_history(rc["P"], b, bc.T_FIX)) and np.ptp(rc["bnd"][:, 0]) > 0 and np.ptp(rc["bnd"][:, 13]) > 0
            for c in range(2):
                tol = bc.x_tols(fx[kb + "x_fd_h"][c], fx[kb + "x_fd_2h"][c], bc.x_floor(rc, c))
                assert np.array_equal(tol, fx[kb + "x_tol"][c]), (kb, c)
                for (name, idx), t in zip(xb, tol):
                    size = float(np.max(np.abs(fx[kb + "x_fd_h"][c][idx])))
                    assert (t > 0) == (size > 0) and t <= bc.MAX_REL_TOL * size, (kb, c, name, t, size)
                    n_blocks += t > 0
            for t in bc.STEP_TS:
                x, nxt, _ = bc.step_inputs(rc, t)
                for c in range(3):
                    tol = bc.step_tols(fx[kb + f"s{t}_fd_h"][c], fx[kb + f"s{t}_fd_2h"][c], bc.step_floor(fx[kb + f"s{t}_gbar"][c], nxt))
                    assert np.array_equal(tol, fx[kb + f"s{t}_tol"][c]), (kb, t, c)
                    a = sc.split_grad(fx[kb + f"s{t}_fd_h"][c], bc.N_FIX)
                    for (name, arr, sl), tt in zip(sc.BLOCKS, tol):
                        size = float(np.max(np.abs(a[arr][..., sl])))
                        assert (tt > 0) == (size > 0) and tt <= bc.MAX_REL_TOL * size, (kb, t, c, name, tt, size)
                        n_blocks += tt > 0
        for k in range(bc.K_FIX):
            kk = f"{fam}_net{k}_"
            if not bc.rods_of(k):
                assert kk + "wfd_h" not in fx.files if hasattr(fx, "files") else kk + "wfd_h" not in fx
                continue
            for c in range(2):
                w_h, w_2h, tol = fx[kk + "wfd_h"][c], fx[kk + "wfd_2h"][c], fx[kk + "w_tol"][c]
                assert len(w_h) == 6 * len(nets[0].weights) == 6 * len(tol)
                for l, t in enumerate(tol):
                    a, b = w_h[6 * l:6 * l + 6], w_2h[6 * l:6 * l + 6]
                    assert 10.0 * np.max(np.abs(a - b)) < t <= bc.MAX_REL_TOL * np.max(np.abs(a)), (kk, c, l)
                    n_blocks += 1
    print(f"{n_blocks} compared blocks carry a tolerance")
    assert n_blocks > 500


def _rollout_gradients(fx, fam, c, row_of=None, net_of=None):
    """the NumPy composition for every rod of a family: (gx per rod, X per rod, C per rod) with rod b on row row_of[b] and
    network net_of[b] (default: its own)"""
    nets = bc.fixture_networks(fx, fam)
    out = []
    for b in range(bc.B_FIX):
        rc = bc.fixture_case(fx, fam, b, nets)
        P = rc["P"] if row_of is None else sc.params(bc.SETS[row_of[b]], bc.N_FIX)
        mlp = rc["mlp"] if net_of is None else nets[net_of[b]]
        out.append(bc.numpy_rollout_adjoint(P, mlp, rc, c))
    return nets, out


@pytest.fixture(scope="module")
def truth(fx):
    return {fam: _rollout_gradients(fx, fam, 0) for fam in bc.FAMILIES}


@pytest.mark.parametrize("fam", bc.FAMILIES)
def test_numpy_composition_agrees_with_the_fixture(fx, truth, fam):
    """The composition of step adjoints with row b and network net_of_rod[b], in NumPy, against the oracle's differences:
    every input block of every rod, and the weight blocks of every network with rods from the rows of ITS rods."""
    nets, res = truth[fam]
    worst = {}
    for b in range(bc.B_FIX):
        kb = bc.key(fam, b)
        bc.x_check(f"{kb} numpy", res[b]["gx"], fx[kb + "x_fd_h"][0], fx[kb + "x_tol"][0], worst)
    for k in range(bc.K_FIX):
        rods = bc.rods_of(k)
        if not rods: continue
        gw = bc.weight_grad(nets[k], np.stack([res[b]["X"] for b in rods], axis=1), np.stack([res[b]["C"] for b in rods], axis=1))
        bc.w_check(f"{fam}_net{k} numpy", gw, fx[f"{fam}_net{k}_wfd_h"][0], fx[f"{fam}_net{k}_w_tol"][0], worst)
    print(f"{fam}: largest err / tol {max(worst.values()):.3f}")


def _worst_miss(fx, fam, res, nets, per_network=True):
    miss = []
    for b in range(bc.B_FIX):
        kb = bc.key(fam, b)
        miss += [(f"rod {b} {n}", r) for n, r in bc.x_misses(res[b]["gx"], fx[kb + "x_fd_h"][0], fx[kb + "x_tol"][0])]
    for k in range(bc.K_FIX):
        if not bc.rods_of(k): continue
        rods = bc.rods_of(k) if per_network else list(range(bc.B_FIX))
        gw = bc.weight_grad(nets[k], np.stack([res[b]["X"] for b in rods], axis=1), np.stack([res[b]["C"] for b in rods], axis=1))
        miss += [(f"net {k} {n}", r) for n, r in bc.w_misses(gw, fx[f"{fam}_net{k}_wfd_h"][0], fx[f"{fam}_net{k}_w_tol"][0])]
    return sorted(miss, key=lambda m: -m[1])


def test_mutant_networks_swapped_between_rods_is_caught(fx):
    """rods of network 0 on network 1 and the other way round, on the stored states: blocks miss by more than ten tolerances"""
    swap = [{0: 1, 1: 0}.get(k, k) for k in bc.NET_OF_ROD]
    nets, res = _rollout_gradients(fx, MUTANT_FAMILY, 0, net_of=swap)
    miss = _worst_miss(fx, MUTANT_FAMILY, res, nets)
    print("networks swapped:", miss[:5])
    assert miss[0][1] > 10.0
    for b in range(bc.B_FIX):  # every rod is on the wrong network: every rod is caught
        assert max(r for n, r in miss if n.startswith(f"rod {b} ")) > 10.0, b


def test_mutant_weight_gradient_summed_over_all_rods_is_caught(fx, truth):
    """the right rows, but network k's gradient taken over EVERY rod's rows instead of its own rods': the input blocks all
    pass and a weight block of each network misses by more than ten tolerances"""
    nets, res = truth[MUTANT_FAMILY]
    miss = _worst_miss(fx, MUTANT_FAMILY, res, nets, per_network=False)
    print("weight gradient over all rods:", miss[:5])
    assert all(r <= 1.0 for n, r in miss if n.startswith("rod "))
    for k in (0, 1):
        assert max(r for n, r in miss if n.startswith(f"net {k} ")) > 10.0, k


def test_mutant_every_rod_on_row_0_is_caught(fx):
    """every rod with the constants of row 0: the rods of the other rows miss by more than ten tolerances, the rods of row 0
    (0 and 4) are untouched"""
    nets, res = _rollout_gradients(fx, MUTANT_FAMILY, 0, row_of=[0] * bc.B_FIX)
    miss = _worst_miss(fx, MUTANT_FAMILY, res, nets)
    print("every rod on row 0:", miss[:5])
    for b in range(bc.B_FIX):
        worst = max(r for n, r in miss if n.startswith(f"rod {b} "))
        if bc.ROW_OF_ROD[b] == 0: assert worst <= 1.0, (b, worst)
        else: assert worst > 10.0, (b, worst)
