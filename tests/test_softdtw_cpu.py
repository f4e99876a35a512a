"""CPU tier of soft-DTW on the device (kr_softdtw_batch): the host statement ``krod_eval.softdtw_grad`` against the 50-digit
fixture within the two derived bounds (tests/softdtw_cases.py), the exact 1 x 1 table, the sandwich between the hard DTW and
DTW - n gamma ln 3, the test of the tests (five mistakes a kernel could make miss the bounds wherever they can be felt, and
are asserted invisible where they cannot), the C ABI surface and the refusals that need no device.  No kernel is launched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import softdtw_cases as sc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = {"kr_softdtw_ws_bytes": ("size_t", ctypes.c_size_t), "kr_softdtw_batch": ("int", ctypes.c_int)}
SHAPES = {(1, 1), (1, 5), (5, 1), (2, 3), (63, 65), (64, 64), (65, 64), (101, 101), (40, 130), (130, 67), (129, 200), (40, 70)}


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_fixture_holds_the_cases_of_the_contract():
    fx = sc.fixture()
    assert len(fx) == 11 * 2 * 3 + 6
    assert {(len(c["a"]), len(c["b"])) for c in fx.values()} == SHAPES
    for shape in SHAPES:
        got = {(c["cost"], c["gamma"]) for c in fx.values() if (len(c["a"]), len(c["b"])) == shape}
        assert got == {(k, g) for k in ("l1", "sq") for g in (1e-6, 1e-3, 1e-1)}, shape
    warp = [c for n, c in fx.items() if n.startswith("warp")]
    assert len(warp) == 6 and all((c["a"][:, None, :] == c["b"][None, :, :]).all(-1).any(0).all() for c in warp)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "softdtw.npz")) < 1 << 20


@pytest.mark.parametrize("name", sc.names())
def test_host_statement_meets_the_bounds(name):
    import krod_eval as ke
    c = sc.fixture()[name]
    value, g = ke.softdtw_grad(c["a"], c["b"], c["gamma"], c["cost"])
    rv, rg = sc.ratios(c, value, g)
    print(f"{name}: value error / tolR = {rv:.3g}, gradient error / tolG = {rg:.3g}")
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)
    assert ke.softdtw_distance(c["a"], c["b"], c["gamma"], c["cost"]) == value
    # the second statement (one cell at a time, the C library's exp and log), which the mutants are made of, meets them too
    assert max(sc.ratios(c, *sc.statement(c["a"], c["b"], c["gamma"], c["cost"]))) <= 1.0


@pytest.mark.parametrize("cost", ["l1", "sq"])
@pytest.mark.parametrize("gamma", [1e-6, 1e-3, 1e-1])
def test_one_by_one_is_exact(cost, gamma):
    import krod_eval as ke
    c = sc.fixture()[f"1x1_c{0 if cost == 'l1' else 1}_g{gamma:g}"]
    d = c["a"][0] - c["b"][0]
    want = (abs(d[0]) + abs(d[1])) + abs(d[2]) if cost == "l1" else (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    value, g = ke.softdtw_grad(c["a"], c["b"], gamma, cost)
    assert value == want
    assert np.array_equal(g, (np.sign(d) if cost == "l1" else 2.0 * d)[None, :])


@pytest.mark.parametrize("name", [n for n in sc.names() if "_c0_" in n])
def test_sandwich_against_the_hard_dtw(name):
    """softmin <= min and min - softmin <= gamma ln 3 per cell: dtw - n gamma ln 3 - tolR <= value <= dtw + tolR"""
    import krod_eval as ke
    c = sc.fixture()[name]
    Ta, Tb = len(c["a"]), len(c["b"])
    n, tr = Ta + Tb - 1, sc.tol_R(Ta, Tb, c["gamma"], c["Rmax"])
    dtw = ke.dtw_distance(c["a"], c["b"])
    value = ke.softdtw_distance(c["a"], c["b"], c["gamma"], "l1")
    assert dtw - c["gamma"] * np.log(3.0) * n - tr <= value <= dtw + tr, (dtw, value)


def _seen(c, mutant):
    """by how many bounds the mutant misses the case: max of the two ratios"""
    value, g = sc.statement(c["a"], c["b"], c["gamma"], c["cost"], mutant)
    return max(sc.ratios(c, value, g))


def _same(c, mutant):
    v0, g0 = sc.statement(c["a"], c["b"], c["gamma"], c["cost"])
    v1, g1 = sc.statement(c["a"], c["b"], c["gamma"], c["cost"], mutant)
    return v0 == v1 and np.array_equal(g0, g1)


def _structure(c):
    """mutant -> can the mistake touch a table of this shape and cost at all"""
    Ta, Tb = len(c["a"]), len(c["b"])
    return {"diag_cost": Ta >= 2 and Tb >= 2,       # needs a diagonal successor
            "edge_row": Tb > 64 and Ta >= 2,        # needs a second stripe and a second row
            "corner": True,                         # zeroes every E
            "sign_d": c["cost"] == "l1",            # is the L1 derivative, absent from the squared cost
            "no_log": min(Ta, Tb) >= 2}             # one row or one column: one warp path, no minimum to soften


@pytest.mark.parametrize("name", sc.names())
def test_mutants_of_the_statement_miss_the_bounds(name):
    """The bounds separate the definition from five mistakes a kernel could make.
    Where the shape or the cost keeps the mistake out of the table (_structure), the mutant IS the statement, bit for bit.
    Where it can get in and the table is soft - gamma >= 1e-3, not small against the gaps between neighbouring warp paths (the
    walks step by 2e-3), so every cell near the optimal path carries weight - the mutant misses a bound by at least ten bounds.
    At gamma = 1e-6 the table has hardened to a single warp path and a mistake is felt only if it lies on that path:
    softdtw_cases.HARD_UNSEEN records, case by case, the mutants that are let in and NOT seen, and says why; those stay within
    the bounds (asserted), every other one misses by ten bounds (asserted), so a change that makes a mutant invisible on a case
    that sees it today fails here.  The hard minimum (no_log) is held to the sandwich 0 <= mutant - value <= n gamma ln 3 too."""
    c = sc.fixture()[name]
    Ta, Tb, gamma = len(c["a"]), len(c["b"]), c["gamma"]
    assert gamma >= 1e-3 or gamma == 1e-6
    unseen = sc.HARD_UNSEEN.get(name, ())
    for mutant, can in _structure(c).items():
        if not can:
            assert _same(c, mutant), mutant
            assert mutant not in unseen, mutant  # (the record holds only what the shape lets in)
        elif mutant in unseen:
            assert _seen(c, mutant) <= 1.0, mutant
        else:
            assert _seen(c, mutant) >= 10.0, mutant
    if gamma < 1e-3 and min(Ta, Tb) >= 2:
        hard = sc.statement(c["a"], c["b"], gamma, c["cost"], "no_log")[0]
        tr = sc.tol_R(Ta, Tb, gamma, c["Rmax"])
        assert -tr <= hard - c["value"] <= (Ta + Tb - 1) * gamma * np.log(3.0) + tr


def test_the_record_of_unseen_mutants_names_hard_cases_only():
    """HARD_UNSEEN holds fixture cases at gamma = 1e-6 and known mutants, and at that gamma every mutant is still seen by a case"""
    fx = sc.fixture()
    for name, mutants in sc.HARD_UNSEEN.items():
        assert name in fx and fx[name]["gamma"] == 1e-6 and set(mutants) <= set(sc.MUTANTS), name
    hard = [n for n, c in fx.items() if c["gamma"] == 1e-6]
    for mutant in sc.MUTANTS:
        assert any(_structure(fx[n])[mutant] and mutant not in sc.HARD_UNSEEN.get(n, ()) for n in hard), mutant


def test_softdtw_symbols_declared_exported_and_bound(lib):
    import krod_native as kn
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name, (ctype, restype) in SYMBOLS.items():
        proto = re.search(r"\b" + ctype + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert proto, f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is restype
        assert len(getattr(lib, name).argtypes) == proto.group(1).count(",") + 1, name
    assert int(re.search(r"#define\s+KR_SOFTDTW_MAX_LEN\s+(\d+)", src).group(1)) == kn.KR_SOFTDTW_MAX_LEN == 1024
    assert hasattr(kn.Handle, "softdtw")
    import krod_eval as ke
    assert kn.SOFTDTW_COSTS == ke.SOFTDTW_COSTS == {"l1": 0, "sq": 1}


def test_softdtw_refuses_a_null_handle(lib):
    """The first check needs no device: a null handle is KR_E_ARG with a message, and no output byte is written."""
    import krod_native as kn
    value = (ctypes.c_double * 2)(7.0, 7.0)
    g = (ctypes.c_double * 12)(*([7.0] * 12))
    buf = (ctypes.c_double * 64)()
    rc = lib.kr_softdtw_batch(None, 1, buf, 2, 6, 3, buf, 2, 6, 3, 1e-2, 0, value, g, 6, 3, None, kn.KR_F64, None)
    assert rc == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert list(value) == [7.0, 7.0] and list(g) == [7.0] * 12


def test_softdtw_workspace_size(lib):
    """0 for value only, for what the LDS holds and for what is refused; else the stripe-major table, a multiple of 16"""
    import krod_native as kn
    L = kn.KR_SOFTDTW_MAX_LEN
    for B, Ta, Tb in ((1, 1, 1), (5, 33, 37), (3, 40, 70), (1024, 5, 4)):
        assert int(lib.kr_softdtw_ws_bytes(B, Ta, Tb, 1)) == 0, (B, Ta, Tb)
    for B, Ta, Tb in ((3, 64, 64), (1, 101, 101), (1024, 101, 101), (3, 40, 130), (1, L, L)):
        n = int(lib.kr_softdtw_ws_bytes(B, Ta, Tb, 1))
        assert n == B * ((Tb + 63) // 64) * (Ta + 63) * 64 * 8 and n % 16 == 0, (B, Ta, Tb, n)
        assert int(lib.kr_softdtw_ws_bytes(B, Ta, Tb, 0)) == 0
    assert int(lib.kr_softdtw_ws_bytes(0, 101, 101, 1)) == 0 and int(lib.kr_softdtw_ws_bytes(1, L + 1, 9, 1)) == 0


def test_python_layer_refusals_without_a_device():
    import torch
    import krod_eval as ke
    import krod_grad as kg
    import krod_native as kn
    for gamma in (0.0, -1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(kn.KrError, match="gamma"):
            kn.softdtw_args(gamma, "l1")
    for cost in ("l2", 0, None):
        with pytest.raises(kn.KrError, match="cost"):
            kn.softdtw_args(1e-2, cost)
    with pytest.raises(kn.KrError, match="at most") as e:
        kn.softdtw_args(1e-2, "l1", kn.KR_SOFTDTW_MAX_LEN + 1, 4)
    assert e.value.code == kn.KR_E_UNSUPPORTED
    assert kn.softdtw_args(1e-2, "sq", kn.KR_SOFTDTW_MAX_LEN, 1) == (1e-2, 1)
    tips, ref = torch.zeros((2, 5, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64)
    # (robot = None: every refusal below comes before the handle is asked for)
    with pytest.raises(kn.KrError, match="torch tensor"):
        kg.softdtw_loss(None, tips.numpy(), ref, 1e-2)
    with pytest.raises(kn.KrError, match=r"\[B, T, 3\]"):
        kg.softdtw_loss(None, tips[0], ref, 1e-2)
    with pytest.raises(kn.KrError, match="float32 or float64"):
        kg.softdtw_loss(None, tips.to(torch.float16), ref, 1e-2)
    with pytest.raises(kn.KrError, match="ref must be"):
        kg.softdtw_loss(None, tips, torch.zeros((3, 4, 3), dtype=torch.float64), 1e-2)
    with pytest.raises(kn.KrError, match="ref requires grad"):
        kg.softdtw_loss(None, tips, ref.clone().requires_grad_(True), 1e-2)
    with pytest.raises(kn.KrError, match="gamma"):
        kg.softdtw_loss(None, tips, ref, 0.0)
    with pytest.raises(kn.KrError, match="cost"):
        kg.softdtw_loss(None, tips, ref, 1e-2, cost="l2")
    with pytest.raises(kn.KrError, match="at most"):
        kg.softdtw_loss(None, tips, torch.zeros((kn.KR_SOFTDTW_MAX_LEN + 1, 3), dtype=torch.float64), 1e-2)
    for bad in (dict(gamma=0.0), dict(cost="l2")):
        with pytest.raises(ValueError):
            ke.softdtw_grad(tips[0].numpy(), ref.numpy(), **{"gamma": 1e-2, **bad})
    with pytest.raises(ValueError):
        ke.softdtw_distance(np.zeros((0, 3)), ref.numpy(), 1e-2)
