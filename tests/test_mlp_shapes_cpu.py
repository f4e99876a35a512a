"""The reference side of tests/test_gpu_mlp_shapes.py, checked without a GPU (tests/mlp_shape_cases.py holds the cases):

* every parity and count reference converges on the oracle (``ier == 1`` on every step), and a parity network moves its
  rod by orders more than any tolerance of the GPU tests;
* the sweep counts separate a working network Jacobian from a dead one far enough for the bound of the GPU count test to
  lie between them: no count case backtracks or takes more than 6 exact iterations in a step; S_frozen >= 2.5 S_full at
  the fp64 stopping rule, >= 1.75 S_full at the fp32 one; bound <= S_frozen - T on every rod;
* the host shape rules (``kr_mlp_bank_check``, tests/gpu_helpers.py) serve every parity shape and refuse the first shape
  beyond each limit with a message that names it."""
import os
import sys

import numpy as np
import pytest

import mlp_shape_cases as sc
from conftest import ROOT
from gpu_helpers import expected_path, mlp_on_matrix_cores


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    return kn


def preset_params(N):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r, None)
    r.N = N
    r.compute_intermediate_terms()
    return r._params()


@pytest.mark.parametrize("cid", sc.PARITY_IDS)
def test_parity_references_converge_and_the_network_matters(cid):
    """``ier == 1`` on every step is asserted where a reference is computed (mlp_shape_cases._tight)."""
    for N in (20, 40) if cid in sc.W2_IDS else (20,):
        refs = sc.parity_case(cid, N)
        assert len(refs) == sc.B and all(r.shape == (sc.T_PARITY + 1, 25, N) for r in refs)
        for b, ref in enumerate(refs[:1] if N == 40 else refs):
            plain = sc.plain_rod(N, b)
            d = np.linalg.norm(ref - plain) / np.linalg.norm(plain)
            d_tip = np.linalg.norm(ref[:, :3, -1] - plain[:, :3, -1]) / np.linalg.norm(plain[:, :3, -1])
            print(f"case {cid}, N = {N}, rod {b}: trajectory {d:.3e}, tip path {d_tip:.3e} relative from the MLP-off run; "
                  f"nfev per step {sc.parity_rod(cid, N, b)[1]}")
            assert d > 5e-2 and d_tip > 1e-3  # (tolerances of the GPU tests: 1e-8 and 1e-5)


@pytest.mark.parametrize("cid", sc.BANK_IDS)
def test_bank_references_converge(cid):
    refs = sc.bank_case(cid)
    assert len(refs) == sc.B and all(r.shape == (sc.T_PARITY + 1, 25, 20) for r in refs)
    # network BANK_NETS[0] on the plain preset is not the case's own network (seed 7) on it
    own = sc.parity_rod(cid, 20, 0)[0]
    assert sc.BANK_SEEDS[sc.BANK_NETS[0]] != sc.NET_SEED and sc.BANK_MODS[0] is None
    d_tip = np.linalg.norm(own[:, :3, -1] - refs[0][:, :3, -1]) / np.linalg.norm(refs[0][:, :3, -1])
    print(f"case {cid}, rod 0: two networks of the bank move the tip path by {d_tip:.3e} relative")
    assert d_tip > 1e-4


def test_the_count_cases_that_must_remain_are_there():
    for dtype in ("f64", "f32"):
        ids = sc.COUNT_OF[dtype]
        assert set(ids) <= set(sc.COUNT_IDS)
        assert "c3_64_64" in ids  # the one-chunk three-layer case
        assert any(len(sc.COUNT[c][0]) == 3 and sc.COUNT[c][0][1] > 64 for c in ids)  # a two-layer multi-chunk case
    for cid in sc.COUNT_IDS:
        sizes, act, gain = sc.COUNT[cid]
        assert 0.4 <= gain <= 0.6, "above 0.6 the oracle backtracks"
        mlp = sc.count_mlp(cid)
        assert sc.layer_widths(mlp) == list(sizes) and all(w.dtype == np.float32 for w in mlp.weights)
        assert not np.any(mlp.weights[0][:, :3]) and np.all(np.any(mlp.weights[0][:, 3:] != 0, axis=0))


@pytest.mark.parametrize("dtype,cid", [(d, c) for d in ("f64", "f32") for c in sc.COUNT_OF[d]])
def test_count_references_separate_a_dead_jacobian(dtype, cid):
    T = sc.T_COUNT
    for b in range(sc.B):
        full, frozen = sc.sweep_counts(cid, b, dtype, False), sc.sweep_counts(cid, b, dtype, True)
        s_full, s_frozen = sc.count_sums(cid, b, dtype)
        bound = sc.count_bound(cid, b, dtype)
        print(f"{cid} {dtype} rod {b}: exact {full['iters']} = {s_full}, frozen {frozen['iters']} = {s_frozen}, "
              f"bound {bound:.2f}")
        assert all(full["ok"]) and all(frozen["ok"]), "ier != 1"
        assert all(n == it + 1 for n, it in zip(full["base"], full["iters"])), f"the exact Newton backtracks: {full}"
        assert max(full["iters"]) <= 6
        assert s_frozen >= sc.RULE[dtype]["ratio"] * s_full
        assert bound <= s_frozen - T
    if dtype == "f64":
        refs = [sc.count_ref(cid, b) for b in range(sc.B)]  # (asserts ier == 1)
        assert all(r.shape == (T + 1, 25, 20) for r in refs)


def test_frozen_counts_reach_the_same_root():
    """The frozen Newton changes the Jacobian only: its accepted unknowns are the exact Newton's to the stopping rule."""
    import cosserat_oracle as orc
    cid, b = "c3_64_64", 0
    D = orc.setup_params(None, 20).derived()
    ref = sc.count_ref(cid, b)
    for frozen in (False, True):
        # re-run the last step of the tight trajectory from its own history with either Jacobian
        import copy
        mlp = copy.copy(sc.count_mlp(cid))
        tap = sc._Frozen(orc) if frozen else None
        mlp.tap = tap
        T = sc.T_COUNT
        y, z = ref[T - 1][:19].copy(), ref[T - 1][19:].copy()
        yp, zp = ref[T - 2][:19], ref[T - 2][19:]
        yh, zh = D.c1 * y + D.c2 * yp, D.c1 * z + D.c2 * zp
        tens = sc.controls(T)[b][T - 1]

        def base(g):
            if tap is not None:
                tap.start(False)
            return orc.residual_euler(D, g, y, z, yh, zh, tens, mlp)

        def perturbed(g):
            if tap is not None:
                tap.start(True)
            return orc.residual_euler(D, g, y, z, yh, zh, tens, mlp)

        G0 = np.concatenate([ref[T - 1][7:10, 0], ref[T - 1][10:13, 0]])
        G, ok, it = orc.newton_shoot(base, G0, tol=1e-8, fd_eps=1e-7, fun_fd=perturbed)
        assert ok
        got = np.vstack([y, z])
        err = np.linalg.norm(got[:, :-1] - ref[T][:, :-1]) / np.linalg.norm(ref[T][:, :-1])
        print(f"frozen = {frozen}: {it} iterations, state {err:.3e} relative from the tight reference")
        assert err < 1e-7


def test_host_shape_rules_serve_every_parity_shape(kn):
    for N in (20, 40):
        base = preset_params(N)
        for cid in sc.PARITY_IDS:
            mlp = sc.parity_mlp(cid)
            dims = sc.layer_widths(mlp)
            assert dims == list(sc.PARITY[cid][0])
            assert kn.mlp_bank_check(base, 3, dims, mlp.acts) == (0, ""), (cid, N)
            assert mlp_on_matrix_cores(mlp)
            assert [expected_path(m, N, mlp) for m in ("single", "multi", "persistent", "overlap")] == [0, 1, 2, 2], cid
    for cid in sc.COUNT_IDS:
        mlp = sc.count_mlp(cid)
        assert kn.mlp_bank_check(preset_params(20), 3, sc.layer_widths(mlp), mlp.acts) == (0, "")
        assert [expected_path(m, 20, mlp) for m in ("single", "multi")] == [0, 1]


def test_host_shape_rules_refuse_the_first_shape_beyond_each_limit(kn):
    import cosserat_oracle as orc
    base = preset_params(20)
    ELU, NONE = orc.ACT_ELU, orc.ACT_NONE
    assert sc.REFUSED == ((28, 64, 193, 25), (28, 65, 64, 25))
    rc, msg = kn.mlp_bank_check(base, 3, list(sc.REFUSED[0]), [ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "second hidden layer" in msg and "193" in msg, msg
    rc, msg = kn.mlp_bank_check(base, 3, list(sc.REFUSED[1]), [ELU, ELU, NONE])
    assert rc == kn.KR_E_UNSUPPORTED and "first hidden layer" in msg and "65" in msg, msg
    wide2 = orc.make_mlp(list(sc.REFUSED[0]), "elu", seed=1)
    assert mlp_on_matrix_cores(wide2) and expected_path("persistent", 20, wide2) == 1  # (one launch per step serves it)
    wide1 = orc.make_mlp(list(sc.REFUSED[1]), "elu", seed=1)
    assert not mlp_on_matrix_cores(wide1) and expected_path("persistent", 20, wide1) == 0
