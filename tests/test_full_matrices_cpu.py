"""CPU side of the full-material-matrix tests (tests/full_matrix_cases.py; the GPU side is
tests/test_gpu_full_matrices.py):

(a) both oracles against the unmodified reference on "full-asym" (tests/golden/full_matrices.npz), block by block;
(b) the test of the tests: on every case the GPU file runs, the oracle's own answer under each of the four mutants
    (``Bse`` / ``Bbt`` transposed or stripped of its off-diagonals) must miss a quantity the GPU test compares by at least
    ten times the tolerance the GPU test applies to it - a kernel that computed a mutant would fail there.  Under the fp32
    bounds this holds for ``Bbt`` and, with the network off, provably NOT for ``Bse``, whose mutants stay below the fp32
    state bound: fp32 runs hold ``Bbt`` only.  Measured margins: LABBOOK.md (full material matrices);
(c) what clears ``RodConst::diag`` (fill_consts, kr_api.hip), as far as the host shows it: the derived inverses of
    "full-asym" have off-diagonal entries and equal the oracle's entry by entry (an inverse transposed on the way would
    not), the twin's are diagonal.  Which kernel then runs is asserted on the GPU side, call by call."""
import numpy as np
import pytest

import full_matrix_cases as fm

# the bounds of test_oracle_golden.py::test_c_oracle_long_runs_vs_reference (tips 1e-9, states 1e-8), the states per block.
# Measured worst: tips 1.9e-11, a block 1.9e-10 (u at N = 100 / 400).
TIP_TOL, BLOCK_TOL = 1e-9, 1e-8


def _against_fixture(N, T, kind, tips, states):
    f = fm.fixture_run(N, kind)
    assert f["T"] == T and np.array_equal(f["ctl"], fm.controls(T, kind))
    entries = sorted(f["states"])
    te = fm.tip_error(tips[0, :T], f["tips"])   # (the reference drops its last solve: entries 0 .. T - 1)
    be = fm.block_errors(states[0][entries], np.array([f["states"][e] for e in entries]))
    print(f"N={N} {kind}: tips {te:.1e} | {fm.fmt_blocks(be)}")
    assert te < TIP_TOL, te
    assert all(e < BLOCK_TOL for e in be.values()), be


@pytest.mark.parametrize("N,T,kind", fm.FIXTURE_RUNS)
def test_c_oracle_vs_reference(N, T, kind):
    _against_fixture(N, T, kind, *fm.oracle_run(N, T, kind))


@pytest.mark.parametrize("N,T,kind", [r for r in fm.FIXTURE_RUNS if r[0] <= 100])
def test_numpy_oracle_vs_reference(N, T, kind):
    """``solver="newton"``; N = 400 is left to the C oracle (the NumPy sweep of 400 points takes a minute)."""
    _against_fixture(N, T, kind, *fm.numpy_oracle_run(N, T, kind))


def test_fixture_is_the_parameter_set():
    from conftest import load_golden
    g = load_golden("full_matrices")
    Bse, Bbt = fm.matrices("full-asym")
    assert np.array_equal(g["Bse"], Bse) and np.array_equal(g["Bbt"], Bbt)
    for M in (Bse, Bbt):  # nothing symmetric: every off-diagonal pair differs
        assert all(M[i, j] != M[j, i] for i in range(3) for j in range(i))
    for N, T, kind in fm.FIXTURE_RUNS:
        assert fm.fixture_run(N, kind)["T"] == T


def _mutant_misses(run, N, T, kind, mutant, **kw):
    """(error / tolerance) of the mutant's answer against the set's own, fp64 and fp32 bounds, over all entries 1 .. T
    (what a "full" call compares) and on entry T alone (what a ring leaves to compare); and its largest block distance."""
    tips, st = run(N, T, kind, "full-asym", **kw)
    tm, sm = run(N, T, kind, mutant, **kw)
    te = fm.tip_error(tm[0, 1:], tips[0, 1:])
    be_all, be_last = fm.block_errors(sm[0, 1:], st[0, 1:]), fm.block_errors(sm[0, T], st[0, T])
    out = {(d, w): fm.misses(te, be, d) for d in ("f64", "f32") for w, be in (("all", be_all), ("last", be_last))}
    print(f"N={N} T={T} {kind} {mutant}: tips {te:.1e} | {fm.fmt_blocks(be_all)} | x tol " +
          " ".join(f"{d}/{w}:{v:.3g}" for (d, w), v in out.items()))
    return out, max(max(be_all.values()), max(be_last.values()))


@pytest.mark.parametrize("N,T,kind", fm.SIM_CASES)
def test_mutants_are_seen(N, T, kind):
    for m in fm.MUTANTS:
        miss, worst_block = _mutant_misses(fm.oracle_run, N, T, kind, m)
        assert miss["f64", "all"] >= fm.MARGIN and miss["f64", "last"] >= fm.MARGIN, (m, miss)
        if m in fm.BBT_MUTANTS:
            assert miss["f32", "all"] >= fm.MARGIN and miss["f32", "last"] >= fm.MARGIN, (m, miss)
        else:  # the limitation, in code: an fp32 run cannot tell a wrong Bse branch from a right one
            assert worst_block < fm.TOL["f32"][1], (m, worst_block)
            assert miss["f32", "all"] < 1.0 and miss["f32", "last"] < 1.0, (m, miss)


@pytest.mark.parametrize("net", fm.NN_NETS)
def test_mutants_are_seen_with_the_network_on(net):
    """The NumPy oracle with the network in every sweep.  The networks of sim_nn.npz read q and w and answer in every
    row, so here a wrong ``Bse`` is carried further: its mutants are visible under the fp32 bounds, too (measured 46 to
    220 times the bound), which is asserted, not assumed."""
    N, T, kind = fm.NN_CASE
    for m in fm.MUTANTS:
        miss, _ = _mutant_misses(fm.numpy_oracle_run, N, T, kind, m, net=net)
        assert min(miss.values()) >= fm.MARGIN, (m, miss)


def test_mutants_are_seen_in_one_step():
    """kr_step_batch's case: one step from entries 7, 8 of the N = 40 run; only the state it writes is compared."""
    nxt = fm.step_case()[3]
    for m in fm.MUTANTS:
        be = fm.block_errors(fm.step_case(m)[3][0], nxt[0])
        print(f"step {m}: {fm.fmt_blocks(be)}")
        assert max(be.values()) >= fm.MARGIN * fm.TOL["f64"][1], (m, be)
        if m in fm.BBT_MUTANTS:
            assert max(be.values()) >= fm.MARGIN * fm.TOL["f32"][1], (m, be)
        else:
            assert max(be.values()) < fm.TOL["f32"][1], (m, be)
    # the step oracle and the C oracle's time loop agree on the state after it
    _, st = fm.oracle_run(*fm.STEP_CASE[:3])
    assert max(fm.block_errors(nxt[0], st[0, fm.STEP_CASE[3] + 1]).values()) < 1e-11


def test_twin_is_another_problem():
    """The control runs the diagonal twin: a different rod (tips 4e-2 .. 7e-2 away), so a kernel that ignored the
    off-diagonals would not pass the full-matrix comparison by computing the twin."""
    for N, T, kind in fm.SIM_CASES:
        tips, _ = fm.oracle_run(N, T, kind)
        twin, _ = fm.oracle_run(N, T, kind, "twin")
        assert fm.tip_error(twin[0, 1:], tips[0, 1:]) > 1e-2


def test_what_clears_the_diag_flag():
    import cosserat_oracle as orc
    import krod_native as kn
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    off = lambda M: np.abs(M - np.diag(np.diag(M))).max()
    for variant in fm.VARIANTS:
        r = CosseratRod(use_fsolve=True)
        setup_robot(r, None)
        r.N = 40
        fm.apply_to_rod(r, variant)
        P = fm.rod_params(40, variant)
        D = P.derived()
        p = r._params()
        assert np.array_equal(np.array(p.Bse).reshape(3, 3), P.Bse) and np.array_equal(np.array(p.Bbt).reshape(3, 3), P.Bbt)
        assert p.del_t == fm.DEL_T == P.del_t
        d = kn.derive(p)
        Ksei, Kbti = (np.array(a).reshape(3, 3) for a in (d.Kse_plus_c0_Bse_inv, d.Kbt_plus_c0_Bbt_inv))
        # entry by entry against the oracle's inverse, on the scale of the matrix: a transposed inverse is 1e-1 off
        assert np.abs(Ksei - D.Kse_inv).max() < 1e-13 * np.abs(D.Kse_inv).max()
        assert np.abs(Kbti - D.Kbt_inv).max() < 1e-13 * np.abs(D.Kbt_inv).max()
        assert np.array_equal(r.Kse_plus_c0_Bse_inv, Ksei) and np.array_equal(r.Kbt_plus_c0_Bbt_inv, Kbti)
        if variant == "twin":
            assert off(Ksei) == 0.0 and off(Kbti) == 0.0 and off(P.Bse) == 0.0 and off(P.Bbt) == 0.0
        else:  # either matrix alone clears the flag
            assert off(Ksei) > 0.0 or off(P.Bse) > 0.0 or off(Kbti) > 0.0 or off(P.Bbt) > 0.0
        if variant == "full-asym":
            assert off(Ksei) > 1e-2 * np.abs(np.diag(Ksei)).min() and off(Kbti) > 1e-2 * np.abs(np.diag(Kbti)).min()
            assert np.abs(Ksei - Ksei.T).max() > 1e-2 * np.abs(np.diag(Ksei)).min()
