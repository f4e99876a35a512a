"""CPU side of the RK4-sweep tests (tests/rk4_cases.py; the GPU side is tests/test_gpu_rk4_sweeps.py):

(a) the C oracle's RK4 sweep against the NumPy oracle's, on both parameter sets;
(b) both oracles against every run of the unmodified reference under RK4 (tests/golden/rk4_sweeps.npz), block by block;
(c) the test of the tests: the oracle's own answer under each of the seven mutants of the sweep (rk4_cases.MUTANTS) must
    miss a quantity the GPU test compares by at least ten times the tolerance the GPU test applies to it.  In fp64 that
    holds for every mutant at N = 9 and N = 40; under the fp32 bounds for every mutant at N = 9 - the shape at which an
    fp32 run holds the whole scheme - and at N = 40 for the mutants of the histories and of the stored ``v``, ``u`` only:
    a wrong stage 3 and wrong weights are O(ds^2) and smaller, BELOW ten fp32 bounds on a fine grid, which is asserted
    too.  An fp32 run at N >= 40 does not hold them;
(d) RK4 and Euler answers are more than ten fp32 tip bounds apart at every N <= 131 of the cases: a kernel that ignores
    ``scheme`` passes in neither type;
(e) the None preset under RK4 at N = 9 is not solved by the reference - why no case here uses it on a coarse grid.
Measured figures: LABBOOK.md (RK4 sweeps)."""
import numpy as np
import pytest

import full_matrix_cases as fm
import rk4_cases as rk
from conftest import load_golden

# The bounds of test_oracle_golden.py::test_c_oracle_long_runs_vs_reference (tips 1e-9, states 1e-8), the states per block,
# as test_full_matrices_cpu.py holds both oracles to under Euler.  Measured worst: (a) C against NumPy oracle tips 5.2e-16, a
# block 6.0e-15 (q at N = 40); (b) either oracle against the reference tips 8.4e-12, a block 1.8e-10 (u at N = 400).
TIP_TOL, BLOCK_TOL = 1e-9, 1e-8
MUTANT_T = {9: 16, 40: 6}  # steps of the mutant runs (the NumPy oracle: 28 sweeps of 4 (N - 1) ode calls per step)


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("N,T", [(9, 16), (12, 8), (40, 4)])
def test_c_oracle_vs_numpy_oracle(N, T, variant):
    tips, st = rk.oracle_run(N, T, "sine", variant)
    tn, sn = rk.numpy_oracle_run(N, T, "sine", variant)
    te, be = fm.tip_error(tips[0, 1:], tn[0, 1:]), fm.block_errors(st[0, 1:], sn[0, 1:])
    print(f"N={N} T={T} {variant}: tips {te:.1e} | {fm.fmt_blocks(be)}")
    assert te < TIP_TOL and all(e < BLOCK_TOL for e in be.values()), (te, be)


def _against_fixture(variant, N, T, kind, tips, states):
    f = rk.fixture_run(N, kind, variant)
    assert f["T"] == T and np.array_equal(f["ctl"], fm.controls(T, kind))
    entries = sorted(f["states"])
    te = fm.tip_error(tips[0, :T], f["tips"])   # (the reference drops its last solve: entries 0 .. T - 1)
    be = fm.block_errors(states[0][entries], np.array([f["states"][e] for e in entries]))
    print(f"{variant} N={N} {kind}: tips {te:.1e} | {fm.fmt_blocks(be)}")
    assert te < TIP_TOL, te
    assert all(e < BLOCK_TOL for e in be.values()), be


@pytest.mark.parametrize("variant,N,T,kind", rk.FIXTURE_RUNS)
def test_c_oracle_vs_reference(variant, N, T, kind):
    _against_fixture(variant, N, T, kind, *rk.oracle_run(N, T, kind, variant))


@pytest.mark.parametrize("variant,N,T,kind", [r for r in rk.FIXTURE_RUNS if r[1] <= 40])
def test_numpy_oracle_vs_reference(variant, N, T, kind):
    """``solver="newton"``; N = 100 and 400 are left to the C oracle, which agrees with this one to 1e-14 (above): an RK4
    sweep of the NumPy oracle over 400 points takes half a minute."""
    _against_fixture(variant, N, T, kind, *rk.numpy_oracle_run(N, T, kind, variant))


def test_fixture_is_the_parameter_set():
    g = load_golden("rk4_sweeps")
    Bse, Bbt = fm.matrices("full-asym")
    assert np.array_equal(g["Bse"], Bse) and np.array_equal(g["Bbt"], Bbt)
    for variant, N, T, kind in rk.FIXTURE_RUNS:
        assert rk.fixture_run(N, kind, variant)["T"] == T
        assert (N, T, kind) in rk.SIM_CASES


def test_preset_is_not_solved_on_a_coarse_grid():
    """The None preset under RK4 at N = 9: the reference's fsolve gives up (``ier != 1``) from step 2 on and its tips end
    as NaN.  The cases use "full-asym" and its twin instead, on every grid."""
    g = load_golden("rk4_sweeps")
    N, T, kind = rk.PRESET_RUN
    ier, tips = g["preset_n9_sine_ier"], g["preset_n9_sine_tips"]
    assert np.array_equal(g["preset_n9_sine_ctl"], fm.controls(T, kind)) and ier.shape == (T,)
    assert ier[0] == 1 and np.all(ier[1:] != 1), ier
    assert not np.all(np.isfinite(tips)), "the preset's run stayed finite: has the fixture been regenerated?"
    assert N < 27 and all(v in ("full-asym", "twin") for v in rk.VARIANTS)


def test_the_mutant_sweep_with_nothing_wrong_is_the_sweep():
    tn, sn = rk.numpy_oracle_run(9, 16, "sine", "full-asym")
    tm, sm = rk.mutant_run(9, 16, "sine", "full-asym", None)
    assert np.array_equal(tn, tm) and np.array_equal(sn, sm)


def _mutant_misses(N, T, variant, mutant):
    """(error / tolerance) of the mutant's answer against the true RK4 answer, fp64 and fp32 bounds, over all entries
    1 .. T (what a "full" call compares) and on entry T alone (what a ring leaves to compare)."""
    tips, st = rk.oracle_run(N, T, "sine", variant)
    tm, sm = rk.mutant_run(N, T, "sine", variant, mutant)
    te = fm.tip_error(tm[0, 1:], tips[0, 1:])
    be_all, be_last = fm.block_errors(sm[0, 1:], st[0, 1:]), fm.block_errors(sm[0, T], st[0, T])
    out = {(d, w): fm.misses(te, be, d) for d in ("f64", "f32") for w, be in (("all", be_all), ("last", be_last))}
    worst = max(be_all, key=be_all.get)
    print(f"N={N} T={T} {variant} {mutant}: tips {te:.1e} / worst block {worst} {be_all[worst]:.1e} | x tol " +
          " ".join(f"{d}/{w}:{v:.3g}" for (d, w), v in out.items()))
    return out


@pytest.mark.parametrize("variant", rk.VARIANTS)
@pytest.mark.parametrize("N", sorted(MUTANT_T))
def test_mutants_are_seen(N, variant):
    T = MUTANT_T[N]
    for m in rk.MUTANTS:
        miss = _mutant_misses(N, T, variant, m)
        assert miss["f64", "all"] >= fm.MARGIN and miss["f64", "last"] >= fm.MARGIN, (m, miss)
        if N == 9 or m in rk.HISTORY_MUTANTS:
            assert miss["f32", "all"] >= fm.MARGIN and miss["f32", "last"] >= fm.MARGIN, (m, miss)
        else:  # the limitation, in code: an fp32 run on a fine grid does not hold stage 3 or the weights
            assert m in rk.FINE_MUTANTS
            assert miss["f32", "all"] < fm.MARGIN and miss["f32", "last"] < fm.MARGIN, (m, miss)


@pytest.mark.parametrize("variant", rk.VARIANTS)
def test_rk4_is_not_euler(variant):
    """A kernel that ignored ``scheme`` would return the Euler answer: more than ten fp32 tip bounds (hence 10^4 fp64
    ones) from the RK4 answer at every N of the cases up to 131."""
    for N, T, kind in rk.SIM_CASES:
        if N > 131:
            continue
        tips, _ = rk.oracle_run(N, T, kind, variant)
        euler, _ = rk.oracle_run(N, T, kind, variant, scheme="euler")
        te = fm.tip_error(euler[0, 1:], tips[0, 1:])
        print(f"N={N} T={T} {kind} {variant}: Euler tips {te:.1e} from RK4's")
        assert te > fm.MARGIN * fm.TOL["f32"][0], (N, te)


def test_one_step_case_is_the_runs_own():
    """kr_step_batch's case is three consecutive entries of one oracle run, and the step between them moves the state by
    far more than a bound (so that returning ``cur`` is no answer)."""
    for variant in rk.VARIANTS:
        prev, cur, tens, nxt = rk.step_case(variant, 2)
        _, st = rk.oracle_run(*rk.STEP_CASE[:3], variant, 2)
        e = rk.STEP_CASE[3]
        assert np.array_equal(nxt, st[:, e + 1]) and np.array_equal(cur, st[:, e]) and np.array_equal(prev, st[:, e - 1])
        be = fm.block_errors(cur[0], nxt[0])
        print(f"{variant}: entry 8 against entry 9: {fm.fmt_blocks(be)}")
        # (v, the stretch of a rod stiff in extension, moves by 7e-6 in a step: above the fp64 bound only)
        assert min(be.values()) > fm.MARGIN * fm.TOL["f64"][1]
        assert min(e for k, e in be.items() if k != "v") > fm.MARGIN * fm.TOL["f32"][1]
