"""CPU side of the sweep-count tests with the MLP off (tests/sweep_count_cases.py; the GPU side is
tests/test_gpu_sweep_counts.py) - the test of the tests:

(a) the fixture tests/golden/sweep_counts.npz is what ``mlp_shape_cases.newton_steps`` computes: small cells recomputed;
(b) a mutant alters ``fun_fd`` or the start only, so it keeps the root: every converged mutant run of the fixture ended within
    ``ROOT_TOL`` of the exact run, the exact runs converged at every step, and the recomputed cells show the same;
(c) for every row of the GPU file, with the family's measured slack: every mutant DECLARED HELD exceeds the bound
    S_exact + slack + (S_held_min - S_exact) / 3 on every rod - the row fails on a kernel that needs the mutant's count,
    whichever rod one looks at - and every mutant NOT held is at or below the bound on some rod: the row cannot be relied on
    to see it.  A row without a held mutant is not a GPU row and is listed ("Not held");
(d) what the figures were expected to show (the issue's table): "no-history" and "no-c2" are held by every family on every
    Jacobian row, and "hist-j+1" under "damping" at the fp32 rule costs the oracle not one sweep - no row holds it there;
(e) the start rules: rule -1 is rule 2 in a loop that hands over every state, rule 1 / 2 differ from the warm start only from
    step 1 / 2 on, and the counts of the oracle do not depend on which extrapolation formula is written down.
Measured figures: LABBOOK.md (Sweep counts with the MLP off)."""
import numpy as np
import pytest

import sweep_count_cases as cc

RECOMPUTED_JAC = [("euler", "damping", 9, "f32"), ("euler", "preset", 9, "f64"), ("rk4", "twin", 9, "f64")]
RECOMPUTED_START = [("euler", "preset", 9)]


@pytest.mark.parametrize("scheme,pset,N,dtype", RECOMPUTED_JAC)
def test_fixture_is_the_oracles_count_jacobian(scheme, pset, N, dtype):
    it, dev = cc.jac_counts(scheme, pset, N, dtype)
    b = 1
    exact = cc.run(pset, scheme, N, b, dtype)
    assert all(exact["ok"]) and np.array_equal(exact["iters"], it[None][b])
    for m in cc.JAC_MUTANTS[scheme]:
        with np.errstate(all="ignore"):
            r = cc.run(pset, scheme, N, b, dtype, "jac", m)
        d = cc.root_deviation(r, exact)
        print(f"{scheme} {pset} N={N} {dtype} rod {b} {m}: {list(r['iters'])} = {sum(r['iters'])}, root deviation {d:.1e}")
        assert np.array_equal(r["iters"], it[m][b]), m
        assert d == dev[m][b] or (np.isinf(d) and np.isinf(dev[m][b])), (m, d, dev[m][b])
        assert np.isinf(d) or d <= cc.ROOT_TOL[dtype], (m, d)


@pytest.mark.parametrize("scheme,pset,N", RECOMPUTED_START)
def test_fixture_is_the_oracles_count_start(scheme, pset, N):
    it, dev = cc.start_counts(scheme, pset, N)
    b = 2
    spec = {"rule0": (0, None), "rule1": (1, None), "rule2": (2, None), "sign1": (1, "sign"), "sign2": (2, "sign"), "zero": (2, "zero")}
    exact = cc.run(pset, scheme, N, b, "f64", "start", None, 0)
    for row, (rule, mutant) in spec.items():
        r = cc.run(pset, scheme, N, b, "f64", "start", mutant, rule)
        d = cc.root_deviation(r, exact)
        print(f"{scheme} {pset} N={N} rod {b} {row}: {list(r['iters'])} = {sum(r['iters'])}, root deviation {d:.1e}")
        assert all(r["ok"]) and np.array_equal(r["iters"], it[row][b]), row
        assert d <= cc.ROOT_TOL["f64"] and d == dev[row][b], (row, d)
    # rule -1 = rule 2, "order0" = rule 0: by construction of the loop, shown once
    for rule, mutant, same in ((-1, None, "rule2"), (2, "order0", "rule0"), (1, "order0", "rule0"), (1, "zero", "zero")):
        r = cc.run(pset, scheme, N, b, "f64", "start", mutant, rule)
        assert np.array_equal(r["iters"], it[same][b]), (rule, mutant)


def test_every_run_of_the_fixture_kept_the_root():
    for cell in cc.jac_cells():
        it, dev = cc.jac_counts(*cell)
        assert np.all(dev[None] == 0.0) and np.all(it[None] >= 1) and np.all(it[None] < cc.MAXIT), cell
        for m in cc.JAC_MUTANTS[cell[0]]:
            ok = np.isfinite(dev[m])
            assert np.all(dev[m][ok] <= cc.ROOT_TOL[cell[3]]), (cell, m, dev[m])
            # a run that did not converge somewhere is counted at the cap there: far above any bound
            assert np.all(it[m][~ok].max(axis=1) == cc.MAXIT), (cell, m)
    for cell in cc.start_cells():
        it, dev = cc.start_counts(*cell)
        for row in cc.START_ROWS:
            assert np.all(np.isfinite(dev[row])) and np.all(dev[row] <= cc.ROOT_TOL["f64"]), (cell, row, dev[row])
            assert np.all(it[row] >= 1) and np.all(it[row] < cc.MAXIT), (cell, row)
        for b in range(cc.B):  # the rules agree until they have the states to differ
            assert np.array_equal(it["rule1"][b][:1], it["rule0"][b][:1]) and np.array_equal(it["rule2"][b][:2], it["rule1"][b][:2])


def _check_row(label, row):
    """(c) of the module docstring for one row; returns whether it is a GPU row."""
    if row["bound"] is None:
        assert not row["held"]
        return False
    assert row["held"] and row["slack"] is not None
    for b in range(cc.B):
        for m in row["held"]:
            assert row["s_mut"][m][b] > row["bound"][b], (label, m, b, row["s_mut"][m][b], row["bound"][b])
        assert row["s_exact"][b] + row["slack"] <= row["bound"][b], label   # (what the family was measured to need passes)
    for m in row["not_held"]:
        assert any(row["s_mut"][m][b] <= row["bound"][b] for b in range(cc.B)), (label, m, row["s_mut"][m], row["bound"])
    return True


def test_what_each_jacobian_row_holds():
    dropped, held_sets = [], {}
    for r in cc.jac_rows():
        family, scheme, pset, N, dtype = r
        assert 0 <= cc.slack_of(family, dtype) <= cc.T_JAC, (family, dtype)
        row = cc.jac_row(*r)
        if not _check_row(r, row):
            dropped.append(r)
            continue
        held_sets.setdefault((family, dtype, row["held"]), []).append((scheme, pset, N))
        # (d): what every family holds
        assert "no-history" in row["held"] and "no-c2" in row["held"], (r, row["held"])
        if scheme == "euler" and pset == "damping" and dtype == "f32":
            assert "hist-j+1" in row["not_held"], r
            # (24 against 24 on most rods, never more than one sweep apart: invisible under this rule)
            assert np.all(row["s_mut"]["hist-j+1"] - row["s_exact"] <= 1) and np.any(row["s_mut"]["hist-j+1"] == row["s_exact"])
    for (family, dtype, held), cells in sorted(held_sets.items()):
        print(f"{family} {dtype} holds {held} on {cells}")
    print(f"dropped rows (no held mutant): {dropped}")
    assert not dropped, dropped  # (every Jacobian row holds the two history mutants at least)


def test_what_each_start_row_holds():
    dropped, rows = [], 0
    for r in cc.start_rows():
        assert 0 <= cc.slack_of(r[0], r[4], "start") <= cc.T_START
        row = cc.start_row(*r)
        if _check_row(r, row):
            rows += 1
            print(f"{r}: exact {row['s_exact'].tolist()} mutants { {m: s.tolist() for m, s in row['s_mut'].items()} } holds {row['held']}")
        else:
            dropped.append(r)
    print(f"start rows kept {rows}, dropped (no held mutant, DESIGN.md section 2): {dropped}")
    # K2a holds the sign and G = 0 under ``predictor = 1`` (slack 0) on every cell; with a quadratic start either family needs
    # 11 - 12 sweeps over the oracle's 16-step sum, which leaves G = 0 on "full-asym" alone
    assert all(("K2a", s, p, N, 1) not in dropped for s in ("euler", "rk4") for p in cc.PSETS_OF[s] for N in cc.FAMILIES["K2a"][2])
    assert all(r[0] == "K2b" or r[4] != 1 for r in dropped)
    assert rows == 20 and len(dropped) == len(cc.start_rows()) - 20
