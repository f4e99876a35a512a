"""The derivative oracle (oracle/ode_derivative.py) against the reference's own autograd, on the CPU.

tests/golden/ode_deriv.npz holds the reference's fp64 autograd Jacobians of one grid point - through ``ODE_parallel``
(complete graph) and through the serial ``ODE`` (graph cut at quad(h) and Omega(u)) - on 5 parameter sets x 4 rows, and
its ``getResidualEuler`` gradients on 18 sweep cases.  Here the 50-digit derivative is held to both Jacobians block by
block (tests/ode_derivative_cases.py), which is what entitles the GPU tests to use it as THE derivative; the distances
measured here are the yardstick of their bounds."""
import numpy as np
import pytest

import ode_derivative_cases as dc
from conftest import load_golden, rel_l2

_cache = {}


def oracle_jacobians(s, cut):
    """[4, 25, 47] of a set, computed once (0.1 s per row and mode)."""
    if (s, cut) not in _cache:
        import ode_derivative as od
        J = od.jacobian_mp_batch(dc.rod_params(s).derived(), *dc.rows(), cut=cut)
        J.setflags(write=False)
        _cache[s, cut] = J
    return _cache[s, cut]


def test_fixture_holds_the_cases():
    g = load_golden("ode_deriv")
    for name, a in zip(("y", "yh", "zh", "tf"), dc.rows()):
        assert np.array_equal(g[f"rows_{name}"], a)
    y = g["rows_y"]
    assert y.shape[0] == dc.N_ROWS
    hn = np.linalg.norm(y[:, 3:7], axis=1)
    assert np.all(np.abs(hn - 1) > 0.02) and np.all((hn[2:] > 0.7) & (hn[2:] < 1.4))      # un-normalised quaternions
    q = y[2:, 13:16]
    assert np.any(q > 0) and np.any(q < 0) and np.any(q == 0.0)
    for s in dc.SETS:
        P = dc.rod_params(s)
        for f in dc.PARAM_FIELDS:
            assert np.array_equal(g[f"set_{s}_{f}"], np.asarray(getattr(P, f), np.float64)), (s, f)
    # what the sets are for: a Bse whose c0 multiple is 0.1 .. 1 of Kse's diagonal; a set with nothing diagonal or small
    D = dc.rod_params("bse_diag").derived()
    ratio = D.c0 * np.diag(D.Bse) / np.diag(D.Kse)
    assert np.all((ratio >= 0.1) & (ratio <= 1.0))
    F = dc.rod_params("full")
    for M in (F.Bse, F.Bbt):
        assert np.all(M != 0) and np.all(np.abs(M - M.T)[np.triu_indices(3, 1)] > 0.1 * np.abs(M).min())
    assert len(set(F.C)) == 3 and np.all(F.C > 0.1) and np.all(dc.rod_params("noair").C == 0)


@pytest.mark.parametrize("s", dc.SETS)
def test_reference_uncut_jacobian_vs_oracle(s):
    """ODE_parallel's fp64 autograd is another fp64 evaluation of the derivative the oracle gives to 50 digits.
    Measured over the committed rows: worst block 6.7e-15 (d(w_s)/d(uh)), every other block below 5.1e-16."""
    g = load_golden("ode_deriv")
    ref, J = g[f"J_uncut_{s}"], oracle_jacobians(s, False)
    errs = dc.assert_blocks(ref, J, dc.CPU_MARGIN * dc.REF_UNCUT_WORST, what=f"reference (uncut), set {s}")
    assert dc.zero_pattern(ref) == dc.zero_pattern(J)
    # the table the GPU bounds are made of is an upper bound of what is measured here
    for k, e in errs.items():
        if e is not None:
            assert e <= dc.REF_UNCUT_DIST[k], (k, e)


@pytest.mark.parametrize("s", dc.SETS)
def test_reference_cut_jacobian_vs_oracle(s):
    """The serial ODE's autograd against the frozen-leaf derivative.  The reference rounds the leaf it makes of quad(h)
    to fp32 there (``.float()``), so the distance - 2.06e-7 at worst, block d(q_s)/d(h) - is its rounding."""
    g = load_golden("ode_deriv")
    ref, J = g[f"J_cut_{s}"], oracle_jacobians(s, True)
    dc.assert_blocks(ref, J, dc.CPU_MARGIN * dc.REF_CUT_WORST, what=f"reference (cut), set {s}")
    assert dc.zero_pattern(ref) == dc.zero_pattern(J)


@pytest.mark.parametrize("s", dc.SETS)
def test_cut_differs_from_uncut_where_it_should(s):
    """The two graphs differ in the h columns (R sees h only through 2 / (h . h)) and in d(h_s)/d(m), d(h_s)/d(uh)
    (h_s does not see u), which the cut graph has as zero blocks - and nowhere else."""
    Ju, Jc = oracle_jacobians(s, False), oracle_jacobians(s, True)
    errs = dc.block_errors(Jc, _with_blocks_of(Ju, Jc, [(ob, "h") for ob in dc.OUT_BLOCKS] + [("h_s", "m"), ("h_s", "uh")]))
    # two correctly rounded doubles of numbers that agree to 1e-30 differ by one unit in the last place at most
    assert all(e is None or e <= 2.0 ** -52 for e in errs.values())
    zu, zc = dc.zero_pattern(Ju), dc.zero_pattern(Jc)
    for k in zu:
        if k in (("h_s", "m"), ("h_s", "uh")):
            assert zc[k] and not zu[k]
        else:
            assert zc[k] == zu[k], k
    diff = dc.block_errors(_only_h(Jc), _only_h(Ju))
    for ob in dc.OUT_BLOCKS:
        assert diff[ob, "h"] > 1e-3, ob


def _with_blocks_of(J, other, blocks):
    out = np.array(J)
    for ob, ib in blocks:
        out[:, dc.OUT_BLOCKS[ob], dc.IN_BLOCKS[ib]] = other[:, dc.OUT_BLOCKS[ob], dc.IN_BLOCKS[ib]]
    return out


def _only_h(J):
    out = np.zeros_like(J)
    out[:, :, dc.IN_BLOCKS["h"]] = J[:, :, dc.IN_BLOCKS["h"]]
    return out


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("row", [1, 3])
def test_step_convergence(row, cut):
    """The oracle's own error: steps 1e-20 and 1e-15 give the same Jacobian to 1e-25."""
    import ode_derivative as od
    y, yh, zh, tf = dc.rows()
    D = dc.rod_params("full").derived()
    assert od.step_agreement(D, y[row], yh[row], zh[row], tf[row], cut=cut) < 1e-25


def test_default_path_of_the_oracle_ode_is_untouched():
    """``leaves`` with nothing held is the same arithmetic as the default path, bit for bit."""
    import cosserat_oracle as orc
    y, yh, zh, tf = dc.rows()
    for s in dc.SETS:
        D = dc.rod_params(s).derived()
        for i in range(dc.N_ROWS):
            a = np.concatenate(orc.ode(D, y[i], yh[i], zh[i], tf[i]))
            b = np.concatenate(orc.ode(D, y[i], yh[i], zh[i], tf[i], leaves={}))
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# sweep cases: d L / d G of the function itself, from the fp64 oracle sweep
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,s,net", dc.SWEEP_CASES)
def test_sweep_gradient_of_the_oracle(N, s, net):
    """Central differences of the fp64 oracle sweep at two steps agree to 1e-8 (truncation ~ step^2, rounding ~
    1e-16 |L| / (step |dL/dG|): both far below at these steps), and the gradient of the FUNCTION is not the gradient of
    the reference's cut graph: the two modes of the adjoint sweep can be told apart on every case."""
    g = load_golden("ode_deriv")
    dG, agree, L = dc.oracle_sweep_dG(g, N, s, net)
    tag = dc.sweep_tag(N, s, net)
    assert agree < 1e-8
    assert rel_l2(dG, g[f"{tag}_dG"]) > 1e-3
    # same sweep, same loss: the value (fp32 in the reference) at the bound test_torch_full_sweep_autograd holds L to
    assert abs(L - float(g[f"{tag}_L"])) < 2e-5 * abs(float(g[f"{tag}_L"]))


@pytest.mark.parametrize("N,s,net", [(10, "full", "hist64"), (33, "None", "elu64")])
def test_weight_differences_of_the_oracle_sweep(N, s, net):
    """The step of ``oracle_sweep_dparams`` against one ten times smaller (ten times the rounding floor, a hundredth of
    the truncation): the sampled parameter gradients agree two orders below the 1e-3 they are used at."""
    g = load_golden("ode_deriv")
    a = dc.oracle_sweep_dparams(g, N, s, net, n_samples=6)
    b = dc.oracle_sweep_dparams(g, N, s, net, n_samples=6, step=dc.W_STEP / 10)
    for (k, ia, va), (_, ib, vb) in zip(a, b):
        assert np.array_equal(ia, ib) and rel_l2(va, vb) < 1e-5, k
