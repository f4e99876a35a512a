"""Shared by tests/test_sweep_counts_cpu.py and tests/test_gpu_sweep_counts.py (not a test module): the number of Newton
sweeps a step needs with the MLP OFF, by the oracle's Newton (``mlp_shape_cases.newton_steps``: ``orc.newton_shoot`` in the
BDF2 loop) with the exact forward-difference Jacobian and start rule, and with one thing wrong in either.

A step kernel finds the same root whatever its Jacobian columns and its start values are (DESIGN.md sections 2 and 6): a
wrong column, a perturbed sweep that reads the wrong history, a time extrapolation that is not applied leave every
trajectory and every ``status`` as they are.  Only the sweep COUNT moves.  So the kernels' ``iters`` are held to

    bound = S_exact + slack + (S_held_min - S_exact) / 3            (per rod, summed over the steps of the case)

the form of ``mlp_shape_cases.count_bound``: S_exact the oracle's sum, S_held_min the smallest sum among the mutants DECLARED
HELD for that cell (``held`` below - data, decided by the figures, checked by tests/test_sweep_counts_cpu.py), ``slack`` what
the kernel family needs over the oracle (``SLACK_JAC`` / ``SLACK_START``, measured on the MI355X).

JACOBIAN MUTANTS (only ``fun_fd``, the six perturbed sweeps of an iteration, differs; ``fun`` never does):
  "no-history"   they read zero histories;                 "no-c2"      they read c1 * current only (``c2 * older`` dropped);
  "hist-j+1"     they read the history of column j + 1;    "half-col-k" column k is perturbed by half its step, the
  "mid=j"        RK4 only: their stages 2 and 3 read                          quotient divides by the whole step (k = 0 .. 5).
                 column j's history (rk4_cases' "hist23=j", perturbed sweeps only);
START RULES (kr_step_batch's ``predictor``, knode_rod.h): 0 warm start; 1 / 2 linear / quadratic extrapolation in time of
the unknowns - for single shooting (n, m) at the base, slots 19 .. 24 of record 0 - from state_cur, state_prev, state_prev2,
at the highest order <= the rule the states of the loop allow (step 0: 0, step 1: 1); -1 the highest order, which in this
loop IS rule 2 step by step.  START MUTANTS of rule k: "order0" the order silently 0 (= rule 0's run); "sign" the
extrapolated increment subtracted instead of added; "zero" G = 0 at every step.

Cases: B = 3 rods of ``batch_sine_controls(3, T, DEL_T, 1235)``.  Jacobian cells: T = 8 at each type's stopping rule
(``mlp_shape_cases.RULE``).  Start cells: T = 16 at ``tol = 1e-10`` in fp64 only - an fp32 update cannot be measured to 1e-10
of |G|, and at the default tolerances the counts are quantised to 3 - 4 per step whatever the start.  Parameter sets: the
None preset ("preset"), "damping", "full-asym" (``DIAG = false``) and its diagonal twin; under RK4 the last two only (the
preset is not solved on a coarse grid under RK4, rk4_cases.py).

Every count is in tests/golden/sweep_counts.npz, written by tests/golden/make_golden_sweep_counts.py from this module (the
1400 oracle runs take minutes of NumPy); the CPU test recomputes small cells and compares."""
import functools

import numpy as np

import full_matrix_cases as fm
import mlp_shape_cases as sc
from conftest import load_golden

DEL_T = sc.DEL_T
CTL_SEED = 1235
B = sc.B
T_JAC, T_START = 8, 16
TOL_START = 1e-10
# A mutant keeps the root: its stored states are the exact run's to a hundred update tolerances.  The stopping rule bounds
# the last update of G (relative to max(1, |G|)); a degraded Jacobian converges linearly and leaves factor / (1 - factor)
# of that update behind (the slowest mutant here takes 28 sweeps per step: factor 0.6), the sweep carries the error of G
# into the stored state, and the exact run has its own tolerance.  Measured worst: 1.04e-7 (fp64 rule), 8.6e-5 (fp32 rule).
ROOT_TOL = {"f64": 1e-6, "f32": 1e-3}
MAXIT = 50                       # newton_shoot's cap: a step of a mutant that does not converge counts 50
PSETS = ("preset", "damping", "full-asym", "twin")
PSETS_OF = {"euler": PSETS, "rk4": ("full-asym", "twin")}
DTYPES = ("f64", "f32")
HALF_COLS = tuple(f"half-col-{k}" for k in range(6))
JAC_MUTANTS = {"euler": ("no-history", "no-c2", "hist-j+1") + HALF_COLS,
               "rk4": ("no-history", "no-c2", "hist-j+1") + HALF_COLS + ("mid=j",)}
START_RULES = (1, 2, -1)
START_MUTANTS = ("order0", "sign", "zero")
# the grids of the GPU rows: K2a 9, 20; K2b 9, 20, 27 (ragged sub-intervals at 9 and 27); K2d W = 2 at 20, 27, W = 4 at 27,
# 40 (N - 1 >= 2 (4 + 3 (W - 1)): the 7- and 13-interval distributed condensation).  K2d has Euler sweeps only (msw_waves,
# kr_plan.hip): with RK4 and waves_per_rod = 2 the planner runs K2b, which has its own rows.
FAMILIES = {"K2a": ("single", 1, (9, 20)), "K2b": ("multi", 1, (9, 20, 27)),
            "K2d-W2": ("multi", 2, (20, 27)), "K2d-W4": ("multi", 4, (27, 40))}
FAMILY_SCHEMES = {"K2a": ("euler", "rk4"), "K2b": ("euler", "rk4"), "K2d-W2": ("euler",), "K2d-W4": ("euler",)}
START_FAMILIES = ("K2a", "K2b")
JAC_N = {"euler": (9, 20, 27, 40), "rk4": (9, 20, 27)}
START_N = (9, 20, 27)

# What a family needs over the oracle's sum, per rod: the largest excess of sum(iters) over S_exact seen on the MI355X over
# every cell of the family - Jacobian rows per (family, type), start rows per (family, ``predictor``); LABBOOK.md, "Sweep
# counts with the MLP off", has the run and the per-step tables.  The cap is T, one sweep per step - what
# mlp_shape_cases.count_bound grants K2b; a family that needed more would be a finding, not a reason to raise it.  Where the
# sweeps go: K2a stores the state during the sweep it expects to be the accepted one (``predict_final``, kr_sim_impl.hpp);
# a sweep that meets the stopping rule without having been expected to is followed by one more, which newton_shoot performs
# outside its count.  In fp64 at the default tolerances K2a expects right at every step of every cell: its counts ARE the
# oracle's, step by step.  At tol = 1e-10 with a quadratic start the first update of a step is already below what a second
# sweep needs but above sqrt(tol), the threshold without an estimate of the contraction: one sweep more on most steps.  The
# multiple-shooting families also carry the interval starts as unknowns and accept on |dY_i| as well.
SLACK_JAC = {("K2a", "f64"): 0, ("K2a", "f32"): 6, ("K2b", "f64"): 7, ("K2b", "f32"): 8,
             ("K2d-W2", "f64"): 7, ("K2d-W2", "f32"): 8, ("K2d-W4", "f64"): 7, ("K2d-W4", "f32"): 7}
SLACK_START = {("K2a", 1): 0, ("K2a", 2): 11, ("K2a", -1): 11, ("K2b", 1): 14, ("K2b", 2): 12, ("K2b", -1): 12}
assert all(0 <= v <= T_JAC for v in SLACK_JAC.values()) and all(0 <= v <= T_START for v in SLACK_START.values())


def rule_of(dtype, kind="jac"):
    r = sc.RULE[dtype]
    return dict(tol=TOL_START if kind == "start" else r["tol"], fd_eps=r["fd_eps"])


@functools.lru_cache(maxsize=None)
def controls(T):
    import cosserat_oracle as orc
    c = orc.batch_sine_controls(B, T, DEL_T, CTL_SEED)
    c.setflags(write=False)
    return c


def rod_params(pset, N):
    """The oracles' ``RodParams`` of a parameter set."""
    import cosserat_oracle as orc
    if pset in ("full-asym", "twin"):
        return fm.rod_params(N, pset)
    assert pset in ("preset", "damping"), pset
    return orc.setup_params(None if pset == "preset" else pset, N)


def gpu_robot(pset, N):
    """The same set on a ``CosseratRod`` of the package."""
    from gpu_helpers import make_robot
    if pset in ("full-asym", "twin"):
        return fm.apply_to_rod(make_robot(None, N), pset)
    return make_robot(None if pset == "preset" else pset, N)


# ---------------------------------------------------------------------------
# the mutants, as hooks of mlp_shape_cases.newton_steps
# ---------------------------------------------------------------------------
def jac_hooks(D, mutant):
    """Keyword arguments of ``newton_steps`` for a Jacobian mutant (``None``: the exact Jacobian)."""
    if mutant is None:
        return {}
    if mutant == "no-history":
        return dict(fd_hist=lambda yh, zh, y, z, yo, zo: (np.zeros_like(yh), np.zeros_like(zh)))
    if mutant == "no-c2":
        return dict(fd_hist=lambda yh, zh, y, z, yo, zo: (D.c1 * y, D.c1 * z))
    if mutant == "hist-j+1":  # (the last column keeps its own: no sweep reads past it)
        shift = lambda a: np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
        return dict(fd_hist=lambda yh, zh, y, z, yo, zo: (shift(yh), shift(zh)))
    if mutant == "mid=j":
        return dict(fd_mid=lambda yh, zh: (yh[:, :-1].copy(), zh[:, :-1].copy()))
    if mutant in HALF_COLS:
        k = HALF_COLS.index(mutant)

        def point(g0, gp):
            d = gp - g0
            c = int(np.argmax(np.abs(d)))
            assert np.count_nonzero(d) == 1, d   # (one column per perturbed sweep)
            if c == k:
                gp = g0 + 0.5 * d
            return gp
        return dict(fd_point=point)
    raise ValueError(mutant)


def start_hook(rule, mutant=None):
    """``start(t, Gs)`` of ``newton_steps`` for kr_step_batch's ``predictor`` = rule in a loop that hands over every state
    it has (step 0: prev == cur, step 1: no prev2), with a start mutant or none."""
    want = 2 if rule < 0 else rule
    if mutant == "order0":
        want = 0

    def start(t, Gs):
        if mutant == "zero":
            return np.zeros(6)
        order = min(want, t)
        g0 = Gs[0]
        if order == 0:
            return g0
        g = 2.0 * g0 - Gs[1] if order == 1 else 3.0 * (g0 - Gs[1]) + Gs[2]
        return g0 - (g - g0) if mutant == "sign" else g
    return start


def run(pset, scheme, N, b, dtype, kind="jac", mutant=None, rule=0):
    """One oracle run of a cell: ``newton_steps``' dict.  kind "jac": T_JAC steps from the warm start with a Jacobian
    mutant; "start": T_START steps at TOL_START from start rule ``rule`` with a start mutant."""
    D = rod_params(pset, N).derived()
    r = rule_of(dtype, kind)
    if kind == "jac":
        assert mutant is None or mutant in JAC_MUTANTS[scheme], mutant
        return sc.newton_steps(D, controls(T_JAC)[b], r["tol"], r["fd_eps"], scheme=scheme, **jac_hooks(D, mutant))
    assert mutant is None or mutant in START_MUTANTS
    return sc.newton_steps(D, controls(T_START)[b], r["tol"], r["fd_eps"], scheme=scheme, start=start_hook(rule, mutant))


def root_deviation(out, exact):
    """Largest distance of a mutant's states from the exact run's, relative per stored state (inf when a step failed)."""
    if not all(out["ok"]):
        return np.inf
    a, e = out["traj"][1:], exact["traj"][1:]
    return float(max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(a, e)))


# ---------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------
def jac_key(scheme, pset, N, dtype):
    return f"jac_{scheme}_{pset}_n{N}_{dtype}"


def start_key(scheme, pset, N):
    return f"start_{scheme}_{pset}_n{N}"


def jac_cells():
    return [(s, p, N, d) for s in ("euler", "rk4") for p in PSETS_OF[s] for N in JAC_N[s] for d in DTYPES]


def start_cells():
    return [(s, p, N) for s in ("euler", "rk4") for p in PSETS_OF[s] for N in START_N]


# rows of a start cell's table: the three distinct exact runs, then the mutants of rules 1 and 2 ("order0" of any rule is
# rule 0's run, rule -1 is rule 2's: module docstring)
START_ROWS = ("rule0", "rule1", "rule2", "sign1", "sign2", "zero")


def jac_counts(scheme, pset, N, dtype):
    """{None | mutant: int[B, T_JAC]} and {mutant: root deviation [B]} of a Jacobian cell, from the fixture."""
    g = load_golden("sweep_counts")
    k = jac_key(scheme, pset, N, dtype)
    names = (None,) + JAC_MUTANTS[scheme]
    it, dev = g[k + "_iters"], g[k + "_dev"]
    assert it.shape == (len(names), B, T_JAC) and dev.shape == (len(names), B), (k, it.shape)
    return dict(zip(names, it)), dict(zip(names, dev))


def start_counts(scheme, pset, N):
    """{row of START_ROWS: int[B, T_START]}, {row: root deviation [B]} of a start cell, from the fixture."""
    g = load_golden("sweep_counts")
    k = start_key(scheme, pset, N)
    it, dev = g[k + "_iters"], g[k + "_dev"]
    assert it.shape == (len(START_ROWS), B, T_START) and dev.shape == (len(START_ROWS), B), (k, it.shape)
    return dict(zip(START_ROWS, it)), dict(zip(START_ROWS, dev))


def start_exact_row(rule):
    return {0: "rule0", 1: "rule1", 2: "rule2", -1: "rule2"}[rule]


def start_mutant_rows(rule):
    """{mutant: row} of the start mutants of a rule."""
    k = 2 if rule < 0 else rule
    return {"order0": "rule0", "sign": f"sign{k}", "zero": "zero"}


# ---------------------------------------------------------------------------
# held sets and bounds
# ---------------------------------------------------------------------------
def slack_of(family, dtype_or_rule, kind="jac"):
    """Jacobian rows: (family, type); start rows: (family, ``predictor``)."""
    return (SLACK_JAC if kind == "jac" else SLACK_START)[family, dtype_or_rule]


def _held(s_exact, s_mut, slack):
    """The mutants a row holds on EVERY rod: the largest set H with min over H of S_mut above the bound H gives.  With
    g = S_mut - S_exact the condition on the smallest held gap g_min is g_min > slack + g_min / 3, so H is every mutant
    whose gap exceeds 1.5 slack on every rod - and then bound = S_exact + slack + g_min / 3 with g_min from H per rod."""
    return tuple(m for m, s in s_mut.items() if all(2.0 * (s[b] - s_exact[b]) > 3.0 * slack for b in range(B)))


def bound_of(s_exact_b, s_held_b, slack):
    return s_exact_b + slack + (min(s_held_b) - s_exact_b) / 3.0


def jac_row(family, scheme, pset, N, dtype):
    """dict(exact=int[B, T], s_exact=[B], s_mut={mutant: [B]}, held=(...), not_held=(...), bound=[B] or None) of a GPU
    row of part a.  ``bound is None``: no mutant is held - the row is dropped ("Not held")."""
    slack = slack_of(family, dtype)
    it, _ = jac_counts(scheme, pset, N, dtype)
    s_exact = it[None].sum(axis=1)
    s_mut = {m: it[m].sum(axis=1) for m in JAC_MUTANTS[scheme]}
    out = dict(exact=it[None], s_exact=s_exact, s_mut=s_mut, slack=slack, held=(), not_held=tuple(s_mut), bound=None)
    held = _held(s_exact, s_mut, slack)
    out["held"], out["not_held"] = held, tuple(m for m in s_mut if m not in held)
    if held:
        out["bound"] = [bound_of(s_exact[b], [s_mut[m][b] for m in held], slack) for b in range(B)]
    return out


def start_row(family, scheme, pset, N, rule):
    """The same for a row of part b (fp64, ``predictor`` = rule)."""
    slack = slack_of(family, rule, "start")
    it, _ = start_counts(scheme, pset, N)
    exact = it[start_exact_row(rule)]
    s_exact = exact.sum(axis=1)
    s_mut = {m: it[r].sum(axis=1) for m, r in start_mutant_rows(rule).items()}
    out = dict(exact=exact, s_exact=s_exact, s_mut=s_mut, slack=slack, held=(), not_held=tuple(s_mut), bound=None)
    held = _held(s_exact, s_mut, slack)
    out["held"], out["not_held"] = held, tuple(m for m in s_mut if m not in held)
    if held:
        out["bound"] = [bound_of(s_exact[b], [s_mut[m][b] for m in held], slack) for b in range(B)]
    return out


def jac_rows():
    """Every (family, scheme, pset, N, dtype) of part a."""
    return [(f, s, p, N, d) for f, (_, _, Ns) in FAMILIES.items() for s in FAMILY_SCHEMES[f] for p in PSETS_OF[s] for N in Ns
            for d in DTYPES]


def start_rows():
    """Every (family, scheme, pset, N, rule) of part b."""
    return [(f, s, p, N, r) for f in START_FAMILIES for s in FAMILY_SCHEMES[f] for p in PSETS_OF[s] for N in FAMILIES[f][2]
            for r in START_RULES]


# ---------------------------------------------------------------------------
# the exact answers the GPU trajectories are compared with (the C oracle: tight Newton, every step converged)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_states(pset, scheme, N, T):
    """float64[B, T + 1, 25, N], read-only."""
    import cosserat_oracle_c as oc
    P = rod_params(pset, N)
    out = []
    for ctl in controls(T):
        _, tr, bad = oc.simulate(P, np.ascontiguousarray(ctl), scheme=scheme)
        assert bad == 0 and np.all(np.isfinite(tr)), (pset, scheme, N, T)
        out.append(tr)
    out = np.array(out)
    out.setflags(write=False)
    return out
