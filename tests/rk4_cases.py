"""Shared by tests/test_rk4_sweeps_cpu.py and tests/test_gpu_rk4_sweeps.py (not a test module): the cases the step kernels
are run on with ``scheme = KR_RK4``, the oracles' answers to them, the runs of tests/golden/rk4_sweeps.npz (written by
tests/golden/make_golden_rk4_sweeps.py from the unmodified reference) and the seven mutants of the RK4 sweep.  Parameter
sets, controls and the block-by-block comparison are those of tests/full_matrix_cases.py.

The parameter sets are "full-asym" (through ``DIAG = false``) and its diagonal twin (``DIAG = true``) on EVERY grid, and
never the None preset: under RK4 the reference does not solve the preset on a coarse grid (``ier = 5`` from step 2 on at
N = 9, 12, 20, then NaN; the fixture keeps that ``ier`` row, test_rk4_sweeps_cpu.py::test_preset_is_not_solved_on_a_coarse_grid),
and the coarse grids are where the ragged sub-intervals of the multiple-shooting kernels are.  Both sets carry the larger
damping of ode_derivative_cases.FULL, which is what stabilises RK4 there: the reference solves them with ``ier == 1`` at
every step of every run below.

The mutants are what a kernel with a wrong RK4 sweep would compute: one local sweep function with a ``kind`` switch, put
in the place of ``cosserat_oracle.residual_rk4`` for the duration of one ``cosserat_oracle.simulate`` call."""
from unittest import mock

import numpy as np

import full_matrix_cases as fm
from conftest import load_golden

VARIANTS = ("full-asym", "twin")
# every (N, T, kind) a simulate call of the GPU tests runs: ragged sub-intervals at N = 9 / 27, the edges of the persistent
# kernel at N = 112 (fp64: its LDS) and N = 128 (fp32 only), the first N past it at 131, the workspace history at 400
SIM_CASES = ((9, 16, "sine"), (12, 8, "sine"), (27, 16, "sine"), (40, 16, "sine"), (40, 16, "jump"), (100, 8, "sine"),
             (112, 6, "sine"), (128, 6, "sine"), (131, 6, "sine"), (400, 5, "sine"))
# the runs of the fixture: (variant, N, T controls, kind).  The reference drops its last solve: entries 0 .. T - 1.
FIXTURE_RUNS = (("full-asym", 9, 16, "sine"), ("full-asym", 40, 16, "sine"), ("full-asym", 40, 16, "jump"),
                ("full-asym", 100, 8, "sine"), ("full-asym", 400, 5, "sine"), ("twin", 9, 16, "sine"), ("twin", 40, 16, "sine"))
PRESET_RUN = (9, 16, "sine")              # the None preset under RK4: ``ier`` and tips only, NOT solved by the reference
NN_CASE = (12, 8, "sine")                 # with a network of sim_nn.npz in every sweep
STEP_CASE = (40, 16, "sine", 8)           # kr_step_batch: entries 7, 8 of this run -> entry 9

MUTANTS = ("euler", "hist23=j", "hist4=j", "hist4=mid", "k3<-k1", "weights1331", "vu<-stage4")
HISTORY_MUTANTS = ("euler", "hist23=j", "hist4=j", "hist4=mid", "vu<-stage4")   # (what an fp32 run holds on a fine grid)
FINE_MUTANTS = ("k3<-k1", "weights1331")  # O(ds^2) and smaller: an fp32 run on a fine grid cannot see them


def fixture_key(variant, N, kind):
    return f"{'full' if variant == 'full-asym' else variant}_n{N}_{kind}"


def fixture_run(N, kind, variant="full-asym"):
    """dict(T, ctl[T, 4], tips[T, 3], ier[T], states = {entry: [25, N]}) of a run of the fixture, or None."""
    if not any((variant, N, kind) == (v, n, k) for v, n, _, k in FIXTURE_RUNS):
        return None
    g = load_golden("rk4_sweeps")
    k = fixture_key(variant, N, kind)
    ier = g[k + "_ier"]
    assert np.all(ier == 1), k
    T = len(g[k + "_ctl"])
    states = {int(e): s for e, s in zip(g[k + "_entries"], g[k + "_states"])}
    assert sorted(states) == fm.fixture_entries(T)
    return dict(T=T, ctl=g[k + "_ctl"], tips=g[k + "_tips"], ier=ier, states=states)


# ---------------------------------------------------------------------------
# the oracles' answers, once per process
# ---------------------------------------------------------------------------
_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def oracle_run(N, T, kind, variant="full-asym", B=1, scheme="rk4"):
    """The C oracle under RK4 on the case's B rods (rod b: rod 0's controls scaled by 1 + 0.01 b), in the layout of
    ``full_matrix_cases.oracle_run``: (tips[B, T + 1, 3], states[B, T + 1, 25, N]); every step converged."""
    key = ("c", N, T, kind, variant, B, scheme)
    if key not in _cache:
        import cosserat_oracle_c as oc
        P = fm.rod_params(N, variant)
        tips, states = [], []
        for ctl in fm.batch_controls(T, kind, B):
            tip, tr, bad = oc.simulate(P, ctl, scheme=scheme)
            assert bad == 0 and np.all(np.isfinite(tr)), (N, T, kind, variant, scheme)
            tips.append(np.concatenate([tr[0, :3, -1][None], tip]))
            states.append(tr)
        _cache[key] = _frozen(np.array(tips), np.array(states))
    return _cache[key]


def _numpy_run(N, T, kind, variant, B, net, must_converge=True):
    import cosserat_oracle as orc
    D = fm.rod_params(N, variant).derived()
    mlp = None if net is None else fm.network(net)
    states = []
    for ctl in fm.batch_controls(T, kind, B):
        with np.errstate(all="ignore"):
            tr, info = orc.simulate(D, np.vstack([ctl, ctl[-1:]]), mlp=mlp, scheme="rk4", solver="newton", return_info=True)
        if must_converge:
            assert np.all(info["ier"][:T] == 1), (N, T, kind, variant, net)
        states.append(tr[:, :25])
    states = np.array(states)
    return _frozen(np.ascontiguousarray(states[:, :, :3, -1]), states)


def numpy_oracle_run(N, T, kind, variant="full-asym", B=1, net=None):
    """The NumPy oracle under RK4 (``solver="newton"``, the only oracle with a network) in the layout of ``oracle_run``."""
    key = ("np", N, T, kind, variant, B, net)
    if key not in _cache:
        _cache[key] = _numpy_run(N, T, kind, variant, B, net)
    return _cache[key]


def step_case(variant="full-asym", B=1):
    """kr_step_batch's case: (prev[B, 25, N], cur[B, 25, N], tensions[B, 4], next[B, 25, N]) - entries 7, 8 of the
    variant's own RK4 run of STEP_CASE, the controls of step 8, and the oracle's entry 9."""
    N, T, kind, e = STEP_CASE
    _, states = oracle_run(N, T, kind, variant, B)
    return states[:, e - 1], states[:, e], fm.batch_controls(T, kind, B)[:, e], states[:, e + 1]


# ---------------------------------------------------------------------------
# the mutants of the sweep
# ---------------------------------------------------------------------------
def mutant_sweep(kind):
    """``cosserat_oracle.residual_rk4`` with one thing wrong (``kind`` of MUTANTS); ``None``: nothing wrong, the control of
    this function itself."""
    import cosserat_oracle as orc
    assert kind is None or kind in MUTANTS, kind

    def sweep(D, G, y, z, yh, yh_int, zh, zh_int, tensions, mlp=None):
        if kind == "euler":  # the scheme argument ignored
            return orc.residual_euler(D, G, y, z, yh, zh, tensions, mlp)
        G = np.asarray(G, float)
        y[:, 0] = np.concatenate([D.y0_head, G[0:3], G[3:6], D.y0_tail])
        tf = orc.tendon_force(D, tensions)
        ds = D.ds
        mid = (lambda j: (yh[:, j], zh[:, j])) if kind == "hist23=j" else (lambda j: (yh_int[:, j], zh_int[:, j]))
        end = {"hist4=j": lambda j: (yh[:, j], zh[:, j]), "hist4=mid": mid}.get(kind, lambda j: (yh[:, j + 1], zh[:, j + 1]))
        for j in range(D.N - 1):
            yj = y[:, j]
            k1, z1 = orc.ode(D, yj, yh[:, j], zh[:, j], tf, mlp)
            k2, _ = orc.ode(D, yj + k1 * ds / 2, *mid(j), tf, mlp)
            k3, _ = orc.ode(D, yj + (k1 if kind == "k3<-k1" else k2) * ds / 2, *mid(j), tf, mlp)
            k4, z4 = orc.ode(D, yj + k3 * ds, *end(j), tf, mlp)
            z[:, j] = z4 if kind == "vu<-stage4" else z1
            if kind == "weights1331":  # the 3/8 rule's weights on the classical rule's stages
                y[:, j + 1] = yj + ds * (k1 + 3 * (k2 + k3) + k4) / 8
            else:
                y[:, j + 1] = yj + ds * (k1 + 2 * (k2 + k3) + k4) / 6
        return np.concatenate([D.P.F_tip - y[7:10, -1], D.P.M_tip - y[10:13, -1]])

    return sweep


def mutant_run(N, T, kind, variant, mutant):
    """One rod of the NumPy oracle with the mutant's sweep in the place of ``residual_rk4``, in the layout of
    ``oracle_run``.  A mutant is a wrong scheme, not an unsolvable one: its steps are not required to converge."""
    key = ("mutant", N, T, kind, variant, mutant)
    if key not in _cache:
        import cosserat_oracle as orc
        with mock.patch.object(orc, "residual_rk4", mutant_sweep(mutant)):
            _cache[key] = _numpy_run(N, T, kind, variant, 1, None, must_converge=mutant is None)
    return _cache[key]
