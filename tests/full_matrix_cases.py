"""Shared by tests/test_full_matrices_cpu.py and tests/test_gpu_full_matrices.py (not a test module): the parameter set
"full-asym", its four mutants and its diagonal twin, the cases the step kernels are run on, the runs of
tests/golden/full_matrices.npz (written by tests/golden/make_golden_full_matrices.py from the unmodified reference) and
the comparison of stored states block by block.

"full-asym" is the None preset with ``Bse`` and ``Bbt`` replaced by the ``FULL`` matrices of ode_derivative_cases.py:
nothing symmetric, nothing small (``c0 Bse`` is 0.07 .. 0.19 of ``Kse``'s diagonal at the preset's ``del_t = 0.05``).
Everything else stays the preset's.  Two traps this set is built to avoid: a symmetric matrix cannot tell ``A[3 i + j]``
from ``A[3 j + i]``, and a ``Bse`` of 1e-3 .. 3e-2 is 1e-6 of ``Kse`` and moves nothing a test can see.

The mutants are what a kernel with a wrong full-matrix branch would compute: ``Bse`` or ``Bbt`` transposed, or its
off-diagonals dropped.  The diagonal twin keeps the diagonals of both matrices only: the same numbers through the
``DIAG = true`` instantiation of the same kernel, the control of every comparison.

A stored state ``[25, N]`` (rows p h n m q w v u) is never judged by one norm: q and w are 1e-2 of the record's norm and
``Bse`` acts on them and on n; ``block_errors`` gives the relative L2 error of each of the eight blocks."""
import numpy as np

import ode_derivative_cases as dc
from conftest import load_golden

DEL_T = 0.05  # every preset's time step (knode.setup_robot)
BLOCKS = (("p", 0, 3), ("h", 3, 7), ("n", 7, 10), ("m", 10, 13), ("q", 13, 16), ("w", 16, 19), ("v", 19, 22), ("u", 22, 25))
MUTANTS = ("Bse.T", "Bse.diag", "Bbt.T", "Bbt.diag")
BSE_MUTANTS, BBT_MUTANTS = MUTANTS[:2], MUTANTS[2:]
VARIANTS = ("full-asym", "twin") + MUTANTS

# tolerances of the GPU comparison: (tip path, a block of the stored states).  fp64: the project's bounds (DESIGN.md
# section 2), the state bound applied per block; fp32: the contract's tip bound and the 1e-4 of test_gpu_long_runs.py.
TOL = {"f64": (1e-8, 1e-7), "f32": (1e-5, 1e-4)}
MARGIN = 10.0  # a mutant must miss a compared quantity by this many times its tolerance


def matrices(variant="full-asym"):
    """(Bse, Bbt) of a variant."""
    Bse, Bbt = dc.FULL["Bse"].copy(), dc.FULL["Bbt"].copy()
    if variant == "twin":
        return np.diag(np.diag(Bse)), np.diag(np.diag(Bbt))
    if variant == "Bse.T":
        return Bse.T.copy(), Bbt
    if variant == "Bse.diag":
        return np.diag(np.diag(Bse)), Bbt
    if variant == "Bbt.T":
        return Bse, Bbt.T.copy()
    if variant == "Bbt.diag":
        return Bse, np.diag(np.diag(Bbt))
    if variant != "full-asym":
        raise ValueError(variant)
    return Bse, Bbt


def rod_params(N, variant="full-asym"):
    """The variant as the oracles' ``RodParams``."""
    import cosserat_oracle as orc
    P = orc.setup_params(None, N)
    P.Bse, P.Bbt = matrices(variant)
    return P


def apply_to_rod(robot, variant="full-asym"):
    """The variant on a ``CosseratRod`` that carries the None preset (ours or the reference's): assign, then derive."""
    robot.Bse, robot.Bbt = matrices(variant)
    robot.compute_intermediate_terms()
    return robot


# ---------------------------------------------------------------------------
# controls and cases
# ---------------------------------------------------------------------------
def controls(T, kind="sine"):
    """ctl[T, 4]: ``calc_controls("sine", 1.0)``; "jump": the same with + 0.5 N on tendon 0 from step T // 2 on."""
    import cosserat_oracle as orc
    ctl = np.array(orc.calc_controls("sine", 1.0, DEL_T, T), dtype=np.float64)
    if kind == "jump":
        ctl[T // 2:, 0] += 0.5
    elif kind != "sine":
        raise ValueError(kind)
    return ctl


def batch_controls(T, kind, B):
    """ctl[B, T, 4]: rod 0 the controls above, rod b the same scaled by 1 + 0.01 b."""
    ctl = controls(T, kind)
    return np.stack([ctl * (1.0 + 0.01 * b) for b in range(B)])


# the runs of the fixture: (N, T controls, kind).  The reference drops its last solve: entries 0 .. T - 1.
FIXTURE_RUNS = ((9, 16, "sine"), (40, 16, "sine"), (40, 16, "jump"), (100, 8, "sine"), (400, 5, "sine"))
# every (N, T, kind) a simulate call of the GPU tests runs (each at B = 5, K2a also at B = 9); the shapes are the
# smallest at which a kernel's full-matrix code differs from a neighbour's: ragged sub-intervals at N = 9 / 27 / 131, the
# edges of the one-wavefront persistent kernel at N = 112 (fp64: its LDS) and N = 128 (its register history), the
# workspace history and the states-as-tiles form at N = 400.
SIM_CASES = ((9, 16, "sine"), (12, 16, "sine"), (27, 16, "sine"), (40, 16, "sine"), (40, 16, "jump"), (60, 16, "sine"),
             (100, 8, "sine"), (112, 6, "sine"), (128, 6, "sine"), (131, 6, "sine"), (400, 5, "sine"))
NN_CASE = (12, 8, "sine")                 # with a network of sim_nn.npz in every sweep
NN_NETS = ("elu64", "elu6464", "hist64")  # 28 -> 64 -> 25, 28 -> 64 -> 64 -> 25, 53 -> 64 -> 25 (history inputs)
STEP_CASE = (40, 16, "sine", 8)           # kr_step_batch: entries 7, 8 of this run -> entry 9


def fixture_key(N, kind):
    return f"n{N}_{kind}"


def fixture_entries(T):
    """The entries whose states the fixture stores: every fourth, and the last one (T - 1)."""
    return sorted(set(range(4, T, 4)) | {T - 1})


def fixture_run(N, kind):
    """dict(T, ctl[T, 4], tips[T, 3], ier[T], states = {entry: [25, N]}) of a run of the fixture, or None."""
    if not any((N, kind) == (n, k) for n, _, k in FIXTURE_RUNS):
        return None
    g = load_golden("full_matrices")
    k = fixture_key(N, kind)
    ier = g[k + "_ier"]
    assert np.all(ier == 1), k
    T = len(g[k + "_ctl"])
    states = {int(e): s for e, s in zip(g[k + "_entries"], g[k + "_states"])}
    assert sorted(states) == fixture_entries(T)
    return dict(T=T, ctl=g[k + "_ctl"], tips=g[k + "_tips"], ier=ier, states=states)


def network(name):
    """A network of sim_nn.npz as the oracle's ``Mlp``."""
    import cosserat_oracle as orc
    return orc.mlp_from_arrays(load_golden("sim_nn"), f"mlp_{name}")


# ---------------------------------------------------------------------------
# the oracles' answers, once per process
# ---------------------------------------------------------------------------
_cache = {}


def oracle_run(N, T, kind, variant="full-asym", B=1):
    """The C oracle on the case's B rods: (tips[B, T + 1, 3] with entry 0 the initial tip, states[B, T + 1, 25, N]); every
    step converged.  Read-only, computed once."""
    key = ("c", N, T, kind, variant, B)
    if key not in _cache:
        import cosserat_oracle_c as oc
        P = rod_params(N, variant)
        tips, states = [], []
        for ctl in batch_controls(T, kind, B):
            tip, tr, bad = oc.simulate(P, ctl)
            assert bad == 0 and np.all(np.isfinite(tr)), (N, T, kind, variant)
            tips.append(np.concatenate([tr[0, :3, -1][None], tip]))
            states.append(tr)
        out = (np.array(tips), np.array(states))
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def numpy_oracle_run(N, T, kind, variant="full-asym", B=1, net=None):
    """The NumPy oracle (``solver="newton"``, the only oracle with a network) in the layout of ``oracle_run``."""
    key = ("np", N, T, kind, variant, B, net)
    if key not in _cache:
        import cosserat_oracle as orc
        D = rod_params(N, variant).derived()
        mlp = None if net is None else network(net)
        states = []
        for ctl in batch_controls(T, kind, B):
            tr, info = orc.simulate(D, np.vstack([ctl, ctl[-1:]]), mlp=mlp, solver="newton", return_info=True)
            assert np.all(info["ier"][:T] == 1), (N, T, kind, variant, net)
            states.append(tr[:, :25])
        states = np.array(states)
        out = (np.ascontiguousarray(states[:, :, :3, -1]), states)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def step_case(variant="full-asym", B=1):
    """kr_step_batch's case: (prev[B, 25, N], cur[B, 25, N], tensions[B, 4], next[B, 25, N]) - entries 7, 8 of the
    full-asym run of STEP_CASE (the states a kernel is handed do not depend on the variant), the controls of step 8, and
    the oracle's own step from them under ``variant``, solved to 1e-15 (step_adjoint_cases.oracle_step)."""
    key = ("step", variant, B)
    if key not in _cache:
        import step_adjoint_cases as sac
        N, T, kind, e = STEP_CASE
        _, states = oracle_run(N, T, kind, "full-asym", B)
        ctl = batch_controls(T, kind, B)
        P = rod_params(N, variant)
        nxt = []
        for b in range(B):
            prev, cur = sac.pack(states[b, e - 1, :19], states[b, e - 1, 19:]), sac.pack(states[b, e, :19], states[b, e, 19:])
            rec, _ = sac.oracle_step(P, sac.x_of(cur, prev, ctl[b, e], sac.bnd_of(P)), np.zeros(6))
            nxt.append(np.vstack(sac.unpack(rec)))
        out = (states[:, e - 1], states[:, e], ctl[:, e], np.array(nxt))
        out[3].setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def block_errors(got, ref):
    """{block: relative L2 error of that block's rows} of states ``[..., 25, N]`` (any leading axes: entries, rods -
    taken together per block, never across blocks)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.shape[-2] == 25, (got.shape, ref.shape)
    out = {}
    for name, a, b in BLOCKS:
        nr = float(np.linalg.norm(ref[..., a:b, :]))
        assert nr > 0.0, f"block {name} of the answer is zero"
        out[name] = float(np.linalg.norm(got[..., a:b, :] - ref[..., a:b, :])) / nr
    return out


def tip_error(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.shape[-1] == 3, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def fmt_blocks(errs):
    return " ".join(f"{k}:{v:.1e}" for k, v in errs.items())


def misses(tip_err, blocks, dtype):
    """The largest of (error / tolerance) over the compared quantities of one run: the tip path and the eight blocks."""
    tip_tol, state_tol = TOL[dtype]
    return max([tip_err / tip_tol] + [e / state_tol for e in blocks.values()])
