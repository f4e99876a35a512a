"""Shared by tests/test_sick_rod_cpu.py and tests/test_gpu_sick_rod.py (not a test module): a clean input set of a
simulate call and its SICK TWIN, which differs from it in ONE rod ``s``, from ONE step ``t0`` on.

An input set is a dict of float64 arrays: ``ctl[B, T, 4]`` (``orc.batch_sine_controls``), ``loads[B, T, 6]`` (F_tip, M_tip of
every rod and step: the load histories of tests/tip_loads_cases.py, one per rod, scaled per rod) and ``wrench[B, 6]`` (the
F_tip, M_tip a parameter-table row of rod b carries).  A call uses the entries it has a use for.

Sick kinds (the one entry that changes):
  nan_ctl       ctl[s, t0, 1] = NaN, that step only (the states of the rod carry the NaN on)
  overflow_ctl  ctl[s, t0, 1] = 1e200: finite, fp64 runs only; the step must report a nonzero status, not necessarily 2
  nan_row       wrench[s, 0] = NaN: row s of a parameter table has F_tip[0] = NaN - the rod is sick from step 0
  nan_load      loads[s, t0, 0] = NaN, for the loads call"""
import numpy as np

from tip_loads_cases import load_history

KINDS = ("nan_ctl", "overflow_ctl", "nan_row", "nan_load")
T0 = 3          # steady overlapped steps before the failure, more steps after it
DEL_T = 0.05    # every preset's time step (knode.setup_robot)
# family -> (N, B, T, sick rods): the smallest shapes at which the sharing in question exists
SHAPES = {
    "k2a": (10, 11, 7, (2, 10)),     # one full wavefront of eight rods + three; a rod inside it and the last one
    "one_wave": (23, 5, 7, (1, 4)),  # four rods per workgroup: a full and a partial workgroup
    "waves": (27, 3, 7, (1,)),       # 2 or 4 wavefronts per rod (N - 1 = 26 = 2 x 13 sub-intervals)
    "long": (400, 2, 5, (0,)),       # tiles of leading slots read from the states
}
LOAD_CASES = ("const", "jump", "alt", "sine")


def clean_set(family, seed=None):
    """The clean inputs of a family's shape (read-only arrays)."""
    import cosserat_oracle as orc
    N, B, T, _ = SHAPES[family]
    ctl = orc.batch_sine_controls(B, T, DEL_T, 1000 + N if seed is None else seed)
    loads = np.stack([load_history(LOAD_CASES[b % 4], T) * (1.0 + 0.25 * b) for b in range(B)])
    rng = np.random.default_rng(5 + N)
    wrench = np.concatenate([rng.normal(0, 0.05, (B, 3)), rng.normal(0, 0.002, (B, 3))], axis=1)
    out = dict(ctl=ctl, loads=loads, wrench=wrench)
    for v in out.values():
        v.setflags(write=False)
    return out


def sick_entry(kind, s, t0=T0):
    """(array name, index) of the ONE entry the twin changes, and the value it puts there."""
    if kind == "nan_ctl":
        return "ctl", (s, t0, 1), np.nan
    if kind == "overflow_ctl":
        return "ctl", (s, t0, 1), 1e200
    if kind == "nan_row":
        return "wrench", (s, 0), np.nan
    if kind == "nan_load":
        return "loads", (s, t0, 0), np.nan
    raise ValueError(kind)


def first_sick_step(kind, t0=T0):
    """The first step whose solve sees the sick entry."""
    return 0 if kind == "nan_row" else t0


def sick_twin(clean, kind, s, t0=T0):
    """Copies of the clean arrays with the one sick entry written (read-only)."""
    name, idx, value = sick_entry(kind, s, t0)
    out = {k: v.copy() for k, v in clean.items()}
    out[name][idx] = value
    for v in out.values():
        v.setflags(write=False)
    return out


def differing_entries(a, b):
    """[(array name, index tuple)] of every entry in which two input sets differ (a NaN differs from a number, and
    from nothing else)."""
    assert a.keys() == b.keys()
    out = []
    for k in sorted(a):
        assert a[k].shape == b[k].shape, k
        same = (a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))
        out += [(k, tuple(int(i) for i in idx)) for idx in np.argwhere(~same)]
    return out


MODS5 = (None, "damping", "short", "youngs", "noair")  # the table rows of the one-wavefront shape (B = 5)
BANK_NETS = (0, 1, 0, 1, 1)                             # network of rod b in the bank case: both sick rods run network 1


def row_loads(clean):
    """``loads[B, T, 6]`` that repeat every row's own wrench at every step: what a table call does, said as a loads call."""
    T = clean["ctl"].shape[1]
    return np.repeat(clean["wrench"][:, None, :], T, axis=1)
