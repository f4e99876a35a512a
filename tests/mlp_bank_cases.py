"""Inputs and oracle references shared by tests/test_gpu_mlp_bank.py and tests/test_mlp_bank_cpu.py (not a test
module).  Every reference is computed once per process by the CPU oracle's tightly converged Newton solver
(``solver="newton"``), asserts that every step converged (``ier == 1``) and is handed out read-only."""
import functools

import numpy as np

from conftest import load_golden

SEEDS3 = (11, 12, 13, 14)   # three-layer bank 28 -> 64 -> 64 -> 25, ELU
SEEDS2 = (21, 22)           # two-layer bank: bc.npz's mlp_elu64 + these seeds of 28 -> 64 -> 25, ELU
# test 1: six model variants over four networks; test 2: four over three; test 3: the workload's grid size
CASE_THREE = dict(N=20, mods=(None, "damping", "short", "youngs", "noair", "nsw"), nets=(0, 1, 2, 3, 3, 0), steps=20, bank=3)
CASE_TWO = dict(N=20, mods=(None, "damping", "short", "youngs"), nets=(0, 1, 2, 1), steps=20, bank=2)
CASE_N100 = dict(N=100, mods=(None, "damping"), nets=(2, 1), steps=8, bank=3)


@functools.lru_cache(maxsize=None)
def bank_three():
    import cosserat_oracle as orc
    return tuple(orc.make_mlp([28, 64, 64, 25], "elu", seed=s) for s in SEEDS3)


@functools.lru_cache(maxsize=None)
def bank_two():
    import cosserat_oracle as orc
    return (orc.mlp_from_arrays(load_golden("bc"), "mlp_elu64"),) + tuple(orc.make_mlp([28, 64, 25], "elu", seed=s) for s in SEEDS2)


def bank_of(case):
    return bank_three() if case["bank"] == 3 else bank_two()


@functools.lru_cache(maxsize=None)
def controls(steps):
    c = np.array(load_golden("bc")["nn_elu64_ctl"], dtype=np.float64)[:steps]
    assert c.shape == (steps, 4)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle_rod(N, mod, bank, k, steps):
    """float64[steps, 25, N]: entry 0 the straight rod, entry t the state after step t (the last solve is dropped)."""
    import cosserat_oracle as orc
    mlp = (bank_three() if bank == 3 else bank_two())[k]
    traj, info = orc.simulate(orc.setup_params(mod, N).derived(), controls(steps), mlp=mlp, solver="newton", return_info=True)
    assert np.all(info["ier"] == 1), (N, mod, bank, k, info["ier"])
    ref = np.ascontiguousarray(traj[:, :25])
    ref.setflags(write=False)
    return ref


def oracle_case(case):
    return [oracle_rod(case["N"], m, case["bank"], k, case["steps"]) for m, k in zip(case["mods"], case["nets"])]
