"""Per-rod parameter tables, host side (no GPU): ``kr_param_table_check`` - which rows may ride in one launch with a
base parameter set - and the argument validation of ``knode.simulate_batch(..., robots=[...])``, which raises before
anything touches a device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

PRESETS = [None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    return kn


def preset_robot(mod, N=10):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r, mod)
    r.N = N
    r.compute_intermediate_terms()
    return r


def test_eight_presets_ride_with_a_preset_base(kn):
    base = preset_robot(None)._params()
    rows = [preset_robot(m)._params() for m in PRESETS]
    rc, bad, msg = kn.param_table_check(base, rows)
    assert (rc, bad) == (0, -1), msg


@pytest.mark.parametrize("field", ["N", "del_t", "nn_input_history"])
def test_shared_fields_must_agree(kn, field):
    from cosserat_ode import CosseratRod
    base = preset_robot(None)._params()
    rows = [preset_robot(m)._params() for m in PRESETS]
    if field == "N":
        rows[5].N = 12
    elif field == "del_t":
        rows[5].del_t = CosseratRod().del_t  # the class default 0.005 against the presets' 0.05
        assert rows[5].del_t == 0.005 and base.del_t == 0.05
    else:
        rows[5].nn_input_history = 1
    rc, bad, msg = kn.param_table_check(base, rows)
    assert rc == kn.KR_E_ARG and bad == 5
    assert field in msg, msg


def test_off_diagonal_damping_is_unsupported(kn):
    base = preset_robot(None)._params()
    rows = [preset_robot(m)._params() for m in PRESETS]
    rows[3].Bbt[1] = 1e-3
    rc, bad, msg = kn.param_table_check(base, rows)
    assert rc == kn.KR_E_UNSUPPORTED and bad == 3
    assert "Bbt" in msg, msg


def test_grid_sizes_outside_the_persistent_kernels_are_unsupported(kn):
    for N in (8, 400):
        base = preset_robot(None, N)._params()
        rc, bad, msg = kn.param_table_check(base, [preset_robot("short", N)._params()])
        assert rc == kn.KR_E_UNSUPPORTED and bad == -1 and "N" in msg, (N, rc, msg)
    for N in (9, 128):
        base = preset_robot(None, N)._params()
        assert kn.param_table_check(base, [preset_robot("short", N)._params()])[0] == 0


def test_empty_and_null_tables(kn):
    lib = kn.load()
    base = preset_robot(None)._params()
    rc, bad, msg = kn.param_table_check(base, [])
    assert rc == kn.KR_E_ARG and msg
    bad = ctypes.c_int64(7)
    assert lib.kr_param_table_check(ctypes.byref(base), 3, None, ctypes.byref(bad)) == kn.KR_E_ARG
    assert lib.kr_param_table_check(None, 1, ctypes.byref(base), None) == kn.KR_E_ARG
    # bad_rod is optional
    assert lib.kr_param_table_check(ctypes.byref(base), 1, ctypes.byref(base), None) == 0
    # a row the derivation itself refuses is an argument error of that row
    row = preset_robot("short")._params()
    row.L = -1.0
    rc, bad, msg = kn.param_table_check(base, [base, row])
    assert rc == kn.KR_E_ARG and bad == 1


def test_simulate_batch_validates_robots_before_any_device_call(kn, monkeypatch):
    import knode
    from cosserat_ode import CosseratRod

    def no_device(self):
        raise AssertionError("simulate_batch touched the device before validating `robots`")
    monkeypatch.setattr(CosseratRod, "_native", no_device)
    carrier = preset_robot(None)
    ctl = np.zeros((3, 5, 4))
    with pytest.raises(kn.KrError, match="2 rods"):
        knode.simulate_batch(carrier, ctl, robots=[preset_robot("short"), preset_robot("nsw")])
    with pytest.raises(kn.KrError, match=r"rod 1.*\bN\b"):
        knode.simulate_batch(carrier, ctl, robots=[preset_robot("short"), preset_robot("nsw", 12), preset_robot(None)])
    other_dt = preset_robot("damping")
    other_dt.del_t = 0.005
    other_dt.compute_intermediate_terms()
    with pytest.raises(kn.KrError, match=r"rod 2.*del_t"):
        knode.simulate_batch(carrier, ctl, robots=[preset_robot("short"), preset_robot("nsw"), other_dt])
    full = preset_robot("youngs")
    full.Bbt = full.Bbt + 1e-3  # off-diagonal entries
    with pytest.raises(kn.KrError) as e:
        knode.simulate_batch(carrier, ctl, robots=[full, preset_robot("nsw"), preset_robot(None)])
    assert e.value.code == kn.KR_E_UNSUPPORTED and "rod 0" in str(e.value) and "Bbt" in str(e.value)


def test_fixtures_the_gpu_tests_rely_on():
    """tests/test_gpu_param_table.py drives rods 0..6 of its eight-mods batch with ``mod_<mod>_ctl``: one time axis
    needs one ``del_t``, and the reference converged on every step of every fixture."""
    g = load_golden("sim_misc")
    for m in PRESETS[1:]:
        assert np.array_equal(g[f"mod_{m}_ctl"], g["mod_noair_ctl"]) and g[f"mod_{m}_ctl"].shape == (16, 4)
        assert np.all(g[f"mod_{m}_ier"] == 1)
    assert np.all(g["random_ier"] == 1)
    b = load_golden("bc")
    for k in ("sim_N20_ier", "sim_N100_ier", "nn_elu64_ier"):
        assert np.all(b[k] == 1)
    assert int(b["nn_elu64_N"]) == 20
