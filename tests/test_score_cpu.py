"""CPU tier of the device evaluation metrics (kr_dtw_batch, kr_pose_mse_batch): the closed-form Euler angles the kernel
and its host twin share against SciPy, the C ABI surface, and the host-side validation of
``knode.simulate_batch(..., score=...)``.  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SCORE_SYMBOLS = ("kr_dtw_batch", "kr_pose_mse_batch")


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_euler_zyx_matches_scipy():
    """20 000 seeded non-unit quaternions whose middle angle stays below 1.4 rad (away from gimbal lock, where SciPy
    switches to another formula): the closed form differs from SciPy by rounding only.  Bound 1e-13; 2.7e-15 was measured
    with SciPy 1.15.3."""
    from scipy.spatial.transform import Rotation
    from krod_eval import euler_zyx
    rng = np.random.default_rng(20240)
    q = rng.normal(size=(40000, 4)) * rng.uniform(0.5, 2.0, size=(40000, 1))
    want = Rotation.from_quat(q, scalar_first=True).as_euler("zyx")
    keep = np.flatnonzero(np.abs(want[:, 1]) < 1.4)[:20000]
    assert keep.size == 20000
    q, want = q[keep], want[keep]
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).min() > 1e-6  # non-unit, every one
    got = euler_zyx(q)
    err = float(np.abs(got - want).max())
    print(f"euler_zyx vs SciPy: max abs difference {err:.2e} (bound 1e-13)")
    assert err < 1e-13
    # leading axes are kept
    assert np.array_equal(euler_zyx(q[:6].reshape(2, 3, 4)), got[:6].reshape(2, 3, 3))


def test_score_symbols_declared_exported_and_bound(lib):
    import krod_native as kn
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name in SCORE_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int
    # argument counts of the bindings follow the prototypes
    for name in SCORE_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        assert len(getattr(lib, name).argtypes) == proto.count(",") + 1, name
    limit = int(re.search(r"#define\s+KR_DTW_MAX_LEN\s+(\d+)", src).group(1))
    assert limit == kn.KR_DTW_MAX_LEN >= 4096


def test_score_calls_refuse_a_null_handle(lib):
    """The first check of both calls needs no device: a null handle is KR_E_ARG with a message."""
    import krod_native as kn
    out = (ctypes.c_double * 2)(7.0, 7.0)
    buf = (ctypes.c_double * 64)()
    assert lib.kr_dtw_batch(None, 1, buf, 1, 3, 3, buf, 1, 3, 3, out, kn.KR_F64, None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert lib.kr_pose_mse_batch(None, 1, 1, buf, buf, 1, out, None, kn.KR_F64, None) == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert list(out) == [7.0, 7.0]


def _robot(N=10):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r)
    r.N = N
    r.compute_intermediate_terms()
    return r


MISUSE = {
    "tip_only": (dict(reference=np.zeros((16, 7, 10))), dict(tip_only=True), "tip_only"),
    "grid points": (dict(reference=np.zeros((16, 7, 11))), {}, "grid points"),
    "too many states": (dict(reference=np.zeros((18, 7, 10))), {}, "states"),
    "rank 2": (dict(reference=np.zeros((7, 10))), {}, "must be"),
    "rank 5": (dict(reference=np.zeros((1, 2, 16, 7, 10))), {}, "must be"),
    "rods": (dict(reference=np.zeros((3, 16, 7, 10))), {}, "rods"),
    "rows": (dict(reference=np.zeros((16, 6, 10))), {}, "rows"),
    "point": (dict(reference=np.zeros((16, 7, 10)), point=10), {}, "point"),
    "no reference": (dict(point=3), {}, "reference"),
}


@pytest.mark.parametrize("case", sorted(MISUSE))
def test_simulate_batch_score_misuse_raises_on_the_host(lib, case):
    """Every misuse of ``score`` is refused before any device call: without a GPU a valid call fails only when it
    reaches the device (no HIP device), a misuse fails earlier and names the argument."""
    import krod_native as kn
    from knode import simulate_batch
    score, kwargs, word = MISUSE[case]
    with pytest.raises(kn.KrError, match=word):
        simulate_batch(_robot(), np.zeros((2, 16, 4)), score=score, **kwargs)


def test_simulate_batch_score_valid_arguments_reach_the_device(lib):
    import torch
    import krod_native as kn
    from knode import simulate_batch
    if torch.cuda.is_available():
        return  # with a device the call simply runs: tests/test_gpu_score.py
    for ref in (np.zeros((16, 7, 10)), np.zeros((17, 25, 10)), np.zeros((2, 1, 7, 10))):
        with pytest.raises(kn.KrError, match="no HIP device"):
            simulate_batch(_robot(), np.zeros((2, 16, 4)), score={"reference": ref, "point": -1})
