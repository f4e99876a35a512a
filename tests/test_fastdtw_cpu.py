"""CPU tier of FastDTW on the device (kr_fastdtw_batch): the C ABI surface, the per-row interval form of a level's window
against ``krod_eval._expand_window``, ``krod_eval.fastdtw_path``, the host-side validation of
``score={"metric": ..., "radius": ...}`` and the condition that makes the device tests meaningful (FastDTW differs from
the exact DTW on their inputs).  No kernel is launched here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import fastdtw_cases as fc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")
SYMBOLS = {"kr_fastdtw_ws_bytes": ("size_t", ctypes.c_size_t), "kr_fastdtw_batch": ("int", ctypes.c_int)}


@pytest.fixture(scope="module")
def lib():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    return kn.load()


def test_fastdtw_symbols_declared_exported_and_bound(lib):
    import krod_native as kn
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(kn.LIB_PATH)
    for name, (ctype, restype) in SYMBOLS.items():
        proto = re.search(r"\b" + ctype + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert proto, f"{name} is not declared in include/knode_rod.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is restype
        assert len(getattr(lib, name).argtypes) == proto.group(1).count(",") + 1, name
    assert int(re.search(r"#define\s+KR_FASTDTW_MAX_LEN\s+(\d+)", src).group(1)) == kn.KR_FASTDTW_MAX_LEN >= 1024
    assert int(re.search(r"#define\s+KR_FASTDTW_MAX_RADIUS\s+(\d+)", src).group(1)) == kn.KR_FASTDTW_MAX_RADIUS == 8
    assert hasattr(kn.Handle, "fastdtw")
    # the header states what is true now
    text = open(HEADER).read()
    assert "NOT built on the device" not in text


def test_fastdtw_refuses_a_null_handle(lib):
    """The first check needs no device: a null handle is KR_E_ARG with a message, and no output byte is written."""
    import krod_native as kn
    out = (ctypes.c_double * 2)(7.0, 7.0)
    steps = (ctypes.c_int32 * 8)(*([7] * 8))
    count = (ctypes.c_int32 * 2)(7, 7)
    buf = (ctypes.c_double * 64)()
    rc = lib.kr_fastdtw_batch(None, 1, buf, 2, 6, 3, buf, 2, 6, 3, 1, out, steps, count, None, kn.KR_F64, None)
    assert rc == kn.KR_E_ARG
    assert b"handle" in lib.kr_last_error()
    assert list(out) == [7.0, 7.0] and list(steps) == [7] * 8 and list(count) == [7, 7]


def test_fastdtw_ws_bytes_is_monotone_and_aligned(lib):
    import krod_native as kn
    L = kn.KR_FASTDTW_MAX_LEN
    seen_nonzero = False
    for Ta, Tb in [(1, 1), (101, 101), (130, 67), (400, 300), (700, 300), (L, 5), (5, L), (L, L)]:
        for radius in (1, 3, 8):
            last = 0
            for B in (1, 2, 3, 16, 1024):
                n = int(lib.kr_fastdtw_ws_bytes(B, Ta, Tb, radius))
                assert n % 16 == 0, (B, Ta, Tb, radius, n)
                assert n >= last, (B, Ta, Tb, radius, n, last)
                last = n
            seen_nonzero = seen_nonzero or last > 0
    assert seen_nonzero  # (the largest table does not fit the LDS)
    assert int(lib.kr_fastdtw_ws_bytes(1024, 101, 101, 1)) == 0  # the reference's own size needs no workspace
    assert int(lib.kr_fastdtw_ws_bytes(0, 101, 101, 1)) == 0 and int(lib.kr_fastdtw_ws_bytes(4, L + 1, 9, 1)) == 0


WINDOW_PAIRS = [(3, 3), (3, 130), (4, 5), (5, 4), (9, 13), (12, 11), (17, 33), (63, 64), (65, 64), (101, 101), (130, 67)]


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("kind", fc.KINDS)
def test_window_of_every_level_is_one_interval_per_row(kind, radius):
    """What the kernel relies on: on every level of every case, the window ``_expand_window`` builds from the coarse path
    is the per-row interval form (``fastdtw_cases.interval_window``), cell for cell."""
    from krod_eval import _expand_window, _fastdtw
    levels_checked = 0
    for Ta, Tb in WINDOW_PAIRS:
        a, b = fc.sequences(kind, 2, Ta, Tb)
        for r in range(2):
            levels = fc.pyramid([s for s in a[r]], [s for s in b[r]], radius)
            for fine, coarse in zip(levels[:-1], levels[1:]):
                _, path = _fastdtw(coarse[0], coarse[1], radius)
                want = _expand_window(path, len(fine[0]), len(fine[1]), radius)
                got = fc.interval_window(path, len(fine[0]), len(fine[1]), radius)
                assert got == want, (kind, radius, Ta, Tb, r, len(fine[0]), len(fine[1]))
                levels_checked += 1
    assert levels_checked >= 40  # (fewest at radius 3: the pyramid ends at length 4)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_fastdtw_path_returns_the_host_pair(kind):
    from krod_eval import _fastdtw, dtw_distance, fastdtw_distance, fastdtw_path
    for Ta, Tb, radius in [(1, 1, 1), (1, 5, 1), (5, 4, 2), (17, 33, 1), (65, 64, 3), (101, 101, 1)]:
        a, b = fc.sequences(kind, 1, Ta, Tb)
        dist, path = fastdtw_path(a[0], b[0], radius)
        want_dist, want_path = _fastdtw([s for s in a[0]], [s for s in b[0]], radius)
        assert dist == float(want_dist) == fastdtw_distance(a[0], b[0], radius)
        assert path == [(int(i), int(j)) for i, j in want_path]
        assert path[0] == (0, 0) and path[-1] == (Ta - 1, Tb - 1) and len(path) <= Ta + Tb - 1
        steps = {(i1 - i0, j1 - j0) for (i0, j0), (i1, j1) in zip(path[:-1], path[1:])}
        assert steps <= {(1, 0), (0, 1), (1, 1)}, steps
        # the path's own cost is the distance (summed in path order, as the recurrence adds it), and no path beats the DTW
        total = 0.0
        for i, j in path:
            total = total + float(np.abs(a[0][i] - b[0][j]).sum())
        assert total == dist
        assert dist >= dtw_distance(a[0], b[0])
        # the cached host results of the device tests are these
        if (Ta, Tb, radius) in fc.CASES:
            cached_dist, cached_paths = fc.host(kind, 1, Ta, Tb, radius)
            assert cached_dist[0] == dist and cached_paths[0].tolist() == [list(c) for c in path]


def _robot(N=10):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r)
    r.N = N
    r.compute_intermediate_terms()
    return r


MISUSE = {
    "unknown metric": (dict(metric="warp"), "metric"),
    "metric of another type": (dict(metric=1), "metric"),
    "radius 0": (dict(metric="fastdtw", radius=0), "radius"),
    "radius 9": (dict(metric="fastdtw", radius=9), "radius"),
    "radius 1.5": (dict(metric="fastdtw", radius=1.5), "radius"),
    "radius 0 with the exact metric": (dict(radius=0), "radius"),
}


@pytest.mark.parametrize("case", sorted(MISUSE))
def test_score_metric_misuse_raises_on_the_host(lib, case):
    """An unknown metric or a radius outside 1 .. 8 is refused before any device call - in simulate_batch, simulate_bank,
    evaluate_batch and evaluate_bank alike: without a GPU a valid call fails only when it reaches the device."""
    import krod_native as kn
    from knode import simulate_bank, simulate_batch
    from krod_eval import evaluate_bank, evaluate_batch
    extra, word = MISUSE[case]
    ref, ctl = np.zeros((16, 7, 10)), np.zeros((2, 16, 4))
    robot = _robot()
    with pytest.raises(kn.KrError, match=word):
        simulate_batch(robot, ctl, score=dict(reference=ref, **extra))
    with pytest.raises(kn.KrError, match=word):
        simulate_bank(robot, [robot, robot], ctl, score=dict(reference=ref, **extra))
    with pytest.raises(kn.KrError, match=word):
        evaluate_batch(robot, None, ctl, ref, **extra)
    with pytest.raises(kn.KrError, match=word):
        evaluate_bank(robot, [robot, robot], ctl, ref, [9], **extra)


def test_score_fastdtw_refuses_a_reference_beyond_the_limit_on_the_host(lib):
    """More states than KR_FASTDTW_MAX_LEN: refused before the run, not by the library after it; the exact metric serves it."""
    import torch
    import krod_native as kn
    from knode import simulate_batch
    T = kn.KR_FASTDTW_MAX_LEN + 1
    ref, ctl = np.zeros((T, 7, 10)), np.zeros((1, T, 4))
    with pytest.raises(kn.KrError, match="fastdtw serves at most"):
        simulate_batch(_robot(), ctl, score=dict(reference=ref, metric="fastdtw"))
    if not torch.cuda.is_available():
        with pytest.raises(kn.KrError, match="no HIP device"):
            simulate_batch(_robot(), ctl, score=dict(reference=ref))


def test_score_metric_valid_arguments_reach_the_device(lib):
    import torch
    import krod_native as kn
    from knode import simulate_batch
    if torch.cuda.is_available():
        return  # with a device the call simply runs: tests/test_gpu_fastdtw.py
    for extra in (dict(metric="fastdtw"), dict(metric="fastdtw", radius=8), dict(metric="dtw", radius=3), dict(radius=np.int64(2))):
        with pytest.raises(kn.KrError, match="no HIP device"):
            simulate_batch(_robot(), np.zeros((2, 16, 4)), score=dict(reference=np.zeros((16, 7, 10)), point=-1, **extra))


def test_device_cases_separate_fastdtw_from_the_exact_dtw():
    """Guard of tests/test_gpu_fastdtw.py: among the random-walk rods it runs at lengths >= 17 (radius 1), at least one in
    eight has a FastDTW distance that is not the exact DTW's - a kernel that returned the exact distance cannot pass."""
    from krod_eval import dtw_distance
    differ = total = 0
    for Ta, Tb in fc.GUARD_PAIRS:
        a, b = fc.sequences("walk", fc.B16, Ta, Tb)
        fast, _ = fc.host("walk", fc.B16, Ta, Tb, 1)
        exact = np.array([dtw_distance(a[r], b[r]) for r in range(fc.B16)])
        assert np.all(fast >= exact)
        n = int(np.count_nonzero(fast != exact))
        print(f"{Ta} x {Tb}: {n} of {fc.B16} walks have fastdtw != dtw")
        differ += n
        total += fc.B16
    assert len(fc.GUARD_PAIRS) == 7 and total == 112
    assert 8 * differ >= total, (differ, total)
