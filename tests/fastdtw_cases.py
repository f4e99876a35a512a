"""Seeded cases of the FastDTW tests (kr_fastdtw_batch against krod_eval._fastdtw) and the per-row interval form of a
level's window, which is what the device kernel computes.

Three kinds of sequences a[B, Ta, 3], b[B, Tb, 3]:
  ``walk``  random walks, the cumulative sum of N(0, 0.01) steps - where FastDTW and the exact DTW part ways;
  ``ints``  samples drawn from {0, 1, 2}: ties between predecessors everywhere, the tie order decides the next window;
  ``sine``  smooth phase-shifted sines, the shape of a rod's tip path.
Host results are computed once per case and shared (``host``)."""
import functools

import numpy as np

KINDS = ("walk", "ints", "sine")
SEED = 20260  # fixed: test_fastdtw_cpu.py asserts that its walks separate FastDTW from the exact DTW
B16 = 16
# (Ta, Tb) of the device tests: no pyramid (lengths under radius + 2), one side running out first (3 x 130), odd lengths
# (a dropped sample; the last fine row reached only through the radius), stripe edges at 63 / 64 / 65 / 129, and the
# reference's own 101 x 101
PAIRS = [(1, 1), (1, 5), (2, 2), (3, 3), (3, 130), (4, 5), (5, 4), (9, 13), (12, 11), (17, 33), (63, 64), (64, 65), (65, 64),
         (63, 129), (101, 101), (130, 67)]
WIDE_RADIUS_PAIRS = [(5, 4), (17, 33), (65, 64), (101, 101)]  # radius 2 and 3 as well
CASES = [(Ta, Tb, 1) for Ta, Tb in PAIRS] + [(Ta, Tb, r) for Ta, Tb in WIDE_RADIUS_PAIRS for r in (2, 3)]
GUARD_PAIRS = [(Ta, Tb) for Ta, Tb in PAIRS if min(Ta, Tb) >= 17]


def sequences(kind, B, Ta, Tb, seed=SEED):
    """a[B, Ta, 3], b[B, Tb, 3] of one kind; the same arguments give the same arrays."""
    rng = np.random.default_rng([seed, KINDS.index(kind), Ta, Tb])
    if kind == "walk":
        a = np.cumsum(rng.normal(size=(B, Ta, 3)) * 0.01, axis=1)
        b = np.cumsum(rng.normal(size=(B, Tb, 3)) * 0.01, axis=1)
    elif kind == "ints":
        a = rng.integers(0, 3, size=(B, Ta, 3)).astype(np.float64)
        b = rng.integers(0, 3, size=(B, Tb, 3)).astype(np.float64)
    else:
        ta = np.linspace(0.0, 1.0, Ta)[None, :, None]
        tb = np.linspace(0.0, 1.0, Tb)[None, :, None]
        freq = rng.uniform(1.0, 4.0, size=(B, 1, 3))
        pa, pb = rng.uniform(0.0, 0.6, size=(B, 1, 3)), rng.uniform(0.0, 0.6, size=(B, 1, 3))
        amp = rng.uniform(0.05, 0.2, size=(B, 1, 3))
        a = amp * np.sin(2 * np.pi * freq * ta + pa)
        b = amp * 1.05 * np.sin(2 * np.pi * freq * tb + pb)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


@functools.lru_cache(maxsize=None)
def host(kind, B, Ta, Tb, radius, seed=SEED, single=False):
    """``(dist[B], paths)`` of krod_eval.fastdtw_path on ``sequences(kind, B, Ta, Tb, seed)``; ``single``: on the samples
    rounded to fp32 (and upcast again).  Read-only: shared between tests."""
    from krod_eval import fastdtw_path
    a, b = sequences(kind, B, Ta, Tb, seed)
    if single:
        a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    res = [fastdtw_path(a[r], b[r], radius) for r in range(B)]
    dist = np.array([d for d, _ in res])
    dist.setflags(write=False)
    return dist, tuple(np.asarray(p, dtype=np.int32).reshape(-1, 2) for _, p in res)


def interval_window(path, len_x, len_y, radius):
    """The window of the level above a coarse ``path`` in the per-row interval form: coarse row c takes
    lo = min(j) - radius, hi = max(j) + radius over the path cells with |i - c| <= radius; fine rows 2c and 2c + 1 get the
    columns [2 lo, 2 hi + 1], clipped to the sequence.  A monotone path has its extremes in the outermost rows, so only
    the first column of row max(c - radius, 0) and the last column of row min(c + radius, last) are needed - the form the
    kernel evaluates.  Returns the cells sorted by row, then column, like ``krod_eval._expand_window``."""
    rows = max(i for i, _ in path) + 1
    jmin, jmax = [None] * rows, [None] * rows
    for i, j in path:
        jmin[i] = j if jmin[i] is None else min(jmin[i], j)
        jmax[i] = j if jmax[i] is None else max(jmax[i], j)
    window = []
    for fi in range(len_x):
        c = fi // 2
        lo = jmin[max(c - radius, 0)] - radius
        hi = jmax[min(c + radius, rows - 1)] + radius
        window.extend((fi, j) for j in range(max(2 * lo, 0), min(2 * hi + 1, len_y - 1) + 1))
    return window


def pyramid(x, y, radius):
    """The levels ``[(x0, y0), (x1, y1), ...]`` krod_eval._fastdtw visits, finest first (lists of samples)."""
    levels = [(list(x), list(y))]
    while len(levels[-1][0]) >= radius + 2 and len(levels[-1][1]) >= radius + 2:
        half = lambda s: [(s[i] + s[i + 1]) / 2 for i in range(0, len(s) - len(s) % 2, 2)]
        levels.append((half(levels[-1][0]), half(levels[-1][1])))
    return levels
