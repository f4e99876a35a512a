"""What the soft-DTW tests share (tests/test_softdtw_cpu.py, tests/test_gpu_softdtw.py): the 50-digit fixture
(tests/golden/softdtw.npz, written by tests/golden/make_golden_softdtw.py), the two derived error bounds, and a second,
cell-by-cell statement of the definition that can be broken on purpose (the test of the tests).

The bounds (n = Ta + Tb - 1, eps = 2^-52): softmin is non-expansive in the sup norm, so cell errors add along at most n cells
and never amplify, and a cell's own error is a few ulp of |R| + gamma ln 3:
    tolR       = 16 n eps (max |R| + gamma ln 3)
a weight's relative error is (the error of three R values) / gamma, and E accumulates over at most n cells:
    tolG[i][k] = n (3 tolR / gamma + 8 eps) sum_j E(i, j) |dc/da_ik|
They are derived, not fitted; the same bounds hold the host statement and the device."""
import functools

import numpy as np

from conftest import load_golden

EPS = 2.0 ** -52
COST_NAMES = {0: "l1", 1: "sq"}
MUTANTS = ("diag_cost", "edge_row", "corner", "sign_d", "no_log")

# At gamma = 1e-6 the table has hardened to one warp path and a mutant is felt only if the mistake lies ON that path - the
# data's accident, not the shape's.  Recorded per case: the mutants that the shape and the cost let in (test_softdtw_cpu.
# _structure) and that the case nevertheless does NOT see (stays within the bounds); every other one it must miss by ten
# bounds.  Why: the hard minimum (no_log) changes nothing where the optimal path has no near-tie - all L1 cases here, and
# 40 x 130 squared, which stays just inside (0.95 of tolR); the 101 x 101 squared path crosses the stripe along the first row,
# off the edge mutant; in the warped L1 pair all weight sits on cells with a - b = 0, whose derivative is zero whatever E is.
HARD_UNSEEN = {
    "2x3_c0_g1e-06": ("no_log",), "63x65_c0_g1e-06": ("no_log",), "64x64_c0_g1e-06": ("no_log",), "65x64_c0_g1e-06": ("no_log",),
    "101x101_c0_g1e-06": ("no_log",), "40x130_c0_g1e-06": ("no_log",), "130x67_c0_g1e-06": ("no_log",),
    "129x200_c0_g1e-06": ("no_log",), "40x130_c1_g1e-06": ("no_log",), "101x101_c1_g1e-06": ("edge_row",),
    "warp40x70_c0_g1e-06": ("diag_cost", "corner", "sign_d", "no_log"),
}


@functools.lru_cache(maxsize=None)
def fixture():
    """{name: dict(a, b, gamma, cost ("l1" / "sq"), value, g_a, Rmax, A)} in the order of the file"""
    z = load_golden("softdtw")
    out = {}
    for name in z["names"]:
        name = str(name)
        c = {k: z[f"{name}_{k}"] for k in ("a", "b", "gamma", "cost", "value", "g_a", "Rmax", "A")}
        c["gamma"], c["value"], c["Rmax"] = float(c["gamma"]), float(c["value"]), float(c["Rmax"])
        c["cost"] = COST_NAMES[int(c["cost"])]
        for k in ("a", "b", "g_a", "A"):
            c[k].setflags(write=False)
        out[name] = c
    return out


def names():
    return list(fixture())


def tol_R(Ta, Tb, gamma, Rmax):
    return 16.0 * (Ta + Tb - 1) * EPS * (Rmax + gamma * np.log(3.0))


def tol_G(Ta, Tb, gamma, Rmax, A):
    return (Ta + Tb - 1) * (3.0 * tol_R(Ta, Tb, gamma, Rmax) / gamma + 8.0 * EPS) * np.asarray(A)


def ratios(case, value, g_a):
    """(|value - exact| / tolR, max |g_a - exact| / tolG) of a result against the fixture case; a gradient entry whose bound is
    zero (no cell with a nonzero derivative carries weight) must be exact and counts 0, else inf."""
    Ta, Tb = len(case["a"]), len(case["b"])
    tr = tol_R(Ta, Tb, case["gamma"], case["Rmax"])
    tg = tol_G(Ta, Tb, case["gamma"], case["Rmax"], case["A"])
    rv = abs(float(value) - case["value"]) / tr
    rv = np.inf if np.isnan(rv) else rv  # (a NaN misses every bound)
    err = np.abs(np.asarray(g_a, dtype=np.float64) - case["g_a"])
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rg = np.where(tg > 0.0, err / tg, np.where(err == 0.0, 0.0, np.inf))
    return float(rv), float(rg.max())


def statement(a, b, gamma, cost, mutant=None):
    """(value, g_a) by the definition, one cell at a time in the device's order - stripes of 64 columns, rows inside - with
    plain Python floats.  ``mutant``: one of MUTANTS, a mistake a kernel could make:
      diag_cost  the diagonal successor's weight uses c(i + 1, j) instead of c(i + 1, j + 1)
      edge_row   the first column of a second or later stripe reads its left neighbours one row off
      corner     R(Ta + 1, Tb + 1) is left at -inf
      sign_d     the L1 derivative is d instead of sign(d)
      no_log     softmin without its -gamma log term (the hard minimum)"""
    import math
    assert mutant is None or mutant in MUTANTS
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    Ta, Tb = len(a), len(b)
    inf = math.inf
    d = (a[:, None, :] - b[None, :, :]).tolist()
    c = [[0.0] * (Tb + 2) for _ in range(Ta + 2)]
    for i in range(Ta):
        for j in range(Tb):
            x, y, z = d[i][j]
            c[i + 1][j + 1] = (abs(x) + abs(y)) + abs(z) if cost == "l1" else (x * x + y * y) + z * z
    R = [[inf] * (Tb + 2) for _ in range(Ta + 2)]
    R[0][0] = 0.0
    for j in range(1, Tb + 1):
        off = 1 if mutant == "edge_row" and j > 64 and (j - 1) % 64 == 0 else 0
        for i in range(1, Ta + 1):
            r = (R[i - 1][j], R[i + off][j - 1], R[i - 1 + off][j - 1])
            m = min(r)
            s = 0.0
            for x in r:
                s += math.exp((m - x) / gamma) if x != inf else 0.0
            R[i][j] = c[i][j] + (m - (0.0 if mutant == "no_log" else gamma * math.log(s)))
    value = R[Ta][Tb]
    for i in range(Ta + 2):
        R[i][Tb + 1] = -inf
    for j in range(Tb + 2):
        R[Ta + 1][j] = -inf
    if mutant != "corner":
        R[Ta + 1][Tb + 1] = R[Ta][Tb]
    E = [[0.0] * (Tb + 2) for _ in range(Ta + 2)]
    E[Ta + 1][Tb + 1] = 1.0
    for i in range(Ta, 0, -1):
        for j in range(Tb, 0, -1):
            r = R[i][j]
            e = 0.0
            for p, q in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
                cp = c[i + 1][j] if mutant == "diag_cost" and (p, q) == (i + 1, j + 1) else c[p][q]
                x = (R[p][q] - r - cp) / gamma
                e += E[p][q] * math.exp(min(x, 700.0)) if x != -inf else 0.0  # (700: a mutant's exponent may be positive)
            E[i][j] = e
    g = np.zeros((Ta, 3))
    for i in range(Ta):
        for k in range(3):
            s = 0.0
            for j in range(Tb):
                x = d[i][j][k]
                dc = 2.0 * x if cost == "sq" else (x if mutant == "sign_d" else float(np.sign(x)))
                s += E[i + 1][j + 1] * dc
            g[i, k] = s
    return value, g
