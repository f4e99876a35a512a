#!/usr/bin/env python3
"""Writes tests/golden/softdtw.npz: soft-DTW value and gradient of seeded paths by the recurrences of the definition
(include/knode_rod.h, kr_softdtw_batch) in mpmath at 50 digits - independent of krod_eval and of the device.

Per case n (keys ``<n>_<field>``): ``a[Ta, 3]``, ``b[Tb, 3]``, ``gamma``, ``cost`` (0 = L1, 1 = squared Euclidean), ``value``
and ``g_a[Ta, 3]`` rounded to fp64, ``Rmax = max |R(i, j)|`` and ``A[Ta, 3] = sum_j E(i, j) |dc(i, j)/da_ik|`` - the two
quantities the error bounds of the tests are made of, so that a test needs no mpmath.  ``names`` lists the cases.

Cases: Ta x Tb in SHAPES x both costs x gamma in GAMMAS, random walks of step 2e-3 around 0.1 (the scale of tip paths),
plus one pair (``warp``) where b is a with samples repeated - exact zeros of a - b, where sign(0) = 0 matters.

    python3 tests/golden/make_golden_softdtw.py        (about two minutes)"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (63, 65), (64, 64), (65, 64), (101, 101), (40, 130), (130, 67), (129, 200)]
GAMMAS = [1e-6, 1e-3, 1e-1]
COSTS = [0, 1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "softdtw.npz")


def walk(rng, T):
    return 0.1 + np.cumsum(2e-3 * rng.standard_normal((T, 3)), axis=0)


def softdtw_mp(a, b, gamma, cost):
    Ta, Tb = len(a), len(b)
    A_ = [[mp.mpf(float(v)) for v in row] for row in a]
    B_ = [[mp.mpf(float(v)) for v in row] for row in b]
    g = mp.mpf(float(gamma))
    zero, inf = mp.mpf(0), mp.inf
    d = [[[A_[i][k] - B_[j][k] for k in range(3)] for j in range(Tb)] for i in range(Ta)]
    c = [[zero] * (Tb + 2) for _ in range(Ta + 2)]
    for i in range(Ta):
        for j in range(Tb):
            v = d[i][j]
            c[i + 1][j + 1] = abs(v[0]) + abs(v[1]) + abs(v[2]) if cost == 0 else v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    R = [[inf] * (Tb + 2) for _ in range(Ta + 2)]
    R[0][0] = zero
    for i in range(1, Ta + 1):
        for j in range(1, Tb + 1):
            r = (R[i - 1][j], R[i][j - 1], R[i - 1][j - 1])
            m = min(r)
            s = sum(mp.exp((m - x) / g) for x in r if x != inf)
            R[i][j] = c[i][j] + m - g * mp.log(s)
    Rmax = max(abs(R[i][j]) for i in range(1, Ta + 1) for j in range(1, Tb + 1))
    for i in range(Ta + 2):
        R[i][Tb + 1] = -inf
    for j in range(Tb + 2):
        R[Ta + 1][j] = -inf
    R[Ta + 1][Tb + 1] = R[Ta][Tb]
    E = [[zero] * (Tb + 2) for _ in range(Ta + 2)]
    E[Ta + 1][Tb + 1] = mp.mpf(1)
    for i in range(Ta, 0, -1):
        for j in range(Tb, 0, -1):
            e = zero
            for p, q in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
                if E[p][q] != 0:
                    e += E[p][q] * mp.exp((R[p][q] - R[i][j] - c[p][q]) / g)
            E[i][j] = e
    ga = np.zeros((Ta, 3))
    Ab = np.zeros((Ta, 3))
    for i in range(Ta):
        for k in range(3):
            s, sa = zero, zero
            for j in range(Tb):
                dc = mp.sign(d[i][j][k]) if cost == 0 else 2 * d[i][j][k]
                s += E[i + 1][j + 1] * dc
                sa += E[i + 1][j + 1] * abs(dc)
            ga[i, k], Ab[i, k] = float(s), float(sa)
    return float(R[Ta][Tb]), ga, float(Rmax), Ab


def main():
    out, names = {}, []

    def add(name, a, b, gamma, cost):
        value, ga, Rmax, Ab = softdtw_mp(a, b, gamma, cost)
        names.append(name)
        for key, v in (("a", a), ("b", b), ("gamma", np.float64(gamma)), ("cost", np.int32(cost)), ("value", np.float64(value)),
                       ("g_a", ga), ("Rmax", np.float64(Rmax)), ("A", Ab)):
            out[f"{name}_{key}"] = v
        print(name, value, flush=True)

    for n, (Ta, Tb) in enumerate(SHAPES):
        rng = np.random.default_rng(20250 + n)
        a, b = walk(rng, Ta), walk(rng, Tb)
        for cost in COSTS:
            for gamma in GAMMAS:
                add(f"{Ta}x{Tb}_c{cost}_g{gamma:g}", a, b, gamma, cost)
    rng = np.random.default_rng(777)
    a = walk(rng, 40)
    b = a[np.sort(np.concatenate([np.arange(40), rng.integers(0, 40, size=30)]))]  # a, time-warped: 70 samples
    for cost in COSTS:
        for gamma in GAMMAS:
            add(f"warp40x70_c{cost}_g{gamma:g}", a, b, gamma, cost)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
