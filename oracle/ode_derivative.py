"""Derivative oracle: the 25 x 47 Jacobian of one grid point's map at 50 significant digits.

TEST INFRASTRUCTURE ONLY, like ``cosserat_oracle``.  The map is ``cosserat_oracle.ode`` itself,

    [y(19), yh(19), zh(6), tendon force(3)]  ->  [y_s(19), z(6)],

evaluated on NumPy object arrays of ``mpmath.mpf`` and differentiated by central differences with a step of 1e-20:
at 50 digits the truncation error is of order step^2 = 1e-40 and the rounding error of order 1e-50 / step = 1e-30,
both relative - a derivative with no error to speak of next to any fp64 evaluation of it.  The arithmetic carries
``GUARD`` = 10 digits more than ``dps``: the map holds intermediates (Kse vstar, about 1e5) that are 1e5 and more above
the values whose differences are taken, and without the guard digits that factor shows in the difference quotient
(steps 1e-20 and 1e-15 then agree to 9e-25 only, with them to 3e-30).  mpmath comes with torch
(through sympy), so it is present wherever the test suite runs.

Two derivatives of the same map exist in the project (csrc/kr_vjp.hip, ``cut``):

* uncut - the derivative of the function, what autograd gives through ``ODE_parallel`` (cosserat_ode_torch.py:264-306);
* cut   - what autograd gives through the torch twin's serial ``ODE`` (cosserat_ode_torch.py:137-213), which assembles
  the quadratic part of R(h) (:159-162) and the quaternion-rate matrix Omega(u) (:185-189) with ``torch.tensor``,
  i.e. as new leaves.  Reproduced here by holding the entries of quad(h) and of Omega(u) at the expansion point and
  differentiating through what is left: the factor 2 / (h . h) in R, and h in h_s = 0.5 Omega(u) h.

|q| in the drag term is written sign(q0) q with the sign taken at the expansion point, so that a component q0 = 0
gets the derivative 0 that q |q| has there (and that torch's sign(0) = 0 gives) instead of the O(step) a central
difference across the kink would leave.
"""
from __future__ import annotations

import mpmath
import numpy as np

import cosserat_oracle as orc

N_IN = 47   # y(19), yh(19), zh(6), tf(3)
N_OUT = 25  # y_s(19), z(6)
STEP = "1e-20"
GUARD = 10

_D_ARRAYS = ("Kse_inv", "Kbt_inv", "Kse_vstar", "Bse", "Bbt", "C", "rhoAg", "rhoJ")
_D_SCALARS = ("c0", "rhoA")


def _mp(a):
    """float64 array -> object array of mpf, element by element (every float64 is represented exactly)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for i in np.ndindex(a.shape):
        out[i] = mpmath.mpf(float(a[i]))
    return out


class _MpDerived:
    """The derived terms ``ode`` reads, as mpf: the float64 values of ``Derived`` taken as exact numbers, so the
    oracle differentiates the map with the parameters an fp64 implementation holds."""

    def __init__(self, D):
        for k in _D_ARRAYS:
            setattr(self, k, _mp(getattr(D, k)))
        for k in _D_SCALARS:
            setattr(self, k, mpmath.mpf(float(getattr(D, k))))


def _eval(Dm, x, leaves):
    ys, z = orc.ode(Dm, x[0:19], x[19:38], x[38:44], x[44:47], leaves=leaves)
    return np.concatenate([ys, z])


def jacobian_mp(D, y, yh, zh, tf, cut=False, dps=50, step=STEP, as_float=True):
    """d[y_s, z] / d[y, yh, zh, tf] of one row: float64 ``[25, 47]`` (``as_float=False``: mpf objects).

    Rows are ordered y_s(19), z(6); columns y(19), yh(19), zh(6), tf(3).  The inputs are taken as the exact
    float64 (or float32) numbers they are."""
    with mpmath.workdps(dps + GUARD):
        Dm = D if isinstance(D, _MpDerived) else _MpDerived(D)
        x0 = _mp(np.concatenate([np.asarray(y, np.float64), np.asarray(yh, np.float64),
                                 np.asarray(zh, np.float64), np.asarray(tf, np.float64)]))
        q0 = x0[13:16]
        leaves = {"sign_q": np.array([(q > 0) - (q < 0) for q in q0], dtype=object)}
        if cut:
            leaves["h_quad"] = x0[3:7].copy()
            leaves["u_rate"] = _eval(Dm, x0, leaves)[22:25].copy()
        st = mpmath.mpf(step)
        J = np.empty((N_OUT, N_IN), dtype=object)
        for i in range(N_IN):
            xp, xm = x0.copy(), x0.copy()
            xp[i] = x0[i] + st
            xm[i] = x0[i] - st
            J[:, i] = (_eval(Dm, xp, leaves) - _eval(Dm, xm, leaves)) / (2 * st)
        if not as_float:
            return J
        return np.array([[float(v) for v in row] for row in J], dtype=np.float64)


def jacobian_mp_batch(D, y, yh, zh, tf, cut=False, dps=50):
    """``jacobian_mp`` over rows: ``[Q, 19], [Q, 19], [Q, 6], [Q, 3]`` -> float64 ``[Q, 25, 47]``."""
    y, yh, zh, tf = (np.atleast_2d(np.asarray(a, np.float64)) for a in (y, yh, zh, tf))
    with mpmath.workdps(dps + GUARD):
        Dm = _MpDerived(D)
    return np.stack([jacobian_mp(Dm, y[i], yh[i], zh[i], tf[i], cut=cut, dps=dps) for i in range(y.shape[0])])


def step_agreement(D, y, yh, zh, tf, cut=False, dps=50, steps=("1e-20", "1e-15")):
    """Self-check: the largest entrywise difference between the Jacobians of two step sizes, relative to the
    largest entry of the column it stands in (the scale the difference quotient of that column is formed at)."""
    with mpmath.workdps(dps + GUARD):
        A = jacobian_mp(D, y, yh, zh, tf, cut=cut, dps=dps, step=steps[0], as_float=False)
        B = jacobian_mp(D, y, yh, zh, tf, cut=cut, dps=dps, step=steps[1], as_float=False)
        worst = mpmath.mpf(0)
        for i in range(N_IN):
            scale = max(abs(v) for v in B[:, i])
            if scale == 0:
                assert all(v == 0 for v in A[:, i])
                continue
            worst = max(worst, max(abs(a - b) for a, b in zip(A[:, i], B[:, i])) / scale)
        return float(worst)
