"""Gradients of a rollout on the MI355X: the backward pass over a stored trajectory (``kr_simulate_vjp_batch``).

The reference carries a differentiable sweep (``CosseratRodTorch.getResidualEuler``, cosserat_ode_torch.py:325-367) but
never differentiates the solved step of ``knode.simulate`` (knode.py:70-100).  Here the step adjoint applies the
implicit-function theorem at the converged shooting solution and the rollout composes it backwards in time; d(tip path) /
d(tension history) costs about one forward rollout instead of 4 T + 1 of them by finite differences.

* ``rollout_grad(robot, ctl, states, ...)``: the backward pass for given cotangents.
* ``simulate_tips(robot, ctl)``: a ``torch.autograd.Function`` - ``tips[B, T, 3]`` connected to ``ctl``, so that
  ``loss.backward()`` fills ``ctl.grad``.

MLP off, Euler sweeps, the handle's parameters; anything else is refused by the library (no fall-back).  The adjoint is
that of the EXACT root of the shooting equations: solve the forward pass tightly (``tol = 1e-12``, the default of
``simulate_tips``) - the distance to the root enters the gradient at first order."""
from __future__ import annotations

import numpy as np
import torch

import krod_native as kn


def _tdt(dtype):
    if dtype in ("f64", torch.float64, np.float64):
        return torch.float64
    if dtype in ("f32", torch.float32, np.float32):
        return torch.float32
    raise kn.KrError(f"unsupported dtype {dtype}")


def _check_robot(robot):
    if getattr(robot, "_use_nn", False):
        raise kn.KrError("krod_grad: the adjoint with the MLP on is not served (kr_step_vjp_batch); nothing falls back to the "
                         "physics alone")


def _check_ctl(ctl):
    shape = tuple(ctl.shape)
    if len(shape) != 3 or shape[2] != 4 or shape[0] < 1 or shape[1] < 1:
        raise kn.KrError(f"krod_grad: ctl must be [B, T, 4] with B, T >= 1; got {shape}")
    return shape[0], shape[1]


def forward_states(h, ctl_t, tol=1e-12, maxit=0, prev_init=None):
    """The full history ``states[T + 1, B, N, KR_SLOTS]`` of a run from the straight rod - what the backward pass
    reads.  Returns (states, tip, status)."""
    B, T = ctl_t.shape[0], ctl_t.shape[1]
    states = h.new_state(B, ctl_t.dtype, n_slots=T + 1)
    h.init_straight(states[0])
    G = torch.zeros((B, 6), dtype=ctl_t.dtype, device=ctl_t.device)
    tip = torch.empty((B, T, 3), dtype=ctl_t.dtype, device=ctl_t.device)
    status = torch.zeros((B, T), dtype=torch.int32, device=ctl_t.device)
    h.simulate(ctl_t, states, G, ring=False, tip=tip, status=status, tol=tol, maxit=maxit, prev_init=prev_init)
    return states, tip, status


def rollout_grad(robot, ctl, states, g_states=None, g_tips=None, prev_init=None, dtype="f64"):
    """Backward pass over a stored rollout of ``robot`` (MLP off): ``ctl[B, T, 4]`` and the FULL history
    ``states[T + 1, B, N, KR_SLOTS]`` of the forward call (host arrays or device tensors; a ring of three states does not
    hold what is needed and is refused).  The loss enters through ``g_states[T + 1, B, N, KR_SLOTS]`` = dL/dstates and / or
    ``g_tips[B, T, 3]`` = dL/d(tip of step t), which is added to slots 12..14 of the last record of ``states[t + 1]``.
    ``prev_init``: the state before ``states[0]`` of a continued run (None: the reference's start, y_prev = y).

    Returns a dict of host arrays: ``ctl`` [B, T, 4] = dL/dctl; ``states`` [T + 1, B, N, KR_SLOTS] = the total adjoint of
    every stored state (entry 0: the gradient with respect to the initial condition); ``boundary`` [B, KR_BND] = dL/d(p0,
    h0, q0, w0, F_tip, M_tip); ``prev_init`` (with one given); ``resid`` [B, T], the relative residual of each step's
    6 x 6 adjoint solve; ``status`` [B, T] (nonzero: that rod's gradients are NaN from that step back)."""
    _check_robot(robot)
    B, T = _check_ctl(ctl)
    if g_states is None and g_tips is None:
        raise kn.KrError("rollout_grad: give g_states and / or g_tips (a loss has to enter somewhere)")
    if tuple(states.shape)[0] != T + 1:
        raise kn.KrError(f"rollout_grad: states must be the full history [{T + 1}, {B}, N, {kn.KR_SLOTS}] of the forward call, not a "
                         f"ring; got {tuple(states.shape)}")
    if g_tips is not None and tuple(g_tips.shape) != (B, T, 3):
        raise kn.KrError(f"rollout_grad: g_tips must be [{B}, {T}, 3]; got {tuple(g_tips.shape)}")
    h = robot._native()
    tdt, dev = _tdt(dtype), f"cuda:{h.device}"
    to_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(device=dev, dtype=tdt).contiguous()
    ctl_t, states_t = to_dev(ctl), to_dev(states)
    g = to_dev(g_states).clone() if g_states is not None else torch.zeros_like(states_t)
    if g_tips is not None:
        g[1:, :, h.N - 1, 12:15] += to_dev(g_tips).permute(1, 0, 2)
    out = h.simulate_vjp(ctl_t, states_t, g, prev_init=to_dev(prev_init) if prev_init is not None else None)
    res = {"ctl": out["g_ctl"].cpu().numpy(), "states": g.cpu().numpy(), "boundary": out["g_bnd"].cpu().numpy(),
           "resid": out["resid"].cpu().numpy(), "status": out["status"].cpu().numpy()}
    if prev_init is not None:
        res["prev_init"] = out["g_prev_init"].cpu().numpy()
    return res


class _SimulateTips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, tdt, tol):
        h = robot._native()
        dev = f"cuda:{h.device}"
        ctl_t = ctl.detach().to(device=dev, dtype=tdt).contiguous()
        states, tip, status = forward_states(h, ctl_t, tol=tol)
        ctx.h, ctx.ctl_t, ctx.states = h, ctl_t, states
        ctx.like = ctl
        ctx.status = status
        return tip.to(device=ctl.device, dtype=ctl.dtype)

    @staticmethod
    def backward(ctx, g_tips):
        h, states = ctx.h, ctx.states
        g = torch.zeros_like(states)
        g[1:, :, h.N - 1, 12:15] = g_tips.to(device=states.device, dtype=states.dtype).permute(1, 0, 2)
        out = h.simulate_vjp(ctx.ctl_t, states, g, need_bnd=False)
        return out["g_ctl"].to(device=ctx.like.device, dtype=ctx.like.dtype), None, None, None


def simulate_tips(robot, ctl, dtype="f64", tol=1e-12):
    """``tips[B, T, 3]`` of a run of ``robot`` (MLP off) from the straight rod under ``ctl[B, T, 4]`` (a torch tensor, on any
    device), connected to ``ctl`` in torch's graph: ``simulate_tips(robot, ctl).sum().backward()`` fills ``ctl.grad`` by one
    ``kr_simulate_vjp_batch``.  The forward solve runs at ``tol`` (default 1e-12: the adjoint is that of the exact root)."""
    _check_robot(robot)
    if not isinstance(ctl, torch.Tensor):
        raise kn.KrError("simulate_tips: ctl must be a torch tensor (it is the leaf the gradient is connected to)")
    _check_ctl(ctl)
    return _SimulateTips.apply(ctl, robot, _tdt(dtype), float(tol))
