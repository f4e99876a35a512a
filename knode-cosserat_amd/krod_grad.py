"""Gradients of a rollout on the MI355X: the backward pass over a stored trajectory (``kr_simulate_vjp_batch``).

The reference carries a differentiable sweep (``CosseratRodTorch.getResidualEuler``, cosserat_ode_torch.py:325-367) but
never differentiates the solved step of ``knode.simulate`` (knode.py:70-100).  Here the step adjoint applies the
implicit-function theorem at the converged shooting solution and the rollout composes it backwards in time; d(tip path) /
d(tension history) costs about one forward rollout instead of 4 T + 1 of them by finite differences.

* ``rollout_grad(robot, ctl, states, ...)``: the backward pass for given cotangents.
* ``simulate_tips(robot, ctl)``: a ``torch.autograd.Function`` - ``tips[B, T, 3]`` connected to ``ctl``, so that
  ``loss.backward()`` fills ``ctl.grad``.
* ``rollout_grad(..., physical=True)`` / ``simulate_tips_physical(robot, ctl, theta)``: also the gradient of the rod's
  material parameters E, r, rho, L, vstar, g, Bse, Bbt, C, tendon_dirs (``kr_simulate_vjp_par_batch``) - what a calibration
  of the rod against a recorded run needs, in place of 2 x 43 forward rollouts by finite differences.
* ``rollout_grad(..., robots=[...])`` / ``simulate_tips_batch(robot, robots, ctl, theta, base_motion, tip_loads)``: the
  backward side of a heterogeneous batch (``kr_simulate_vjp_table_batch``) - rod b with the parameters of ``robots[b]``, the
  parameter gradients per rod (many rods, or many starting guesses of one rod, calibrated in one backward pass), and the
  gradient with respect to a base trajectory or a tip-wrench history, step by step.
* ``rollout_grad_bank`` / ``simulate_tips_bank``: the heterogeneous batch with the MLP on (``kr_simulate_vjp_bank_batch``) -
  rod b with the parameters of ``robots[b]`` and network ``net_of_rod[b]`` of K, the weight gradient per network: the
  reference's model-mismatch variants, each with its own trained network, differentiated in one backward pass.
* ``rollout_grad_nn`` / ``simulate_tips_nn``: the same for the KNODE model, physics plus the residual MLP in every sweep
  (``kr_simulate_vjp_nn_batch``) - and the gradient of a rollout loss with respect to the network's weights, which the
  reference never had (it trains one step ahead, physics_train.py:250-259).

* ``softdtw_loss(robot, tips, ref, gamma)``: the loss these gradients were missing - the soft-DTW of every rod's tip path
  to a recorded path that is not sample-aligned with it (``kr_softdtw_batch``), the differentiable form of the DTW the runs
  are scored by; an ``autograd.Function`` that composes with every ``simulate_tips*``.  A caller of ``rollout_grad*`` who
  holds ``states`` seeds the cotangent history in the same launch, and no trajectory leaves the device::

      g = torch.zeros_like(states)                                     # [T + 1, B, N, KR_SLOTS]
      value, _ = h.softdtw(states[1:, :, N - 1, 12:15].permute(1, 0, 2), ref, gamma, g_out=g[1:, :, N - 1, 12:15].permute(1, 0, 2))
      grads = rollout_grad(robot, ctl, states, g_states=g)            # h = robot._native()

Euler sweeps, the handle's parameters; anything else is refused by the library (no fall-back).  The adjoint is
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
                         "physics alone - rollout_grad_nn / simulate_tips_nn differentiate the model with its network")


def _check_ctl(ctl):
    shape = tuple(ctl.shape)
    if len(shape) != 3 or shape[2] != 4 or shape[0] < 1 or shape[1] < 1:
        raise kn.KrError(f"krod_grad: ctl must be [B, T, 4] with B, T >= 1; got {shape}")
    return shape[0], shape[1]


def forward_states(h, ctl_t, tol=1e-12, maxit=0, prev_init=None, use_nn=False):
    """The full history ``states[T + 1, B, N, KR_SLOTS]`` of a run from the straight rod - what the backward pass
    reads (``use_nn``: with the handle's MLP in every sweep).  Returns (states, tip, status)."""
    B, T = ctl_t.shape[0], ctl_t.shape[1]
    states = h.new_state(B, ctl_t.dtype, n_slots=T + 1)
    h.init_straight(states[0])
    G = torch.zeros((B, 6), dtype=ctl_t.dtype, device=ctl_t.device)
    tip = torch.empty((B, T, 3), dtype=ctl_t.dtype, device=ctl_t.device)
    status = torch.zeros((B, T), dtype=torch.int32, device=ctl_t.device)
    h.simulate(ctl_t, states, G, ring=False, tip=tip, status=status, tol=tol, maxit=maxit, prev_init=prev_init, use_nn=use_nn)
    return states, tip, status


def _seed_tips(h, g, g_tips, add=False):
    """dL/d(tip of step t) -> slots 12..14 of the last record of g[t + 1] (``add``: on top of what g holds)"""
    tips = g_tips.to(device=g.device, dtype=g.dtype).permute(1, 0, 2)
    if add:
        g[1:, :, h.N - 1, 12:15] += tips
    else:
        g[1:, :, h.N - 1, 12:15] = tips


def _check_rollout(who, ctl, states, g_states, g_tips):
    B, T = _check_ctl(ctl)
    if g_states is None and g_tips is None:
        raise kn.KrError(f"{who}: give g_states and / or g_tips (a loss has to enter somewhere)")
    if tuple(states.shape)[0] != T + 1:
        raise kn.KrError(f"{who}: states must be the full history [{T + 1}, {B}, N, {kn.KR_SLOTS}] of the forward call, not a "
                         f"ring; got {tuple(states.shape)}")
    if g_tips is not None and tuple(g_tips.shape) != (B, T, 3):
        raise kn.KrError(f"{who}: g_tips must be [{B}, {T}, 3]; got {tuple(g_tips.shape)}")


def _rollout(h, vjp, ctl, states, g_states, g_tips, prev_init, dtype, **kw):
    """What rollout_grad and rollout_grad_nn share after their checks: the arguments on the device, the seeded ``g``, the
    call ``vjp`` (``h.simulate_vjp`` or ``h.simulate_vjp_nn``), and the part of the result dict both have.  Returns
    (the handle's output dict, the result dict)."""
    tdt, dev = _tdt(dtype), f"cuda:{h.device}"
    to_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(device=dev, dtype=tdt).contiguous()
    ctl_t, states_t = to_dev(ctl), to_dev(states)
    g = to_dev(g_states).clone() if g_states is not None else torch.zeros_like(states_t)
    if g_tips is not None:
        _seed_tips(h, g, to_dev(g_tips), add=True)
    out = vjp(ctl_t, states_t, g, prev_init=to_dev(prev_init) if prev_init is not None else None, **kw)
    res = {"ctl": out["g_ctl"].cpu().numpy(), "states": g.cpu().numpy(), "boundary": out["g_bnd"].cpu().numpy(),
           "resid": out["resid"].cpu().numpy(), "status": out["status"].cpu().numpy()}
    if prev_init is not None:
        res["prev_init"] = out["g_prev_init"].cpu().numpy()
    return out, res


def _check_robots(who, robots, B, nn_ok=False):
    """one robot per rod, none with its MLP on (no library call, no device; ``nn_ok``: a bank call, whose networks are the
    call's own - the robots supply the rods alone)"""
    robots = list(robots)
    if len(robots) != B:
        raise kn.KrError(f"{who}: robots holds {len(robots)} rods, ctl {B}")
    for b, r in enumerate(robots):
        if not nn_ok and getattr(r, "_use_nn", False):
            raise kn.KrError(f"{who}: rod {b}: the adjoint of a table call differentiates the physics alone; a robot with its MLP on "
                             "is not served (nothing falls back to the physics)")
    return robots


def _table_rows(who, robot, robots, B, nn_ok=False):
    """The KrParams rows of ``robots`` for a table call of the adjoint, checked on the host without the library: one robot
    per rod, none with its MLP on, N and del_t the carrier's.  (What a row may hold - diagonal matrices, 9 <= N <= 128 - is
    checked by the library when the table is made.)"""
    robots = _check_robots(who, robots, B, nn_ok)
    base = robot._params()
    rows = [r._params() for r in robots]
    for b, p in enumerate(rows):
        for f in ("N", "del_t"):
            if getattr(p, f) != getattr(base, f):
                raise kn.KrError(f"{who}: rod {b}: field {f} = {getattr(p, f)} differs from the carrier robot's {getattr(base, f)} "
                                 "(N and del_t are shared by all rods of a launch)")
    return rows


def rollout_grad(robot, ctl, states, g_states=None, g_tips=None, prev_init=None, dtype="f64", physical=False, robots=None,
                 per_step_boundary=False):
    """Backward pass over a stored rollout of ``robot`` (MLP off): ``ctl[B, T, 4]`` and the FULL history
    ``states[T + 1, B, N, KR_SLOTS]`` of the forward call (host arrays or device tensors; a ring of three states does not
    hold what is needed and is refused).  The loss enters through ``g_states[T + 1, B, N, KR_SLOTS]`` = dL/dstates and / or
    ``g_tips[B, T, 3]`` = dL/d(tip of step t), which is added to slots 12..14 of the last record of ``states[t + 1]``.
    ``prev_init``: the state before ``states[0]`` of a continued run (None: the reference's start, y_prev = y).

    Returns a dict of host arrays: ``ctl`` [B, T, 4] = dL/dctl; ``states`` [T + 1, B, N, KR_SLOTS] = the total adjoint of
    every stored state (entry 0: the gradient with respect to the initial condition); ``boundary`` [B, KR_BND] = dL/d(p0,
    h0, q0, w0, F_tip, M_tip); ``prev_init`` (with one given); ``resid`` [B, T], the relative residual of each step's
    6 x 6 adjoint solve; ``status`` [B, T] (nonzero: that rod's gradients are NaN from that step back).
    ``physical``: the dict also holds ``physical``, a dict of host arrays dL/d(material parameter) per rod, keyed ``E``,
    ``r``, ``rho``, ``L`` [B], ``vstar``, ``g``, ``C`` [B, 3], ``Bse``, ``Bbt`` [B, 3, 3] (every entry an independent
    variable), ``tendon_dirs`` [B, 4, 3] (``kr_simulate_vjp_par_batch``; a rod with a nonzero status has NaN in all).
    ``robots`` (one ``CosseratRod`` per rod, as for ``knode.simulate_batch(robots=...)``): the stored rollout is that of a
    heterogeneous batch, rod b with the parameters of ``robots[b]``, and the call takes the table form
    (``kr_simulate_vjp_table_batch``; ``robot`` carries N, del_t and the device handle): ``physical`` is then the gradient of
    rod b's OWN parameters, and with ``per_step_boundary`` ``boundary`` is [B, T, KR_BND] - entry [b, t] the gradient with
    respect to the boundary values rod b's step t used (``base_motion[b, t]``, then ``tip_loads[b, t]``) - instead of their
    sum over the steps."""
    _check_robot(robot)
    _check_rollout("rollout_grad", ctl, states, g_states, g_tips)
    if robots is None and per_step_boundary:
        raise kn.KrError("rollout_grad: per_step_boundary needs robots=[...] (the handle's boundary is constant in time)")
    if robots is not None:
        rows = _table_rows("rollout_grad", robot, robots, tuple(ctl.shape)[0])
        h = robot._native()
        with h.param_table(rows) as table:
            vjp = lambda *a, **kw: h.simulate_vjp_table(table, *a, **kw)
            out, res = _rollout(h, vjp, ctl, states, g_states, g_tips, prev_init, dtype, need_par=bool(physical),
                                bnd_per_step=bool(per_step_boundary))  # (the host copies of _rollout wait for the call)
        if physical:
            res["physical"] = {k: np.ascontiguousarray(v) for k, v in kn.split_par(out["g_par"].cpu().numpy()).items()}
        return res
    h = robot._native()
    out, res = _rollout(h, h.simulate_vjp, ctl, states, g_states, g_tips, prev_init, dtype, need_par=bool(physical))
    if physical:
        res["physical"] = {k: np.ascontiguousarray(v) for k, v in kn.split_par(out["g_par"].cpu().numpy()).items()}
    return res


# ---- what the three autograd.Functions share: the forward run from ctl, the backward's seeded cotangent ----
def _forward_tips(who, h, ctl, tdt, tol, use_nn=False):
    """ctl on the handle's device, the stored rollout under it, and its tips as ``ctl`` wants them.  ``who``: warn under
    this name about steps that did not converge (None: no warning)."""
    ctl_t = ctl.detach().to(device=f"cuda:{h.device}", dtype=tdt).contiguous()
    states, tip, status = forward_states(h, ctl_t, tol=tol, use_nn=use_nn)
    bad = int((status != 0).sum()) if who else 0
    if bad:  # (the adjoint is that of the exact root: say so, as knode.simulate does, instead of handing back a gradient in silence)
        import warnings
        warnings.warn(f"{who}: {bad} of {status.numel()} rod-steps did not converge to tol = {tol:g}; the gradient of those rods is "
                      "not that of the solved step", RuntimeWarning)
    return ctl_t, states, status, tip.to(device=ctl.device, dtype=ctl.dtype)


def _tip_cotangent(h, states, g_tips):
    g = torch.zeros_like(states)
    _seed_tips(h, g, g_tips)
    return g


class _SimulateTips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, tdt, tol):
        h = robot._native()
        ctl_t, states, status, tip = _forward_tips(None, h, ctl, tdt, tol)
        ctx.h, ctx.ctl_t, ctx.states = h, ctl_t, states
        ctx.like = ctl
        ctx.status = status
        return tip

    @staticmethod
    def backward(ctx, g_tips):
        h, states = ctx.h, ctx.states
        out = h.simulate_vjp(ctx.ctl_t, states, _tip_cotangent(h, states, g_tips), need_bnd=False)
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


# ---- the rod's material parameters as leaves -----------------------------------------------------------------------------
PHYSICAL_SHAPES = {name: shape for name, shape, _ in kn.PAR_BLOCKS}


def _check_theta(theta, who):
    if not isinstance(theta, dict) or not theta:
        raise kn.KrError(f"{who}: theta must be a non-empty dict of torch tensors keyed by parameter name ({', '.join(PHYSICAL_SHAPES)})")
    for k, v in theta.items():
        if k not in PHYSICAL_SHAPES:
            raise kn.KrError(f"{who}: unknown parameter {k!r}; the differentiable ones are {', '.join(PHYSICAL_SHAPES)}")
        if not isinstance(v, torch.Tensor):
            raise kn.KrError(f"{who}: theta[{k!r}] must be a torch tensor (it is a leaf the gradient is connected to)")
        if tuple(v.shape) != PHYSICAL_SHAPES[k]:
            raise kn.KrError(f"{who}: theta[{k!r}] must have shape {PHYSICAL_SHAPES[k]}; got {tuple(v.shape)}")


def _write_theta(robot, names, values):
    """values -> the robot's attributes, then the dependent terms (and with them the vstar the device derives from)"""
    for k, v in zip(names, values):
        a = v.detach().to(device="cpu", dtype=torch.float64).numpy().copy()
        setattr(robot, k, float(a) if a.ndim == 0 else a)
    robot.compute_intermediate_terms()


class _SimulateTipsPhysical(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, tdt, tol, names, *values):
        _write_theta(robot, names, values)
        ctl_t, states, _, tip = _forward_tips("simulate_tips_physical", robot._native(), ctl, tdt, tol)
        ctx.robot, ctx.names, ctx.values = robot, names, [v.detach().clone() for v in values]
        ctx.ctl_t, ctx.states = ctl_t, states
        ctx.like, ctx.vlike = ctl, values
        return tip

    @staticmethod
    def backward(ctx, g_tips):
        _write_theta(ctx.robot, ctx.names, ctx.values)  # (the robot may have carried other values since)
        h, states = ctx.robot._native(), ctx.states
        out = h.simulate_vjp(ctx.ctl_t, states, _tip_cotangent(h, states, g_tips), need_bnd=False, need_par=True)
        by_name = kn.split_par(out["g_par"].sum(dim=0))  # one robot, one parameter set: summed over the batch
        return (out["g_ctl"].to(device=ctx.like.device, dtype=ctx.like.dtype), None, None, None, None,
                *[by_name[k].to(device=v.device, dtype=v.dtype) for k, v in zip(ctx.names, ctx.vlike)])


def simulate_tips_physical(robot, ctl, theta, dtype="f64", tol=1e-12):
    """``simulate_tips`` with the rod's material parameters as leaves: ``theta`` is a dict of torch tensors under the names
    ``E``, ``r``, ``rho``, ``L`` (scalars), ``vstar``, ``g``, ``C`` [3], ``Bse``, ``Bbt`` [3, 3], ``tendon_dirs`` [4, 3] - any
    subset.  The values are written into ``robot`` (which keeps them), its dependent terms are recomputed, the forward call
    runs, and ``tips[B, T, 3]`` comes back connected to ``ctl`` and to every tensor of ``theta``: ``loss.backward()`` fills
    ``ctl.grad`` and ``theta[k].grad`` by one ``kr_simulate_vjp_par_batch``, the latter summed over the batch (one robot is one
    parameter set).  Every entry of ``Bse`` / ``Bbt`` is an independent variable.  MLP off only; unknown names, wrong shapes
    or a robot with its MLP on raise ``KrError`` before anything runs."""
    _check_robot(robot)
    if not isinstance(ctl, torch.Tensor):
        raise kn.KrError("simulate_tips_physical: ctl must be a torch tensor (it is a leaf the gradient is connected to)")
    _check_ctl(ctl)
    _check_theta(theta, "simulate_tips_physical")
    names = tuple(theta)
    return _SimulateTipsPhysical.apply(ctl, robot, _tdt(dtype), float(tol), names, *[theta[k] for k in names])


# ---- a heterogeneous batch: per-rod parameters, a base trajectory and a wrench history as leaves ---------------------------
def _check_theta_batch(theta, B, who):
    if not isinstance(theta, dict):
        raise kn.KrError(f"{who}: theta must be a dict of torch tensors keyed by parameter name ({', '.join(PHYSICAL_SHAPES)})")
    for k, v in theta.items():
        if k not in PHYSICAL_SHAPES:
            raise kn.KrError(f"{who}: unknown parameter {k!r}; the differentiable ones are {', '.join(PHYSICAL_SHAPES)}")
        if not isinstance(v, torch.Tensor):
            raise kn.KrError(f"{who}: theta[{k!r}] must be a torch tensor (it is a leaf the gradient is connected to)")
        if tuple(v.shape) != (B, *PHYSICAL_SHAPES[k]):
            raise kn.KrError(f"{who}: theta[{k!r}] must have shape {(B, *PHYSICAL_SHAPES[k])} (one value per rod); got {tuple(v.shape)}")


def _check_history(name, x, B, T, width, who):
    shape = tuple(np.shape(x)) if not isinstance(x, torch.Tensor) else tuple(x.shape)
    if shape != (B, T, width):
        raise kn.KrError(f"{who}: {name} must be [B, T, {width}] = [{B}, {T}, {width}]; got {shape}")


class _SimulateTipsBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, robots, tdt, tol, names, base_motion, tip_loads, *values):
        for b, r in enumerate(robots):  # theta[k][b] -> robots[b], which keeps it
            _write_theta(r, names, [v[b] for v in values])
        h = robot._native()
        dev = f"cuda:{h.device}"
        rows = _table_rows("simulate_tips_batch", robot, robots, ctl.shape[0])
        table = h.param_table(rows)
        ctl_t = ctl.detach().to(device=dev, dtype=tdt).contiguous()
        B, T = ctl_t.shape[0], ctl_t.shape[1]
        on_dev = lambda x: torch.as_tensor(x.detach() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)).to(device=dev, dtype=tdt)
        loads_t = bnd_t = None
        if base_motion is not None:  # a boundary call: the base history, then the wrench history or each rod's own wrench
            bnd_t = torch.empty((B, T, kn.KR_BND), dtype=tdt, device=dev)
            bnd_t[:, :, :13] = on_dev(base_motion)
            if tip_loads is not None:
                bnd_t[:, :, 13:] = on_dev(tip_loads)
            else:
                own = np.array([list(p.F_tip[:]) + list(p.M_tip[:]) for p in rows], dtype=np.float64)
                bnd_t[:, :, 13:] = torch.as_tensor(own, device=dev).to(tdt)[:, None, :]
        elif tip_loads is not None:
            loads_t = on_dev(tip_loads).contiguous()
        states = h.new_state(B, tdt, n_slots=T + 1)
        h.init_straight(states[0], table=table)
        G = torch.zeros((B, 6), dtype=tdt, device=dev)
        tip = torch.empty((B, T, 3), dtype=tdt, device=dev)
        status = torch.zeros((B, T), dtype=torch.int32, device=dev)
        h.simulate(ctl_t, states, G, ring=False, tip=tip, status=status, tol=tol, table=table, loads=loads_t, bnd=bnd_t)
        bad = int((status != 0).sum())
        if bad:
            import warnings
            warnings.warn(f"simulate_tips_batch: {bad} of {status.numel()} rod-steps did not converge to tol = {tol:g}; the gradient of "
                          "those rods is not that of the solved step", RuntimeWarning)
        ctx.h, ctx.table, ctx.ctl_t, ctx.states, ctx.names = h, table, ctl_t, states, names
        ctx.like, ctx.vlike, ctx.base_like, ctx.loads_like = ctl, values, base_motion, tip_loads
        return tip.to(device=ctl.device, dtype=ctl.dtype)

    @staticmethod
    def backward(ctx, g_tips):
        h, states = ctx.h, ctx.states
        leaf = lambda x: isinstance(x, torch.Tensor) and x.requires_grad
        need_bnd = leaf(ctx.base_like) or leaf(ctx.loads_like)
        out = h.simulate_vjp_table(ctx.table, ctx.ctl_t, states, _tip_cotangent(h, states, g_tips), need_bnd=need_bnd,
                                   bnd_per_step=True, need_par=bool(ctx.names))
        like = lambda g, x: g.to(device=x.device, dtype=x.dtype)
        by_name = kn.split_par(out["g_par"]) if ctx.names else {}  # per rod: [B, *shape], NOT summed
        return (like(out["g_ctl"], ctx.like), None, None, None, None, None,
                like(out["g_bnd"][:, :, :13], ctx.base_like) if leaf(ctx.base_like) else None,
                like(out["g_bnd"][:, :, 13:], ctx.loads_like) if leaf(ctx.loads_like) else None,
                *[like(by_name[k], v) for k, v in zip(ctx.names, ctx.vlike)])


def simulate_tips_batch(robot, robots, ctl, theta=None, base_motion=None, tip_loads=None, dtype="f64", tol=1e-12):
    """``simulate_tips_physical`` for a heterogeneous batch: rod b runs with the parameters of ``robots[b]`` (one
    ``CosseratRod`` per rod, MLP off; ``robot`` carries N, del_t and the device handle) and ``tips[B, T, 3]`` comes back
    connected in torch's graph to

    * ``ctl[B, T, 4]``;
    * every ``theta[k]``, a tensor ``[B, *PHYSICAL_SHAPES[k]]``: ``theta[k][b]`` is written into ``robots[b]`` (which keeps
      it) before the table is built, and ``theta[k].grad`` is PER ROD, not summed - B rods, or B starting guesses of one
      rod, calibrated by one backward pass;
    * ``base_motion[B, T, 13]`` (``p0 h0 q0 w0`` per step) and ``tip_loads[B, T, 6]`` (``F_tip M_tip`` per step), as for
      ``knode.simulate_batch``, where they are tensors that require grad: d(tip path)/d(base trajectory) and
      d(tip path)/d(wrench history), step by step (arrays, or tensors that do not, are inputs only).

    The forward run is the table / loads / boundary call with the full history at ``tol``; the backward pass is one
    ``kr_simulate_vjp_table_batch``.  Raises ``KrError`` before anything runs for robots with the MLP on, wrong shapes,
    unknown names and ``len(robots) != B``."""
    who = "simulate_tips_batch"
    _check_robot(robot)
    if not isinstance(ctl, torch.Tensor):
        raise kn.KrError(f"{who}: ctl must be a torch tensor (it is a leaf the gradient is connected to)")
    B, T = _check_ctl(ctl)
    theta = {} if theta is None else theta
    _check_theta_batch(theta, B, who)
    if base_motion is not None:
        _check_history("base_motion", base_motion, B, T, 13, who)
    if tip_loads is not None:
        _check_history("tip_loads", tip_loads, B, T, 6, who)
    robots = _check_robots(who, robots, B)
    tdt = _tdt(dtype)
    names = tuple(theta)
    return _SimulateTipsBatch.apply(ctl, robot, robots, tdt, float(tol), names, base_motion, tip_loads, *[theta[k] for k in names])


# ---- the KNODE model: physics plus the residual MLP in every sweep ----------------------------------------------------------
ROWS_PER_CHUNK = 1 << 20  # rows of one kr_mlp_forward + kr_mlp_backward pair (whole steps; more: "mlp_grad_accumulate")


def _check_robot_nn(robot, who):
    if not getattr(robot, "_use_nn", False):
        raise kn.KrError(f"{who}: the robot has no MLP on (rollout_grad / simulate_tips differentiate the physics alone)")


def _check_params(params, who):
    """the network's tensors in nn.Linear order W1 [out, in], b1, W2, b2, ... -> number of layers"""
    params = list(params)
    if len(params) < 4 or len(params) % 2:
        raise kn.KrError(f"{who}: params must be the network's tensors W1, b1, W2, b2, ... (nn.Linear order); got {len(params)}")
    for k in range(0, len(params), 2):
        W, b = params[k], params[k + 1]
        if not (isinstance(W, torch.Tensor) and isinstance(b, torch.Tensor)) or W.dim() != 2 or tuple(b.shape) != (W.shape[0],):
            raise kn.KrError(f"{who}: params[{k}], params[{k + 1}] must be torch tensors W [out, in], b [out]")
        if k and W.shape[1] != params[k - 2].shape[0]:
            raise kn.KrError(f"{who}: params[{k}] takes {W.shape[1]} inputs, the layer before gives {params[k - 2].shape[0]}")
    return len(params) // 2


def _acts_of(robot):
    from cosserat_ode import mlp_from_layer_strings
    return [int(a) for a in mlp_from_layer_strings(robot.nn_model, robot.param_ls)[2]]


def _push_params(robot, h, params, who):
    """params -> the handle's network (kr_set_mlp with device sources on the current stream).  Returns the float32 device
    copies, which the caller keeps alive: the sources must stay valid and unmodified until the stream reaches the pack
    launch, and every later use here is on that same stream."""
    acts = _acts_of(robot)
    if len(acts) != len(params) // 2:
        raise kn.KrError(f"{who}: the robot's network has {len(acts)} layers, params describe {len(params) // 2}")
    dev = f"cuda:{h.device}"
    p32 = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
    h.set_mlp_device(p32[0::2], p32[1::2], acts)
    robot._mlp_key = None  # (the handle no longer holds the robot's own weights: the next _native() packs them again)
    return p32, acts


def weight_grads(h, p32, acts, nn_x, nn_g):
    """dL/d(W, b) from the rows the backward pass emitted (``nn_x``, ``nn_g`` ``[T, B, N - 1, 32]``): the ordinary MLP
    backward pass over (x, c), by kr_mlp_forward + kr_mlp_backward in fp32, in chunks of whole steps added up by the library
    (option "mlp_grad_accumulate").  Two identical calls give identical bits at any row count: the calls run with the option
    "mlp_grad_ordered", under which kr_mlp_backward adds up its per-workgroup partial gradients in a fixed order instead of
    with float atomics (a network the fused training kernels do not serve - three layers with two different activations -
    is refused by it, not summed in arbitrary order).  A rod with a nonzero status has NaN rows, and the sum over rods is
    then NaN."""
    import ctypes as C
    n = len(acts)
    Ws, bs = p32[0::2], p32[1::2]
    dims = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
    dims_c, acts_c = (C.c_int32 * (n + 1))(*dims), (C.c_int32 * n)(*acts)
    Wp = (C.c_void_p * n)(*[w.data_ptr() for w in Ws])
    bp = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
    dW = [torch.zeros_like(w) for w in Ws]
    db = [torch.zeros_like(b) for b in bs]
    dWp = (C.c_void_p * n)(*[w.data_ptr() for w in dW])
    dbp = (C.c_void_p * n)(*[b.data_ptr() for b in db])
    T, rows_per_step = nn_x.shape[0], nn_x.shape[1] * nn_x.shape[2]
    steps = max(1, ROWS_PER_CHUNK // rows_per_step)
    was, was_ordered = h.get_option("mlp_grad_accumulate"), h.get_option("mlp_grad_ordered")
    h.set_option("mlp_grad_accumulate", 1)
    h.set_option("mlp_grad_ordered", 1)
    try:
        for t0 in range(0, T, steps):
            x = nn_x[t0:t0 + steps].reshape(-1, 32).float().contiguous()
            g = nn_g[t0:t0 + steps].reshape(-1, 32).float().contiguous()
            Q = x.shape[0]
            ws = torch.empty(max(h.lib.kr_mlp_ws_bytes(n, dims_c, Q), 16), dtype=torch.uint8, device=x.device)
            out = torch.empty((Q, 32), dtype=torch.float32, device=x.device)
            kn.check(h.lib.kr_mlp_forward(h._h, Q, n, dims_c, acts_c, Wp, bp, kn._ptr(x), 32, kn._ptr(out), kn._ptr(ws), kn._stream()))
            kn.check(h.lib.kr_mlp_backward(h._h, Q, n, dims_c, acts_c, Wp, kn._ptr(x), 32, kn._ptr(g), kn._ptr(ws), dWp, dbp,
                                           kn._stream()))
    finally:
        h.set_option("mlp_grad_accumulate", was)
        h.set_option("mlp_grad_ordered", was_ordered)
    grads = []
    for a, b in zip(dW, db):
        grads += [a, b]
    return grads


def rollout_grad_nn(robot, ctl, states, g_states=None, g_tips=None, prev_init=None, dtype="f64", params=None):
    """``rollout_grad`` for a robot with its MLP on (``kr_simulate_vjp_nn_batch``): the same arguments and the same dict.
    ``params`` (the network's tensors in nn.Linear order, the weights the stored rollout was run with): they are pushed
    into the handle first, and the dict also holds ``params``, the list of host arrays dL/dW1, dL/db1, ... summed over
    grid points, rods and steps (``weight_grads``).  Without ``params`` the network is the robot's own."""
    _check_robot_nn(robot, "rollout_grad_nn")
    _check_rollout("rollout_grad_nn", ctl, states, g_states, g_tips)
    if params is not None:
        _check_params(params, "rollout_grad_nn")
    h = robot._native(push_mlp=params is None)  # (params: pushed from the device below, no host pack of the robot's own)
    _tdt(dtype)  # (an unsupported dtype is refused before anything is pushed)
    if params is not None:
        p32, acts = _push_params(robot, h, list(params), "rollout_grad_nn")
    out, res = _rollout(h, h.simulate_vjp_nn, ctl, states, g_states, g_tips, prev_init, dtype, need_rows=params is not None)
    if params is not None:
        res["params"] = [t.cpu().numpy() for t in weight_grads(h, p32, acts, out["nn_x"], out["nn_g"])]
    return res


class _SimulateTipsNn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, tdt, tol, *params):
        h = robot._native(push_mlp=False)  # (no host pack of the robot's own weights: the live ones go in from the device)
        p32, acts = _push_params(robot, h, list(params), "simulate_tips_nn")
        ctl_t, states, _, tip = _forward_tips("simulate_tips_nn", h, ctl, tdt, tol, use_nn=True)
        ctx.robot, ctx.h, ctx.ctl_t, ctx.states, ctx.p32, ctx.acts = robot, h, ctl_t, states, p32, acts
        ctx.like, ctx.plike = ctl, params
        return tip

    @staticmethod
    def backward(ctx, g_tips):
        h, states = ctx.h, ctx.states
        h.set_mlp_device(ctx.p32[0::2], ctx.p32[1::2], ctx.acts)  # (the handle may have served another network since)
        ctx.robot._mlp_key = None  # (... and the robot must not believe its own weights are still the handle's)
        out = h.simulate_vjp_nn(ctx.ctl_t, states, _tip_cotangent(h, states, g_tips), need_bnd=False)
        grads = weight_grads(h, ctx.p32, ctx.acts, out["nn_x"], out["nn_g"])
        return (out["g_ctl"].to(device=ctx.like.device, dtype=ctx.like.dtype), None, None, None,
                *[a.to(device=p.device, dtype=p.dtype) for a, p in zip(grads, ctx.plike)])


def simulate_tips_nn(robot, ctl, params, dtype="f64", tol=1e-12):
    """``simulate_tips`` for a robot with its MLP on: ``tips[B, T, 3]`` connected to ``ctl`` AND to ``params``, the network's
    tensors in nn.Linear order - ``simulate_tips_nn(robot, ctl, params).sum().backward()`` fills ``ctl.grad`` and every
    ``p.grad`` (one ``kr_simulate_vjp_nn_batch``, then the MLP backward pass over the rows it emits).  The forward pushes
    ``params`` into the handle (``kr_set_mlp`` with device sources, on the stream everything else here runs on); the robot
    supplies the architecture (its activations) and the rod."""
    _check_robot_nn(robot, "simulate_tips_nn")
    if not isinstance(ctl, torch.Tensor):
        raise kn.KrError("simulate_tips_nn: ctl must be a torch tensor (it is a leaf the gradient is connected to)")
    _check_ctl(ctl)
    _check_params(params, "simulate_tips_nn")
    return _SimulateTipsNn.apply(ctl, robot, _tdt(dtype), float(tol), *params)


# ---- a heterogeneous batch with a bank of networks: per-rod parameters AND per-rod networks ---------------------------------
def _check_bank(who, params, net_of_rod, B):
    """``params``: K lists of one network's tensors each (nn.Linear order), all of one shape; ``net_of_rod``: one index in
    [0, K) per rod.  Host only.  Returns (K, the int32 index array)."""
    if not isinstance(params, (list, tuple)) or not params or not all(isinstance(p, (list, tuple)) for p in params):
        raise kn.KrError(f"{who}: params must be a list of K per-network lists W1, b1, W2, b2, ... (nn.Linear order)")
    for k, p in enumerate(params):
        _check_params(p, f"{who}: network {k}")
        if [tuple(t.shape) for t in p] != [tuple(t.shape) for t in params[0]]:
            raise kn.KrError(f"{who}: network {k} has another shape than network 0 (all networks of a bank share one shape)")
    nets = np.asarray(net_of_rod)
    if nets.ndim != 1 or nets.size != B or not np.issubdtype(nets.dtype, np.integer):
        raise kn.KrError(f"{who}: net_of_rod must hold one integer per rod ({B}); got shape {tuple(nets.shape)} {nets.dtype}")
    if nets.min() < 0 or nets.max() >= len(params):
        raise kn.KrError(f"{who}: net_of_rod must lie in [0, {len(params)}); got {int(nets.min())} .. {int(nets.max())}")
    return len(params), nets.astype(np.int32)


def _bank_networks(robot, h, params, who):
    """The K networks as ``MlpBank`` reads them from the device: float32 device copies (which the caller keeps alive until the
    stream has reached the pack launches), with the carrier robot's activations.  Returns (p32 per network, acts, networks)."""
    acts = _acts_of(robot)
    if len(acts) != len(params[0]) // 2:
        raise kn.KrError(f"{who}: the robot's network has {len(acts)} layers, params describe {len(params[0]) // 2}")
    dev = f"cuda:{h.device}"
    p32 = [[t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in p] for p in params]
    return p32, acts, [(p[0::2], p[1::2], acts) for p in p32]


def bank_weight_grads(h, p32, acts, nets, nn_x, nn_g):
    """Per network k: ``weight_grads`` over the rows of the rods with ``nets[b] == k``, gathered in rod order, step-major
    (``nn_x``, ``nn_g`` ``[T, B, N - 1, 32]`` in rod order); zeros for a network without rods."""
    grads = []
    for k, pk in enumerate(p32):
        rods = torch.as_tensor(np.flatnonzero(nets == k), dtype=torch.long, device=nn_x.device)
        if rods.numel() == 0:
            grads.append([torch.zeros_like(t) for t in pk])
            continue
        grads.append(weight_grads(h, pk, acts, nn_x.index_select(1, rods).contiguous(), nn_g.index_select(1, rods).contiguous()))
    return grads


def rollout_grad_bank(robot, robots, ctl, states, params, net_of_rod, g_states=None, g_tips=None, prev_init=None, dtype="f64",
                      per_step_boundary=False):
    """``rollout_grad(robots=, per_step_boundary=)`` for a stored rollout of ``knode.simulate_bank`` /
    ``Handle.simulate(..., table=, bank=, net_of_rod=)``: rod b with the parameters of ``robots[b]`` and network
    ``net_of_rod[b]`` of ``params``, a list of K per-network tensor lists in nn.Linear order (the weights the stored rollout
    was run with; they go into a bank from the device).  ``robot`` carries N, del_t, the device handle and the networks'
    activations; its own weights are not read.  The dict of ``rollout_grad`` (``boundary`` [B, KR_BND] or, with
    ``per_step_boundary``, [B, T, KR_BND]), and ``params``: per network k the list of host arrays dL/dW1, dL/db1, ... summed
    over the grid points and steps of ITS rods (``bank_weight_grads``), zeros for a network no rod runs.  One
    ``kr_simulate_vjp_bank_batch``.  Not served: ``physical`` (the parameter gradient with the network on)."""
    who = "rollout_grad_bank"
    _check_rollout(who, ctl, states, g_states, g_tips)
    B = tuple(ctl.shape)[0]
    K, nets = _check_bank(who, params, net_of_rod, B)
    rows = _table_rows(who, robot, robots, B, nn_ok=True)
    _tdt(dtype)
    h = robot._native(push_mlp=False)  # (the handle's own network is neither read nor replaced: the robot keeps its weights)
    p32, acts, networks = _bank_networks(robot, h, params, who)
    with h.param_table(rows) as table, h.mlp_bank(networks) as bank:
        vjp = lambda *a, **kw: h.simulate_vjp_bank(table, bank, nets, *a, **kw)
        out, res = _rollout(h, vjp, ctl, states, g_states, g_tips, prev_init, dtype, bnd_per_step=bool(per_step_boundary))
    res["params"] = [[t.cpu().numpy() for t in g] for g in bank_weight_grads(h, p32, acts, nets, out["nn_x"], out["nn_g"])]
    return res


class _SimulateTipsBank(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctl, robot, robots, tdt, tol, nets, base_motion, tip_loads, n_per, *flat):
        who = "simulate_tips_bank"
        params = [list(flat[k:k + n_per]) for k in range(0, len(flat), n_per)]
        h = robot._native(push_mlp=False)  # (the handle's own network is neither read nor replaced: the robot keeps its weights)
        dev = f"cuda:{h.device}"
        rows = _table_rows(who, robot, robots, ctl.shape[0], nn_ok=True)
        p32, acts, networks = _bank_networks(robot, h, params, who)
        table, bank = h.param_table(rows), h.mlp_bank(networks)
        ctl_t = ctl.detach().to(device=dev, dtype=tdt).contiguous()
        B, T = ctl_t.shape[0], ctl_t.shape[1]
        on_dev = lambda x: torch.as_tensor(x.detach() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)).to(device=dev, dtype=tdt)
        bnd_t = None
        if base_motion is not None or tip_loads is not None:  # per-step data beside a bank is a boundary call
            own = np.array([list(p.p0[:]) + list(p.h0[:]) + list(p.q0[:]) + list(p.w0[:]) + list(p.F_tip[:]) + list(p.M_tip[:])
                            for p in rows], dtype=np.float64)
            bnd_t = torch.as_tensor(own, device=dev).to(tdt)[:, None, :].repeat(1, T, 1)
            if base_motion is not None:
                bnd_t[:, :, :13] = on_dev(base_motion)
            if tip_loads is not None:
                bnd_t[:, :, 13:] = on_dev(tip_loads)
            bnd_t = bnd_t.contiguous()
        states = h.new_state(B, tdt, n_slots=T + 1)
        h.init_straight(states[0], table=table)
        G = torch.zeros((B, 6), dtype=tdt, device=dev)
        tip = torch.empty((B, T, 3), dtype=tdt, device=dev)
        status = torch.zeros((B, T), dtype=torch.int32, device=dev)
        h.simulate(ctl_t, states, G, ring=False, tip=tip, status=status, tol=tol, table=table, bank=bank, net_of_rod=nets, bnd=bnd_t)
        bad = int((status != 0).sum())
        if bad:
            import warnings
            warnings.warn(f"{who}: {bad} of {status.numel()} rod-steps did not converge to tol = {tol:g}; the gradient of those rods is "
                          "not that of the solved step", RuntimeWarning)
        ctx.h, ctx.table, ctx.bank, ctx.nets, ctx.ctl_t, ctx.states = h, table, bank, nets, ctl_t, states
        ctx.p32, ctx.acts, ctx.networks = p32, acts, networks
        ctx.like, ctx.plike, ctx.base_like, ctx.loads_like = ctl, flat, base_motion, tip_loads
        return tip.to(device=ctl.device, dtype=ctl.dtype)

    @staticmethod
    def backward(ctx, g_tips):
        h, states = ctx.h, ctx.states
        leaf = lambda x: isinstance(x, torch.Tensor) and x.requires_grad
        need_bnd = leaf(ctx.base_like) or leaf(ctx.loads_like)
        ctx.bank.repack(ctx.networks)  # (the forward's weights, whatever the bank's arena was asked to hold since)
        out = h.simulate_vjp_bank(ctx.table, ctx.bank, ctx.nets, ctx.ctl_t, states, _tip_cotangent(h, states, g_tips),
                                  need_bnd=need_bnd, bnd_per_step=True)
        grads = bank_weight_grads(h, ctx.p32, ctx.acts, ctx.nets, out["nn_x"], out["nn_g"])
        like = lambda g, x: g.to(device=x.device, dtype=x.dtype)
        flat = [g for gk in grads for g in gk]
        return (like(out["g_ctl"], ctx.like), None, None, None, None, None,
                like(out["g_bnd"][:, :, :13], ctx.base_like) if leaf(ctx.base_like) else None,
                like(out["g_bnd"][:, :, 13:], ctx.loads_like) if leaf(ctx.loads_like) else None, None,
                *[like(g, p) for g, p in zip(flat, ctx.plike)])


def simulate_tips_bank(robot, robots, ctl, params, net_of_rod, base_motion=None, tip_loads=None, dtype="f64", tol=1e-12):
    """``simulate_tips_batch`` with the MLP on and a network per rod: rod b runs with the parameters of ``robots[b]`` and
    network ``net_of_rod[b]`` of ``params`` (K per-network tensor lists in nn.Linear order; ``robot`` carries N, del_t, the
    device handle and the activations, and keeps its own weights).  ``tips[B, T, 3]`` comes back connected to ``ctl``, to
    every ``params[k][i]`` (its ``.grad`` the sum over the rods that run network k; zeros for a network without rods), and
    to ``base_motion[B, T, 13]`` / ``tip_loads[B, T, 6]`` where they are tensors that require grad - with the network on, the
    gradient with respect to a base trajectory that no other call gives.  The forward is the bank call with the full history
    at ``tol`` (a boundary call when either history is given, a rod's own base or wrench where one is not); the backward
    pass is one ``kr_simulate_vjp_bank_batch``, then the MLP backward pass per network over the rows it emits."""
    who = "simulate_tips_bank"
    if not isinstance(ctl, torch.Tensor):
        raise kn.KrError(f"{who}: ctl must be a torch tensor (it is a leaf the gradient is connected to)")
    B, T = _check_ctl(ctl)
    K, nets = _check_bank(who, params, net_of_rod, B)
    if base_motion is not None:
        _check_history("base_motion", base_motion, B, T, 13, who)
    if tip_loads is not None:
        _check_history("tip_loads", tip_loads, B, T, 6, who)
    robots = _check_robots(who, robots, B, nn_ok=True)
    flat = [t for p in params for t in p]
    return _SimulateTipsBank.apply(ctl, robot, robots, _tdt(dtype), float(tol), nets, base_motion, tip_loads, len(params[0]), *flat)


# ---- a loss on the tip path that needs no sample alignment ----------------------------------------------------------------
class _SoftDtwLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tips, ref, h, gamma, cost):
        dev = f"cuda:{h.device}"
        a = tips.detach().to(device=dev)
        b = ref.detach().to(device=dev, dtype=a.dtype)
        need = ctx.needs_input_grad[0]
        out = h.softdtw(a, b, gamma, cost=cost, grad=need)  # (one launch: the value and, where asked for, its gradient)
        value, ctx.g_a = out if need else (out, None)
        return value.to(device=tips.device)

    @staticmethod
    def backward(ctx, g_value):
        g = ctx.g_a * g_value.to(device=ctx.g_a.device, dtype=ctx.g_a.dtype)[:, None, None]
        return g.to(device=g_value.device), None, None, None, None


def softdtw_loss(robot, tips, ref, gamma, cost="l1"):
    """Soft-DTW of every rod's tip path ``tips[B, T, 3]`` (a torch tensor of float32 or float64 on any device, what every
    ``simulate_tips*`` returns) to the recorded path ``ref[B, Tr, 3]`` or ``[Tr, 3]`` (one for all rods; tensor or array,
    taken in the dtype of ``tips``): ``value[B]`` in float64 on the device of ``tips``, connected to ``tips`` in torch's graph.
    ``krod_eval.softdtw_grad`` states value and gradient; ``cost`` is ``"l1"``, the point distance of the DTW the runs are
    scored by, or ``"sq"``; as ``gamma`` -> 0 the value tends to ``krod_eval.dtw_distance`` from below.  ``robot`` supplies the
    device handle, as for the neighbouring functions; none of its parameters is read.  The forward is one
    ``kr_softdtw_batch`` that returns the gradient with the value, the backward multiplies it by the incoming cotangent:
    ``softdtw_loss(robot, simulate_tips(robot, ctl), ref, 1e-2).sum().backward()`` fills ``ctl.grad``.  The recorded path is
    data: no gradient with respect to ``ref`` is formed, and a ``ref`` that requires one is refused."""
    who = "softdtw_loss"
    if not isinstance(tips, torch.Tensor):
        raise kn.KrError(f"{who}: tips must be a torch tensor (it is what the gradient is connected to)")
    if tips.dim() != 3 or tips.shape[2] != 3 or tips.shape[0] < 1 or tips.shape[1] < 1:
        raise kn.KrError(f"{who}: tips must be [B, T, 3] with B, T >= 1; got {tuple(tips.shape)}")
    if tips.dtype not in (torch.float32, torch.float64):
        raise kn.KrError(f"{who}: tips must be float32 or float64; got {tips.dtype}")
    if isinstance(ref, torch.Tensor) and ref.requires_grad:
        raise kn.KrError(f"{who}: ref requires grad; the gradient with respect to the recorded path is not served")
    if not isinstance(ref, torch.Tensor):
        ref = torch.as_tensor(np.asarray(ref, dtype=np.float64))
    B = tips.shape[0]
    if not ((ref.dim() == 2 or (ref.dim() == 3 and ref.shape[0] == B)) and ref.shape[-1] == 3 and ref.shape[-2] >= 1):
        raise kn.KrError(f"{who}: ref must be [{B}, Tr, 3] or [Tr, 3] with Tr >= 1; got {tuple(ref.shape)}")
    gamma, _ = kn.softdtw_args(gamma, cost, tips.shape[1], ref.shape[-2])
    return _SoftDtwLoss.apply(tips, ref, robot._native(), gamma, cost)
