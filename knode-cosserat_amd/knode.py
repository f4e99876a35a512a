"""``setup_robot`` / ``simulate`` - drop-in for ``knode_cosserat/knode.py``.

``simulate(robot, ctl)`` keeps the reference's contract (knode.py:55-102):
``ctl`` is a sequence of T tension 4-vectors, the result is
``float64[T, 50, N]`` with rows ``[y; z; yh; zh]``, entry 0 is the straight
initial rod (whose "history" rows are a copy of the state, knode.py:68) and the
last solved step is dropped (knode.py:102).  The time loop, the BDF2 history
terms and the shooting solve all run on the MI355X (``kr_simulate_batch``);
the shooting unknowns are found by Newton iteration instead of MINPACK hybrd /
L-BFGS-B - same root, see DESIGN.md.

``simulate_batch`` is the batched form the reference lacks: B rods with
individual tension histories in one call.
"""
from __future__ import annotations

import numpy as np

import krod_native as kn
from cosserat_ode import CosseratRod, mlp_digest, mlp_from_layer_strings

_MODS = (None, "noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs")


def setup_robot(robot, mod=None, original=False):
    """Experimental parameter set of the physical robot plus one of the
    model-mismatch variants; reference knode.py:6-53.  Works on ``CosseratRod``
    and ``CosseratRodTorch`` objects."""
    if original:
        raise Exception("--original parameter no longer supported")
    p = kn.KrParams()
    kn.check(kn.load().kr_default_params(p))
    # start from the robot's own values for the fields a modifier may leave untouched
    for k in range(3):
        p.C[k] = float(np.asarray(_to_numpy(robot.C)).reshape(-1)[k])
        p.g[k] = float(np.asarray(_to_numpy(robot.g)).reshape(-1)[k])
    rc = kn.load().kr_apply_preset(p, None if mod is None else str(mod).encode())
    if rc != 0:
        raise Exception("Unknown mod " + str(mod))
    robot.del_t = p.del_t
    robot.L = p.L
    robot.tendon_offset = 0.04445
    robot.r = p.r
    robot.rho = p.rho
    robot.E = p.E
    is_np = isinstance(robot, CosseratRod)
    if mod == "noair":
        robot.C = _like(robot, [0, 0, 0], is_np)
    elif mod == "nsw":
        robot.g = _like(robot, [0, 0, 0], is_np)
    bbt = p.Bbt[0]
    if is_np:
        robot.Bbt = np.diag([bbt, bbt, bbt])
    else:
        import torch
        robot.Bbt = torch.diag(torch.tensor([bbt, bbt, bbt], device=robot.device))
    robot.compute_intermediate_terms()


def setup_robot_original(robot, mod=None):
    """The legacy parameter set, knode_cosserat_realworld/prepare.py:35-73 (``setup_robot(robot, mod,
    original=True)`` there): del_t 0.005, L 0.4, E 209e9, r 0.0012, rho 8000, Bbt 5e-4, modifiers
    None / nsw / short / damping / diameter / youngs / dampstiff / lengthstiff."""
    p = kn.KrParams()
    kn.check(kn.load().kr_default_params(p))
    for k in range(3):
        p.g[k] = float(np.asarray(_to_numpy(robot.g)).reshape(-1)[k])
    rc = kn.load().kr_apply_preset_original(p, None if mod is None else str(mod).encode())
    if rc != 0:
        raise Exception("Unknown mod " + str(mod))
    robot.del_t, robot.L, robot.E, robot.r, robot.rho = p.del_t, p.L, p.E, p.r, p.rho
    is_np = isinstance(robot, CosseratRod)
    if mod == "nsw":
        robot.g = _like(robot, [0, 0, 0], is_np)
    bbt = p.Bbt[0]
    if is_np:
        robot.Bbt = np.diag([bbt, bbt, bbt])
    else:
        import torch
        robot.Bbt = torch.diag(torch.tensor([bbt, bbt, bbt], device=robot.device))
    robot.compute_intermediate_terms()


def _to_numpy(a):
    if hasattr(a, "detach"):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _like(robot, values, is_np):
    if is_np:
        return np.array(values)
    import torch
    return torch.tensor(values, device=robot.device)


def _robots_rows(robot, robots, B):
    """KrParams rows of ``robots`` for a heterogeneous ``simulate_batch``; host-side validation only (no device call)."""
    robots = list(robots)
    if len(robots) != B:
        raise kn.KrError(f"simulate_batch: robots holds {len(robots)} rods, ctl {B}")
    base = robot._params()
    rows = [r._params() for r in robots]
    for b, p in enumerate(rows):
        for f in ("N", "del_t", "nn_input_history"):
            if getattr(p, f) != getattr(base, f):
                raise kn.KrError(f"simulate_batch: rod {b}: field {f} = {getattr(p, f)} differs from the carrier robot's "
                                 f"{getattr(base, f)} (N, del_t and nn_input_history are shared by all rods of a launch)")
    rc, bad, msg = kn.param_table_check(base, rows)
    if rc != 0:
        err = kn.KrError(f"libknode_rod error {rc}: {msg}")
        err.code = rc
        raise err
    return rows


def _robots_networks(robot, robots, zero_ok=False):
    """Networks of ``robots`` for ``simulate_batch(..., per_robot_nn=True)``: ``(networks, net_of_rod)`` with the
    distinct networks in order of first appearance (the digest of CosseratRod._push_mlp tells them apart).  Host-side
    validation only (no device call).  ``zero_ok`` (``simulate_bank``): a robot with ``nn_path is None`` takes a zero
    network of the others' shape - the reference's network-free "baseline" rows in the same launch."""
    base = robot._params()
    keys, networks, net_of_rod = {}, [], []
    model0 = shape0 = None
    for b, r in enumerate(robots):
        model, param_ls = getattr(r, "nn_model", None), getattr(r, "param_ls", None)
        if zero_ok and getattr(r, "nn_path", None) is None:
            net_of_rod.append(None)
            continue
        if getattr(r, "nn_path", None) is None or model is None or param_ls is None:
            raise kn.KrError(f"simulate_batch: rod {b}: per_robot_nn needs a network on every robot (nn_path / nn_model / "
                             "param_ls, as the reference leaves a robot after loading nn_path)")
        if bool(r.nn_input_history) != bool(robot.nn_input_history):
            raise kn.KrError(f"simulate_batch: rod {b}: nn_input_history = {bool(r.nn_input_history)} differs from the "
                             f"carrier robot's {bool(robot.nn_input_history)}")
        names = [str(m) for m in model]
        if model0 is None:
            model0 = names
        elif names != model0:
            raise kn.KrError(f"simulate_batch: rod {b}: layers {names} differ from rod 0's {model0} (the networks of one "
                             "launch share one shape)")
        key = mlp_digest(model, param_ls, r.nn_input_history)
        if key not in keys:
            net = mlp_from_layer_strings(model, param_ls)
            try:
                dims, acts, _ = kn._bank_shape([net])
            except kn.KrError as e:
                raise kn.KrError(f"simulate_batch: rod {b}: {e}") from None
            if shape0 is None:
                shape0 = (dims, acts)
            elif (dims, acts) != shape0:
                raise kn.KrError(f"simulate_batch: rod {b}: network of layer widths {dims}, rod 0's has {shape0[0]} (the "
                                 "networks of one launch share one shape)")
            keys[key] = len(networks)
            networks.append(net)
        net_of_rod.append(keys[key])
    if shape0 is None:
        raise kn.KrError("simulate_batch: no robot carries a network (nn_path is None on all of them): the shape of the zero "
                         "network is that of the others")
    if None in net_of_rod:  # W = 0, b = 0: the MLP's 25 outputs vanish and the rod is the physics alone
        weights, biases, acts0 = networks[0]
        networks.append(([np.zeros_like(w) for w in weights], [np.zeros_like(v) for v in biases], list(acts0)))
        net_of_rod = [len(networks) - 1 if k is None else k for k in net_of_rod]
    dims, acts = shape0
    rc, msg = kn.mlp_bank_check(base, len(networks), dims, acts)
    if rc != 0:
        err = kn.KrError(f"libknode_rod error {rc}: {msg}")
        err.code = rc
        raise err
    return networks, net_of_rod


def _tip_loads(tip_loads, B, T, check_finite=True):
    """``loads[B, T, 6]`` (float64, contiguous) of ``simulate_batch(..., tip_loads=...)`` from ``[B, T, 6]`` or ``[T, 6]``
    (one history for all rods); host-side validation only (no device call)."""
    try:
        L = np.asarray(tip_loads, dtype=np.float64)
    except (TypeError, ValueError):
        raise kn.KrError("simulate_batch: tip_loads must be a numeric array [B, T, 6] or [T, 6]") from None
    if L.ndim == 2:
        if L.shape != (T, 6):
            raise kn.KrError(f"simulate_batch: tip_loads must be [T, 6] = [{T}, 6] (F_tip, M_tip per step); got {L.shape}")
        L = np.broadcast_to(L[None], (B, T, 6))
    elif L.ndim == 3:
        if L.shape[0] != B:
            raise kn.KrError(f"simulate_batch: tip_loads holds {L.shape[0]} rods, ctl {B}")
        if L.shape[1:] != (T, 6):
            raise kn.KrError(f"simulate_batch: tip_loads must be [B, T, 6] = [{B}, {T}, 6] (F_tip, M_tip per step); got {L.shape}")
    else:
        raise kn.KrError(f"simulate_batch: tip_loads must be [B, T, 6] or [T, 6]; got shape {L.shape}")
    # (check_finite=False: a wrench that is not finite is ordinary input to the library - that rod reports status 2 at that
    #  step and no other rod of the batch notices, knode_rod.h "failed steps")
    if check_finite and not np.isfinite(L).all():
        b, t, _ = np.argwhere(~np.isfinite(L))[0]
        raise kn.KrError(f"simulate_batch: tip_loads is not finite at rod {b}, step {t}")
    return np.ascontiguousarray(L)


def _base_motion(base_motion, B, T, check_finite=True):
    """``base[B, T, 13]`` (float64, contiguous) of ``simulate_batch(..., base_motion=...)`` from ``[B, T, 13]`` or
    ``[T, 13]`` (one history for all rods), columns ``p0 (3) h0 (4) q0 (3) w0 (3)``; host-side validation only (no device
    call)."""
    try:
        M = np.asarray(base_motion, dtype=np.float64)
    except (TypeError, ValueError):
        raise kn.KrError("simulate_batch: base_motion must be a numeric array [B, T, 13] or [T, 13]") from None
    if M.ndim == 2:
        if M.shape != (T, 13):
            raise kn.KrError(f"simulate_batch: base_motion must be [T, 13] = [{T}, 13] (p0, h0, q0, w0 per step); got {M.shape}")
        M = np.broadcast_to(M[None], (B, T, 13))
    elif M.ndim == 3:
        if M.shape[0] != B:
            raise kn.KrError(f"simulate_batch: base_motion holds {M.shape[0]} rods, ctl {B}")
        if M.shape[1:] != (T, 13):
            raise kn.KrError(f"simulate_batch: base_motion must be [B, T, 13] = [{B}, {T}, 13] (p0, h0, q0, w0 per step); got {M.shape}")
    else:
        raise kn.KrError(f"simulate_batch: base_motion must be [B, T, 13] or [T, 13]; got shape {M.shape}")
    # (check_finite=False: a base value that is not finite is ordinary input to the library, knode_rod.h "failed steps";
    #  h0 is used as given - not normalised, as in the reference - so only the quaternion that is no rotation at all is
    #  refused here)
    if check_finite:
        if not np.isfinite(M).all():
            b, t, _ = np.argwhere(~np.isfinite(M))[0]
            raise kn.KrError(f"simulate_batch: base_motion is not finite at rod {b}, step {t}")
        zero = ~M[:, :, 3:7].any(axis=2)
        if zero.any():
            b, t = np.argwhere(zero)[0]
            raise kn.KrError(f"simulate_batch: base_motion has a zero quaternion h0 at rod {b}, step {t}")
    return np.ascontiguousarray(M)


def _boundary(base, loads, rows):
    """``bnd[B, T, KR_BND]`` of a boundary call: the base history, then the wrench history or - without one - each rod's
    own ``F_tip`` / ``M_tip`` (``rows``: the KrParams of the rods) on every step."""
    B, T = base.shape[0], base.shape[1]
    bnd = np.empty((B, T, kn.KR_BND), dtype=np.float64)
    bnd[:, :, :13] = base
    if loads is not None:
        bnd[:, :, 13:] = loads
    else:
        for b, p in enumerate(rows):
            bnd[b, :, 13:16] = np.asarray(p.F_tip[:], dtype=np.float64)
            bnd[b, :, 16:19] = np.asarray(p.M_tip[:], dtype=np.float64)
    return bnd


def _key_points(key_points, N):
    """The grid points of ``simulate_batch(..., key_points=[...])`` as the library wants them: int32, sorted, without
    duplicates, each in [0, N) (a negative index counts from the tip); host-side validation only (no library call)."""
    try:
        arr = np.asarray(key_points)
        if arr.size and (arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer)):
            raise TypeError
        pts = [int(p) for p in arr.reshape(-1)] if arr.ndim <= 1 else None
    except (TypeError, ValueError):
        pts = None
    if pts is None:
        raise kn.KrError("simulate_batch: key_points must be a list of integer grid points")
    for p in pts:
        if not -N <= p < N:
            raise kn.KrError(f"simulate_batch: key point {p} outside the rod's {N} grid points")
    idx = sorted({p % N for p in pts})
    if not 1 <= len(idx) <= kn.KR_KEYPOINTS_MAX:
        raise kn.KrError(f"simulate_batch: {len(idx)} key points; a call takes 1 .. {kn.KR_KEYPOINTS_MAX}")
    return np.asarray(idx, dtype=np.int32)


def _base_of_rows(rows, T):
    """``base[B, T, 13]`` of a call without ``base_motion``: each rod's own ``p0 h0 q0 w0`` on every step."""
    base = np.empty((len(rows), T, 13), dtype=np.float64)
    for b, p in enumerate(rows):
        base[b, :] = np.concatenate([np.asarray(p.p0[:], dtype=np.float64), np.asarray(p.h0[:], dtype=np.float64),
                                     np.asarray(p.q0[:], dtype=np.float64), np.asarray(p.w0[:], dtype=np.float64)])
    return base


def _kp_rows(records):
    """Packed key-point records ``[T + 1, B, K, KR_SLOTS]`` (q w v u p h n m, entry 0 = the initial state) as the result's
    ``kp``: ``[B, T + 1, 25, K]`` in the reference's row order (p h n m q w v u), i.e. ``traj[:, :, :, key_points]``."""
    r = np.asarray(records).transpose(1, 0, 3, 2)  # [B, T + 1, KR_SLOTS, K]
    return np.ascontiguousarray(np.concatenate([r[:, :, 12:25], r[:, :, 0:12]], axis=2))


SCORE_METRICS = ("dtw", "fastdtw")


def _score_metric(score):
    """``(metric, radius)`` of a ``score`` dictionary: ``"dtw"`` (default; the exact distance, the radius is not used) or
    ``"fastdtw"`` with ``radius`` 1 .. 8 (default 1, the reference's).  Host-side validation only."""
    metric = score.get("metric", "dtw")
    if metric not in SCORE_METRICS:
        raise kn.KrError(f'simulate_batch: score metric must be "dtw" or "fastdtw"; got {metric!r}')
    radius = score.get("radius", 1)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= kn.KR_FASTDTW_MAX_RADIUS:
        raise kn.KrError(f"simulate_batch: score radius must be an integer 1 .. {kn.KR_FASTDTW_MAX_RADIUS}; got {radius!r}")
    return metric, int(radius)


def _score_reference(robot, score, B, T, tip_only):
    """``(reference[R, Tr, >=7, N], point)`` of ``simulate_batch(..., score=...)``, R = 1 or B; host-side validation only
    (no device call), ``metric`` and ``radius`` included (``_score_metric`` returns them)."""
    if tip_only:
        raise kn.KrError("simulate_batch: score needs the state history (tip_only=True keeps three states)")
    if not isinstance(score, dict) or "reference" not in score:
        raise kn.KrError('simulate_batch: score must be {"reference": array[, "point": grid point][, "metric": "dtw" | "fastdtw"]'
                         '[, "radius": 1 .. 8]}')
    metric, _ = _score_metric(score)
    ref = np.asarray(score["reference"], dtype=np.float64)
    N = int(robot.N)
    shared = ref.ndim == 3
    if ref.ndim not in (3, 4):
        raise kn.KrError(f"simulate_batch: score reference must be [Tr, >=7, N] or [B, Tr, >=7, N]; got shape {ref.shape}")
    if shared:
        ref = ref[None]
    R, Tr, rows, n = ref.shape
    if n != N:
        raise kn.KrError(f"simulate_batch: score reference has {n} grid points, the robot {N}")
    if rows < 7:
        raise kn.KrError(f"simulate_batch: score reference has {rows} rows, positions and quaternions need 7")
    if not shared and R != B:
        raise kn.KrError(f"simulate_batch: score reference holds {R} rods, ctl {B}")
    if Tr < 1 or Tr > T + 1:
        raise kn.KrError(f"simulate_batch: score reference has {Tr} states, the run 1 .. {T + 1}")
    if metric == "fastdtw" and Tr > kn.KR_FASTDTW_MAX_LEN:  # (refused here, not after the run)
        raise kn.KrError(f"simulate_batch: score metric fastdtw serves at most {kn.KR_FASTDTW_MAX_LEN} states, the reference has {Tr}")
    point = score.get("point", None)
    point = N - 1 if point is None else int(point)
    if not -N <= point < N:
        raise kn.KrError(f"simulate_batch: score point {point} outside the rod's {N} grid points")
    return ref, point % N


def simulate_batch(robot, ctl, dtype="f64", scheme="euler", return_states=True, tol=0.0, maxit=0, tip_only=False,
                   robots=None, per_robot_nn=False, score=None, tip_loads=None, check_finite=True, base_motion=None,
                   key_points=None):
    """B rods, each with its own tension history.

    robots: None = B copies of ``robot``; otherwise a sequence of B ``CosseratRod`` objects, each prepared the
    reference's way (attributes, ``setup_robot(r, mod)``, ``compute_intermediate_terms()``): rod b runs with the
    parameters of ``robots[b]`` - the reference's eight model-mismatch variants (knode.py:6-53) in one launch.
    ``robot`` stays the carrier of N, del_t, the MLP and the device handle; N, del_t and nn_input_history must agree.

    per_robot_nn (needs ``robots``): rod b also runs with the NETWORK ``robots[b]`` carries (``nn_model`` /
    ``param_ls``) - the reference loads every model variant's own trained network before it simulates
    (physics_multitrain.py:181-199).  Robots that carry the same network share one upload; the result gains
    ``net_of_rod`` int[B] and ``n_networks``.  All networks must have one shape; the carrier's own MLP is not used.

    ctl: array-like [B, T, 4].  Returns a dict with
      ``tip``    float[B, T, 3]  tip position after each solved step,
      ``status`` int32[B, T]     0 converged / 1 iteration cap / 2 non-finite,
      ``traj``   float[B, T+1, 25, N] (reference row order, entry 0 = initial state) unless ``tip_only``.
    All T steps are solved (no off-by-one drop here).

    score: ``{"reference": ref, "point": p}`` scores the run on the device before anything is copied (what
    physics_multitrain.py:213-222 does on the host, one rod at a time): ref is [Tr, >=7, N] (one reference for all rods)
    or [B, Tr, >=7, N], Tr <= T + 1; states 0 .. Tr-1 are compared.  The result gains ``dtw`` float64[B], the exact DTW
    distance (L1) of the path of grid point p (default N - 1, the tip - the reference's literal 9 at its N = 10) to the
    reference's, and ``mse`` float64[B], the position + zyx-Euler MSE x 1000 (``krod_eval.dtw_distance`` /
    ``pos_euler_mse``).  With ``return_states=False`` no trajectory leaves the device.
    ``"metric": "fastdtw"`` (and ``"radius"``, 1 .. 8, default 1) makes ``dtw`` the FastDTW distance instead - the number
    the reference's ``fastdtw(...)[0]`` prints, ``krod_eval.fastdtw_distance`` bit for bit (``kr_fastdtw_batch``); the
    default ``"dtw"`` is the exact distance, as before.  ``dtw_metric`` in the result names the metric used.

    tip_loads: a tip wrench that varies in time, [B, T, 6] or [T, 6] (shared by all rods): rod b solves step t with
    F_tip, M_tip = tip_loads[b, t, :3], tip_loads[b, t, 3:] - the reference with ``robot.F_tip`` / ``robot.M_tip``
    assigned before that solve.  The values replace the robot's own wrench; with ``robots=`` row b keeps everything else.
    Composes with ``score`` and ``tip_only``; not served with ``per_robot_nn`` (``simulate_bank`` serves it).

    base_motion: a base that moves in time, [B, T, 13] or [T, 13] (shared by all rods), columns ``p0 (3) h0 (4) q0 (3)
    w0 (3)``: rod b solves step t with that base state - the reference with ``robot.p0 / h0 / q0 / w0`` assigned before
    that solve (a platform, a carriage, the wrist of an arm).  The values replace the robot's own; ``h0`` is not
    normalised; record 0 of state t + 1 holds them exactly.  The caller supplies consistent ``q0`` / ``w0``.  Composes
    with ``robots``, ``tip_loads`` (without it every rod keeps its own ``F_tip`` / ``M_tip``), ``score`` and ``tip_only``;
    not served with ``per_robot_nn`` (``simulate_bank`` serves it).

    key_points: a list of 1 .. 16 grid points (a negative index counts from the tip; sorted and de-duplicated here): the
    result gains ``kp`` float[B, T+1, 25, K], the states at those points in the reference's row order, entry 0 the initial
    state - ``traj[:, :, :, key_points]`` wherever both exist - and ``key_points`` int32[K], the order used.  With
    ``tip_only=True`` this is the way to the states at a few points of a long run of a large batch: the full history is
    never stored.  Composes with ``robots``, ``tip_loads``, ``base_motion`` (without them the boundary is each rod's own, on
    every step) and ``tip_only``; not served with ``per_robot_nn`` (per-rod networks with ``key_points`` / ``base_motion`` /
    ``tip_loads``: ``simulate_bank``).  With ``key_points``, ``score`` is accepted with
    ``tip_only=True``: ``dtw`` is the DTW of the path of ``score["point"]``, which must then be a key point, and
    ``mse_kp`` the pose MSE over the K key points against the reference at those points (``mse``, the all-points quantity,
    is there only when the full history is).

    check_finite: True (default) refuses ``tip_loads`` / ``base_motion`` that are not finite (and a zero ``h0``) before
    anything touches the device; False hands them to the library, for which they are ordinary input (domain randomisation,
    a diverging row of a sweep).

    Failed steps (knode_rod.h): a rod whose inputs stop being finite at step t0 reports ``status`` 2 at t0; the call returns
    normally and every other rod's outputs are bit for bit those of the batch without the failure.  Where the value enters
    the sweeps (a NaN tension or rod parameter) the rod's states, tips, ``dtw`` and ``mse`` are NaN from there on and every
    later step reports a nonzero status.  A NaN tip wrench (``tip_loads``, ``F_tip`` / ``M_tip``) enters the tip condition
    only: states and scores stay finite and later steps may report 0 again - ``status`` 2 at t0 is the only mark.  A NaN
    base value (``base_motion``) enters the sweeps like a NaN tension."""
    loads = base = kp_idx = None
    # (everything below is validated on the host before anything touches the device)
    per_step = (("key_points", key_points, "key-point records have"), ("base_motion", base_motion, "per-step boundary data has"),
                ("tip_loads", tip_loads, "per-step tip loads have"))
    for name, value, what in per_step:
        if value is not None and per_robot_nn:
            raise kn.KrError(f"simulate_batch: {name} with per_robot_nn=True is not served here ({what} their network-bank form in "
                             "knode.simulate_bank)")
    if score is not None or any(value is not None for _, value, _ in per_step):
        ctl_shape = np.asarray(ctl).shape
        if len(ctl_shape) != 3:
            raise kn.KrError(f"simulate_batch: ctl must be [B, T, 4]; got {ctl_shape}")
    if key_points is not None:
        kp_idx = _key_points(key_points, int(robot.N))
    if base_motion is not None:
        base = _base_motion(base_motion, int(ctl_shape[0]), int(ctl_shape[1]), check_finite)
    if tip_loads is not None:
        loads = _tip_loads(tip_loads, int(ctl_shape[0]), int(ctl_shape[1]), check_finite)
    if score is not None:
        score_ref, score_point = _score_reference(robot, score, int(ctl_shape[0]), int(ctl_shape[1]), tip_only and kp_idx is None)
        score_metric, score_radius = _score_metric(score)
        if tip_only and score_point not in kp_idx.tolist():
            raise kn.KrError(f"simulate_batch: score point {score_point} is not one of the key points {kp_idx.tolist()} "
                             "(tip_only=True keeps the states at the key points only)")
    rows = None
    networks = net_of_rod = None
    if robots is not None:  # (validated on the host before anything touches the device)
        robots = list(robots)
        rows = _robots_rows(robot, robots, int(np.asarray(ctl).shape[0]))
    elif loads is not None:  # only the loads vary: a table of identical rows
        rows = _robots_rows(robot, [robot] * loads.shape[0], loads.shape[0])
    elif base is not None:  # only the base varies
        rows = _robots_rows(robot, [robot] * base.shape[0], base.shape[0])
    elif kp_idx is not None:  # nothing varies: a table of identical rows
        n_rods = int(np.asarray(ctl).shape[0])
        rows = _robots_rows(robot, [robot] * n_rods, n_rods)
    if kp_idx is not None and base is None:  # a key-point call is a boundary call: each rod's own base on every step
        base = _base_of_rows(rows, int(np.asarray(ctl).shape[1]))
    bnd = _boundary(base, loads, rows) if base is not None else None  # (tip_loads alone stays a loads call)
    if per_robot_nn:
        if robots is None:
            raise kn.KrError("simulate_batch: per_robot_nn needs robots=[...]")
        networks, net_of_rod = _robots_networks(robot, robots)
    if score is None:
        score_ref = score_point = None
        score_metric, score_radius = "dtw", 1
    return _run_batch(robot._native(), ctl, dtype, scheme, return_states, tol, maxit, tip_only, robot._use_nn, rows, networks, None,
                      net_of_rod, loads, bnd, kp_idx, score_ref, score_point, score_metric=score_metric, score_radius=score_radius)


def _run_batch(h, ctl, dtype, scheme, return_states, tol, maxit, tip_only, use_nn, rows, networks, bank, net_of_rod, loads, bnd,
               kp_idx, score_ref, score_point, scores_only=False, score_metric="dtw", score_radius=1):
    """The device half of ``simulate_batch`` / ``simulate_bank`` on handle ``h``, everything validated by the caller:
    ``rows`` the table's, ``networks`` of a bank made and closed here or ``bank`` a live one of the caller's, ``loads`` /
    ``bnd`` / ``kp_idx`` / ``score_ref`` as the caller's helpers return them (None: without); ``score_metric`` /
    ``score_radius`` as ``_score_metric`` returns them."""
    import torch
    table = h.param_table(rows) if rows is not None else None
    own_bank = networks is not None
    if own_bank:
        bank = h.mlp_bank(networks)
    dev = f"cuda:{h.device}"
    tdt = torch.float64 if dtype in ("f64", torch.float64, np.float64) else torch.float32
    ctl_t = torch.as_tensor(np.asarray(ctl, dtype=np.float64), device=dev).to(tdt).contiguous()
    B, T = ctl_t.shape[0], ctl_t.shape[1]
    n_slots = 3 if tip_only else T + 1
    states = h.new_state(B, tdt, n_slots=n_slots)
    h.init_straight(states[0], table=table)
    G = torch.zeros((B, 6), dtype=tdt, device=dev)  # knode.py:67
    tip = torch.empty((B, T, 3), dtype=tdt, device=dev)
    status = torch.zeros((B, T), dtype=torch.int32, device=dev)
    loads_t = torch.as_tensor(loads, device=dev).to(tdt).contiguous() if loads is not None and bnd is None else None
    bnd_t = torch.as_tensor(bnd, device=dev).to(tdt).contiguous() if bnd is not None else None
    kp_all = None
    if kp_idx is not None:  # [T + 1, B, K, KR_SLOTS]: entry 0 from the initial state (a ring overwrites its slot), the rest by the run
        kp_all = torch.empty((T + 1, B, len(kp_idx), kn.KR_SLOTS), dtype=tdt, device=dev)
        kp_all[0] = states[0][:, torch.as_tensor(kp_idx.astype(np.int64), device=dev)]
    h.simulate(ctl_t, states, G, ring=tip_only, tip=tip, status=status,
               scheme=kn.KR_RK4 if scheme == "rk4" else kn.KR_EULER, tol=tol, maxit=maxit, use_nn=use_nn,
               table=table, bank=bank, net_of_rod=net_of_rod, loads=loads_t, bnd=bnd_t,
               **({"key_points": kp_idx, "kp": kp_all[1:]} if kp_idx is not None else {}))
    score = score_ref
    if score is not None:  # queued behind the run; the copies below wait for both
        Tr = score_ref.shape[1]
        ref_states = h.pack_poses(score_ref, tdt)  # [Tr, 1 or B, N, KR_SLOTS], packed once
        ref_path = ref_states[:, :, score_point, 12:15].permute(1, 0, 2)
        if tip_only:  # the path of the score point from the key-point records (the ring holds three states)
            path = kp_all[:Tr, :, kp_idx.tolist().index(score_point), 12:15].permute(1, 0, 2)
        else:
            path = states[:Tr, :, score_point, 12:15].permute(1, 0, 2)
        ref_path = ref_path[0] if ref_path.shape[0] == 1 else ref_path
        if score_metric == "fastdtw":  # (no fall-back: the metric asked for, or the library's error)
            score_dtw = h.fastdtw(path, ref_path, radius=score_radius)
        else:
            score_dtw = h.dtw(path, ref_path)
        score_mse = None if tip_only else h.pose_mse(states[:Tr], ref_states)[0]
        if kp_idx is not None:
            ref_kp = ref_states[:, :, torch.as_tensor(kp_idx.astype(np.int64), device=dev)].contiguous()
            score_mse_kp, _ = h.pose_mse_points(kp_all[:Tr], ref_kp)
    if scores_only:  # (evaluate_bank: nothing but the scores leaves the device; .cpu() waits for the run)
        out = {"dtw": score_dtw.cpu().numpy(), "dtw_metric": score_metric, "mse_kp": score_mse_kp.cpu().numpy()}
        table.close()
        if own_bank:
            bank.close()
        return out
    out = {"tip": tip.cpu().numpy(), "status": status.cpu().numpy(), "G": G.cpu().numpy()}  # (.cpu() waits for the run)
    if table is not None:
        table.close()
    if bank is not None:
        out["net_of_rod"] = np.asarray(net_of_rod, dtype=np.int32)
        out["n_networks"] = bank.K
        if own_bank:
            bank.close()
    if score is not None:
        out["dtw"] = score_dtw.cpu().numpy()
        out["dtw_metric"] = score_metric
        if score_mse is not None:
            out["mse"] = score_mse.cpu().numpy()
        if kp_idx is not None:
            out["mse_kp"] = score_mse_kp.cpu().numpy()
    if kp_idx is not None:
        out["kp"] = _kp_rows(kp_all.cpu().numpy())
        out["key_points"] = kp_idx.copy()
    if not tip_only and return_states:
        N = h.N
        traj = torch.empty((B, T + 1, 25, N), dtype=tdt, device=dev)
        for t in range(T + 1):
            y, z = h.unpack(states[t])
            traj[:, t, :19] = y
            traj[:, t, 19:] = z
        out["traj"] = traj.cpu().numpy()
    return out


def _bank_call_inputs(robot, robots, ctl, tip_only, score, tip_loads, base_motion, key_points, check_finite):
    """Everything ``simulate_bank`` validates and prepares on the host, before the first device or library call that
    needs a GPU: ``(rows, networks, net_of_rod, bnd, kp_idx, score_ref, score_point)``."""
    ctl_shape = np.asarray(ctl).shape
    if len(ctl_shape) != 3:
        raise kn.KrError(f"simulate_batch: ctl must be [B, T, 4]; got {ctl_shape}")
    B, T = int(ctl_shape[0]), int(ctl_shape[1])
    if robots is None:
        raise kn.KrError("simulate_batch: simulate_bank needs robots=[...], one per rod (rod b runs with the network robots[b] carries)")
    kp_idx = _key_points(key_points, int(robot.N)) if key_points is not None else None
    base = _base_motion(base_motion, B, T, check_finite) if base_motion is not None else None
    loads = _tip_loads(tip_loads, B, T, check_finite) if tip_loads is not None else None
    score_ref = score_point = None
    if score is not None:
        score_ref, score_point = _score_reference(robot, score, B, T, tip_only and kp_idx is None)
        if tip_only and score_point not in kp_idx.tolist():
            raise kn.KrError(f"simulate_batch: score point {score_point} is not one of the key points {kp_idx.tolist()} "
                             "(tip_only=True keeps the states at the key points only)")
    robots = list(robots)
    rows = _robots_rows(robot, robots, B)
    networks, net_of_rod = _robots_networks(robot, robots, zero_ok=True)
    if base is None:  # a bank call with per-step data is a boundary call: each rod's own base on every step
        base = _base_of_rows(rows, T)
    return rows, networks, net_of_rod, _boundary(base, loads, rows), kp_idx, score_ref, score_point


def _named(fn, *args):
    """``fn(*args)`` with the messages of the helpers it shares with ``simulate_batch`` naming ``simulate_bank``."""
    try:
        return fn(*args)
    except kn.KrError as e:
        err = kn.KrError(str(e).replace("simulate_batch:", "simulate_bank:"))
        if hasattr(e, "code"):
            err.code = e.code
        raise err from None


def simulate_bank(robot, robots, ctl, dtype="f64", tol=0.0, maxit=0, tip_only=False, return_states=True, score=None,
                  tip_loads=None, base_motion=None, key_points=None, check_finite=True):
    """``simulate_batch(robot, ctl, robots=robots, per_robot_nn=True)`` that also takes the per-step arguments: B rods in
    ONE launch, rod b with the parameters of ``robots[b]`` AND the network ``robots[b]`` carries, under ``tip_loads`` /
    ``base_motion`` and with ``key_points`` records - the evaluation half of the reference's experiment
    (physics_multitrain.py:180-233: every trained network rolled out and scored at key points against a recorded run).

    Every argument means what it means in ``simulate_batch``; the result is laid out the same way (``tip``, ``status``,
    ``G``, ``net_of_rod``, ``n_networks``, ``traj`` unless ``tip_only`` or ``return_states=False``, ``kp`` / ``key_points``
    with key points, ``dtw`` / ``mse`` / ``mse_kp`` with ``score``).  A robot with ``nn_path is None`` takes a zero network
    of the others' shape: the reference's network-free "baseline" rows ride in the same launch.  Without ``base_motion`` /
    ``tip_loads`` the boundary is each rod's own on every step.  With ``tip_only=True``, ``score`` needs ``key_points`` and
    a score point among them.  Everything is validated on the host before the first device or library call.  Euler only,
    one network shape per call, 9 <= N <= 128 (what ``kr_simulate_batch_bank_keypoints`` serves)."""
    rows, networks, net_of_rod, bnd, kp_idx, score_ref, score_point = _named(
        _bank_call_inputs, robot, robots, ctl, tip_only, score, tip_loads, base_motion, key_points, check_finite)
    score_metric, score_radius = _score_metric(score) if score is not None else ("dtw", 1)  # (validated above)
    return _run_batch(robot._native(), ctl, dtype, "euler", return_states, tol, maxit, tip_only, True, rows, networks, None, net_of_rod,
                      None, bnd, kp_idx, score_ref, score_point, score_metric=score_metric, score_radius=score_radius)


def simulate(robot, ctl, robot_reference=None):
    """Reference knode.py:55-102.  The time loop is one ``kr_simulate_batch`` call, the ``[y; z; yh; zh]`` rows of all
    steps one ``kr_state_unpack50`` launch.  A step whose shooting solve did not converge raises a ``RuntimeWarning``
    (the reference's ``fsolve`` does the same through SciPy and carries on)."""
    import warnings
    import torch
    if robot_reference is None:
        robot_reference = robot
    ctl = np.asarray([np.asarray(c, dtype=np.float64) for c in ctl], dtype=np.float64).reshape(-1, 4)
    T = ctl.shape[0]
    N = int(robot_reference.N)
    if int(robot.N) != N:
        raise kn.KrError("robot and robot_reference must share N")
    if T == 0:  # np.array([initial])[:-1] in the reference
        return np.empty((0, 50, N), dtype=np.float64)
    # side effect of the reference's loop (knode.py:71): the robot is left holding the LAST control, including the
    # one whose solve is dropped - a following robot.getResidualEuler(...) by the caller reads it
    robot.tendon_tensions = ctl[-1].copy()
    h = robot._native()
    dev = f"cuda:{robot.device}"
    states = h.new_state(1, torch.float64, n_slots=max(T, 2))
    # the initial rod takes its length from robot_reference (knode.py:59)
    if robot_reference is not robot:
        robot_reference._native().init_straight(states[0])
    else:
        h.init_straight(states[0])
    status = None
    if T > 1:  # the T-th solve is dropped by the reference (knode.py:102), so it is not run
        G = torch.zeros((1, 6), dtype=torch.float64, device=dev)
        status = torch.zeros((1, T - 1), dtype=torch.int32, device=dev)
        ctl_t = torch.as_tensor(ctl[: T - 1].reshape(1, T - 1, 4), device=dev).contiguous()
        h.simulate(ctl_t, states, G, ring=False, use_nn=robot._use_nn, status=status)
    # entry t = [state t; c1 * state t-1 + c2 * state t-2] (knode.py:74-75,96): the T entries as one batch of T "rods"
    st = states[:T, 0]
    m1 = torch.cat([st[:1], st[: T - 1]])
    m2 = torch.cat([st[:1], st[:1], st[: T - 2]]) if T > 1 else st[:1]
    out = h.unpack50(st.contiguous(), m1.contiguous(), m2.contiguous())
    out[0, 25:] = out[0, :25]  # knode.py:68: entry 0 is vstack([y, z, y, z])
    res = out.cpu().numpy()
    if status is not None:
        bad = np.flatnonzero(status.cpu().numpy()[0])
        if bad.size:
            warnings.warn(f"shooting solve did not converge at step(s) {bad[:8].tolist()}"
                          f"{' ...' if bad.size > 8 else ''} of {T - 1}", RuntimeWarning)
    return res
