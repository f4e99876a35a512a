"""Trajectory files and evaluation metrics of the reference's drivers.

* ``save_trajectory`` / ``load_trajectory``: the ``.npy`` dictionary ``{"traj": [T, 50, N], "controls": [T-1, 4]}``
  of ``knode_cosserat_realworld/simulate.py:97-100`` (read back with ``np.load(..., allow_pickle=True).item()``,
  cosserat_ode.py:265) and the evaluation record of ``physics_multitrain.py:201-205``.
* ``fastdtw_distance``: the tip-trajectory metric of ``physics_train.py:159-161`` and ``physics_multitrain.py:211``.
  The reference calls ``fastdtw(a, b)[0]`` of the third-party package ``fastdtw`` (slaypni/fastdtw; no version is
  pinned by the reference and the package is absent from this build container): radius 1, L1 point distance for
  vector samples.  This is a restatement of the published algorithm (S. Salvador, P. Chan, "FastDTW: Toward accurate
  dynamic time warping in linear time and space", Intelligent Data Analysis 11(5), 2007): halve both series by
  averaging adjacent samples until one is shorter than radius + 2, solve exactly there, and refine the warp path on
  every finer level inside the projected path widened by the radius.  Ties between predecessors are broken in the
  order (i-1, j), (i, j-1), (i-1, j-1) - the order of the package's ``min`` - which matters for the window of the next
  level.  **Parity with the package is unpinned** (nothing to run it against); ``dtw_distance`` is the exact DTW
  with the same point distance, a lower bound of it (equal whenever the coarse path contains the optimal one).
  ``fastdtw_path`` returns the warp path with the distance.  These host functions are the normative statement of the
  algorithm for the device kernel (``kr_fastdtw_batch``), which reproduces them bit for bit.
* ``pos_euler_mse``: ``physics_multitrain.py:213-222`` (position + zyx Euler angles, x 1000).
* ``euler_zyx``, ``dtw_distance_batch``, ``fastdtw_distance_batch``, ``pos_euler_mse_batch``, ``evaluate_batch``,
  ``evaluate_bank``: the same metrics for B rods at once on the MI355X (``kr_dtw_batch``, ``kr_fastdtw_batch``,
  ``kr_pose_mse_batch``).  ``metric="dtw"`` (default) scores with the exact DTW, ``metric="fastdtw"`` with FastDTW - the
  figure the reference prints - whose warp path is traced back on every level on the device.  ``evaluate_batch`` is the
  inner loop of ``physics_multitrain.py:196-222``; nothing but two doubles per rod leaves the device.
* ``evaluate``: the closed-loop rollout with live weights of ``physics_train.py:136-167``; the rollout is
  ``knode.simulate`` on the MI355X with the MLP inside the shooting sweeps.
"""
from __future__ import annotations

import numpy as np


def save_trajectory(path, traj, controls):
    np.save(path, {"traj": np.asarray(traj, dtype=np.float64), "controls": np.asarray(controls, dtype=np.float64)})


def load_trajectory(path):
    d = np.load(path, allow_pickle=True).item()
    return d["traj"], d["controls"]


def save_eval_record(path, tensions, reference, predicted):
    np.save(path, {"tensions": tensions, "reference": reference, "predicted": predicted})


def dtw_distance(a, b, p=1):
    """Exact dynamic-time-warping distance between the sample sequences a[Ta, d] and b[Tb, d] with the
    p-norm as point distance (1-D inputs: absolute difference).  O(Ta*Tb) work, vectorised along the
    anti-diagonals of the cost table."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if b.ndim == 1:
        b = b[:, None]
    Ta, Tb = len(a), len(b)
    if Ta == 0 or Tb == 0:
        raise ValueError("empty sequence")
    diff = np.abs(a[:, None, :] - b[None, :, :])
    cost = diff.sum(-1) if p == 1 else (diff ** p).sum(-1) ** (1.0 / p)
    D = np.full((Ta + 1, Tb + 1), np.inf)
    D[0, 0] = 0.0
    for k in range(2, Ta + Tb + 1):  # cells (i, j), 1-based, with i + j = k
        i = np.arange(max(1, k - Tb), min(Ta, k - 1) + 1)
        j = k - i
        D[i, j] = cost[i - 1, j - 1] + np.minimum(np.minimum(D[i - 1, j], D[i, j - 1]), D[i - 1, j - 1])
    return float(D[Ta, Tb])


SOFTDTW_COSTS = {"l1": 0, "sq": 1}  # the point costs of the soft form -> the `cost` argument of kr_softdtw_batch


def _softdtw_args(a, b, gamma, cost):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != 3 or b.shape[1] != 3 or len(a) < 1 or len(b) < 1:
        raise ValueError(f"softdtw: sequences must be [Ta, 3] and [Tb, 3] with Ta, Tb >= 1; got {a.shape} and {b.shape}")
    gamma = float(gamma)
    if not (np.isfinite(gamma) and gamma > 0.0):
        raise ValueError(f"softdtw: gamma must be finite and > 0; got {gamma}")
    if cost not in SOFTDTW_COSTS:
        raise ValueError(f"softdtw: cost must be one of {sorted(SOFTDTW_COSTS)}; got {cost!r}")
    return a, b, gamma


def _softdtw_forward(a, b, gamma, cost):
    """(d[Ta, Tb, 3], c padded to [Ta + 2, Tb + 2] with zeros, R[Ta + 2, Tb + 2]) of the forward sweep, 1-based cells."""
    Ta, Tb = len(a), len(b)
    d = a[:, None, :] - b[None, :, :]
    c = np.zeros((Ta + 2, Tb + 2))
    if cost == "l1":
        c[1:Ta + 1, 1:Tb + 1] = (np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])
    else:
        c[1:Ta + 1, 1:Tb + 1] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    R = np.full((Ta + 2, Tb + 2), np.inf)
    R[0, 0] = 0.0
    for k in range(2, Ta + Tb + 1):  # cells (i, j), 1-based, with i + j = k
        i = np.arange(max(1, k - Tb), min(Ta, k - 1) + 1)
        j = k - i
        up, left, diag = R[i - 1, j], R[i, j - 1], R[i - 1, j - 1]
        m = np.minimum(np.minimum(up, left), diag)  # finite: every cell of the table has a finite predecessor
        s = (np.exp((m - up) / gamma) + np.exp((m - left) / gamma)) + np.exp((m - diag) / gamma)  # exp(-inf) = 0
        R[i, j] = c[i, j] + (m - gamma * np.log(s))
    return d, c, R


def softdtw_distance(a, b, gamma, cost="l1"):
    """Soft-DTW (Cuturi & Blondel 2017) of the paths a[Ta, 3], b[Tb, 3]: DTW's recurrence with ``min`` replaced by
    ``softmin(r) = m - gamma log(sum_k exp((m - r_k) / gamma))``, m = min r, over (up, left, diagonal), an infinite entry
    contributing 0.  ``cost``: ``"l1"``, the metric's own point distance ``(|dx| + |dy|) + |dz|``, or ``"sq"``,
    ``(dx dx + dy dy) + dz dz``.  fp64; the statement ``kr_softdtw_batch`` is held to (include/knode_rod.h).  As gamma -> 0
    the value tends to ``dtw_distance(a, b)`` from below, by at most ``gamma ln 3`` per cell of a warp path."""
    a, b, gamma = _softdtw_args(a, b, gamma, cost)
    return float(_softdtw_forward(a, b, gamma, cost)[2][len(a), len(b)])


def softdtw_grad(a, b, gamma, cost="l1"):
    """``(value, g_a[Ta, 3])``: ``softdtw_distance`` and its gradient with respect to a, by the backward sweep over the
    table: E(Ta + 1, Tb + 1) = 1, R(Ta + 1, Tb + 1) = R(Ta, Tb), the rest of row Ta + 1 and column Tb + 1 R = -inf, E = 0,
    c = 0; ``E(i, j) = sum over (p, q) in ((i + 1, j), (i, j + 1), (i + 1, j + 1)) of E(p, q) exp((R(p, q) - R(i, j) -
    c(p, q)) / gamma)`` (every exponent <= 0); ``g_a[i] = sum_j E(i, j) dc(i, j)/da_i`` in increasing j, with dc/da =
    sign(a - b) (sign(0) = 0) for ``"l1"`` and 2 (a - b) for ``"sq"``."""
    a, b, gamma = _softdtw_args(a, b, gamma, cost)
    d, R, E = _softdtw_tables(a, b, gamma, cost)
    dc = np.sign(d) if cost == "l1" else 2.0 * d
    g = np.zeros((len(a), 3))
    for j in range(len(b)):  # (increasing j)
        g += E[1:-1, j + 1, None] * dc[:, j, :]
    return float(R[len(a), len(b)]), g


def _softdtw_tables(a, b, gamma, cost):
    """(d[Ta, Tb, 3] = a_i - b_j, R[Ta + 2, Tb + 2], E[Ta + 2, Tb + 2]) of both sweeps, 1-based cells, borders as defined"""
    Ta, Tb = len(a), len(b)
    d, c, R = _softdtw_forward(a, b, gamma, cost)
    R[Ta + 1, :] = -np.inf
    R[:, Tb + 1] = -np.inf
    R[Ta + 1, Tb + 1] = R[Ta, Tb]
    E = np.zeros((Ta + 2, Tb + 2))
    E[Ta + 1, Tb + 1] = 1.0
    for k in range(Ta + Tb, 1, -1):
        i = np.arange(max(1, k - Tb), min(Ta, k - 1) + 1)
        j = k - i
        r = R[i, j]
        E[i, j] = (E[i + 1, j] * np.exp((R[i + 1, j] - r - c[i + 1, j]) / gamma)
                   + E[i, j + 1] * np.exp((R[i, j + 1] - r - c[i, j + 1]) / gamma)) \
            + E[i + 1, j + 1] * np.exp((R[i + 1, j + 1] - r - c[i + 1, j + 1]) / gamma)
    return d, R, E


def _l1(a, b):
    return float(np.abs(a - b).sum())


def _dtw_window(x, y, window):
    """DTW restricted to the cells of `window` (sorted by row, then column); returns (distance, path)."""
    inf = float("inf")
    D = {(0, 0): (0.0, 0, 0)}
    get = D.get
    for i, j in window:
        i1, j1 = i + 1, j + 1
        d = _l1(x[i], y[j])
        a = get((i1 - 1, j1), (inf,))[0]
        b = get((i1, j1 - 1), (inf,))[0]
        c = get((i1 - 1, j1 - 1), (inf,))[0]
        # first minimum in the order up, left, diagonal
        if a <= b and a <= c:
            D[i1, j1] = (a + d, i1 - 1, j1)
        elif b <= c:
            D[i1, j1] = (b + d, i1, j1 - 1)
        else:
            D[i1, j1] = (c + d, i1 - 1, j1 - 1)
    path = []
    i, j = len(x), len(y)
    while not (i == 0 and j == 0):
        path.append((i - 1, j - 1))
        _, i, j = D[i, j]
    path.reverse()
    return D[len(x), len(y)][0], path


def _expand_window(path, len_x, len_y, radius):
    cells = set(path)
    for i, j in path:
        for a in range(-radius, radius + 1):
            for b in range(-radius, radius + 1):
                cells.add((i + a, j + b))
    fine = set()
    for i, j in cells:
        fine.update(((2 * i, 2 * j), (2 * i, 2 * j + 1), (2 * i + 1, 2 * j), (2 * i + 1, 2 * j + 1)))
    window = []
    start_j = 0
    for i in range(len_x):
        new_start = None
        for j in range(start_j, len_y):
            if (i, j) in fine:
                window.append((i, j))
                if new_start is None:
                    new_start = j
            elif new_start is not None:
                break
        start_j = new_start
    return window


def _fastdtw(x, y, radius):
    if len(x) < radius + 2 or len(y) < radius + 2:
        return _dtw_window(x, y, [(i, j) for i in range(len(x)) for j in range(len(y))])
    half = lambda s: [(s[i] + s[i + 1]) / 2 for i in range(0, len(s) - len(s) % 2, 2)]
    _, path = _fastdtw(half(x), half(y), radius)
    return _dtw_window(x, y, _expand_window(path, len(x), len(y), radius))


def fastdtw_distance(a, b, radius=1):
    """FastDTW (see the module docstring) between the sample sequences a[Ta, d] and b[Tb, d], L1 point distance."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if b.ndim == 1:
        b = b[:, None]
    if len(a) == 0 or len(b) == 0:
        raise ValueError("empty sequence")
    return float(_fastdtw([r for r in a], [r for r in b], int(radius))[0])


def fastdtw_path(a, b, radius=1):
    """``(distance, path)`` of FastDTW between a[Ta, d] and b[Tb, d]: ``fastdtw_distance`` together with the level-0 warp
    path, a list of (i, j) pairs from (0, 0) to (Ta - 1, Tb - 1) - the pair the package's ``fastdtw(a, b)`` returns."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if b.ndim == 1:
        b = b[:, None]
    if len(a) == 0 or len(b) == 0:
        raise ValueError("empty sequence")
    dist, path = _fastdtw([r for r in a], [r for r in b], int(radius))
    return float(dist), [(int(i), int(j)) for i, j in path]


def pos_euler_mse(trajectory, reference):
    """physics_multitrain.py:213-222: mean of the squared position errors and the squared zyx-Euler-angle
    errors over all grid points and steps, times 1000.  trajectory, reference: [T, >=7, N]."""
    from scipy.spatial.transform import Rotation
    trajectory = np.asarray(trajectory)
    reference = np.asarray(reference)
    se_pos = (trajectory[:, :3] - reference[:, :3]).reshape((-1, 3)) ** 2
    eq = trajectory[:, 3:7].transpose((0, 2, 1)).reshape((-1, 4))
    rq = reference[:, 3:7].transpose((0, 2, 1)).reshape((-1, 4))
    ee = Rotation.from_quat(eq, scalar_first=True).as_euler("zyx")
    re = Rotation.from_quat(rq, scalar_first=True).as_euler("zyx")
    return float(np.mean(np.concatenate([(ee - re) ** 2, se_pos])) * 1000)


def euler_zyx(q):
    """SciPy's ``Rotation.from_quat(q, scalar_first=True).as_euler("zyx")`` (extrinsic) in closed form, q[..., 4] =
    (w, x, y, z), not necessarily unit: the host twin of the device kernel behind ``pos_euler_mse_batch``.  No
    gimbal-lock branch: within ~1e-6 of +-pi/2 in the middle angle SciPy zeroes one angle and warns, this does not."""
    q = np.asarray(q, dtype=np.float64)
    n = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
    w, x, y, z = q[..., 0] / n, q[..., 1] / n, q[..., 2] / n, q[..., 3] / n
    a = np.arctan2(2.0 * (w * z - x * y), 1.0 - 2.0 * (y * y + z * z))
    b = np.arcsin(np.clip(2.0 * (x * z + w * y), -1.0, 1.0))
    c = np.arctan2(2.0 * (w * x - y * z), 1.0 - 2.0 * (x * x + y * y))
    return np.stack([a, b, c], axis=-1)


def _torch_dtype(dtype):
    import torch
    return torch.float64 if dtype in ("f64", torch.float64, np.float64) else torch.float32


def dtw_distance_batch(robot, a, b, dtype="f64"):
    """``dtw_distance(a[r], b[r])`` for every rod r in one launch on the robot's device: a[B, Ta, 3], b[B, Tb, 3] or
    b[Tb, 3] (one path for all rods), host arrays, uploaded as ``dtype`` (the arithmetic is fp64).  Returns float64[B],
    bit-identical to the host function on the same samples."""
    import torch
    dev, tdt = f"cuda:{robot.device}", _torch_dtype(dtype)
    h = robot._native()
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev).to(tdt).contiguous()
    return h.dtw(up(a), up(b)).cpu().numpy()


def fastdtw_distance_batch(robot, a, b, radius=1, dtype="f64", return_path=False):
    """``fastdtw_distance(a[r], b[r], radius)`` for every rod r in one launch on the robot's device (``kr_fastdtw_batch``):
    a[B, Ta, 3], b[B, Tb, 3] or b[Tb, 3] (one path for all rods), host arrays, uploaded as ``dtype`` (the arithmetic is
    fp64).  Returns float64[B], bit-identical to the host function on the same samples (NaN for a rod with a non-finite
    sample); with ``return_path=True`` ``(dist, paths)``, ``paths[r]`` the int32 [len, 2] warp path of rod r
    (``fastdtw_path``; empty for a NaN rod)."""
    import torch
    dev, tdt = f"cuda:{robot.device}", _torch_dtype(dtype)
    h = robot._native()
    up = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev).to(tdt).contiguous()
    if not return_path:
        return h.fastdtw(up(a), up(b), radius=radius).cpu().numpy()
    dist, steps, plen = h.fastdtw(up(a), up(b), radius=radius, path=True)
    steps, plen = steps.cpu().numpy(), plen.cpu().numpy()
    return dist.cpu().numpy(), [steps[r, :plen[r]].copy() for r in range(len(plen))]


def pos_euler_mse_batch(robot, trajectories, reference, dtype="f64"):
    """``pos_euler_mse(trajectories[r], reference)`` for every rod r in one launch: trajectories[B, T, >=7, N],
    reference[T, >=7, N] (shared) or [B, T, >=7, N], N = the robot's.  Returns float64[B]."""
    tdt = _torch_dtype(dtype)
    h = robot._native()
    trajectories = np.asarray(trajectories, dtype=np.float64)
    reference = np.asarray(reference, dtype=np.float64)
    if reference.ndim == 3:
        reference = reference[None]
    mse, _ = h.pose_mse(h.pack_poses(trajectories, tdt), h.pack_poses(reference, tdt))
    return mse.cpu().numpy()


def evaluate_batch(robot, robots, controls, reference, per_robot_nn=False, point=-1, dtype="f64", metric="dtw", radius=1):
    """The inner loop of physics_multitrain.py:196-222 for B rods at once: roll every ``robots[b]`` (None: B copies of
    ``robot``) out over ``controls[b]`` in one ``knode.simulate_batch`` call and score states 0 .. Tr-1 against
    ``reference`` ([Tr, >=7, N] or [B, Tr, >=7, N]) on the device.  Returns ``(dtw[B], mse[B])``: the exact DTW of the
    path of grid point ``point`` (-1: the tip) and the position + Euler MSE x 1000; no trajectory leaves the device.
    ``metric="fastdtw"`` (``radius`` 1 .. 8): the first array is the FastDTW distance, the reference's own figure."""
    from knode import simulate_batch
    out = simulate_batch(robot, controls, dtype=dtype, return_states=False, robots=robots, per_robot_nn=per_robot_nn,
                         score={"reference": reference, "point": point, "metric": metric, "radius": radius})
    return out["dtw"], out["mse"]


def evaluate_bank(robot, robots, controls, reference, key_points, point=-1, dtype="f64", metric="dtw", radius=1):
    """physics_multitrain.py:180-233 for a grid of trained networks in ONE tip-only launch: rod b runs with the parameters and
    the network of ``robots[b]`` (``knode.simulate_bank``) over ``controls[b]`` on a three-state ring, the records of
    ``key_points`` are the only states stored, and states 0 .. Tr-1 are scored on the device against ``reference``
    ([Tr, >=7, N] or [B, Tr, >=7, N]).  Returns ``(dtw[B], mse_kp[B])``: the exact DTW of the path of grid point ``point``
    (-1: the tip; it must be a key point) and the pose MSE x 1000 over the key points.  Nothing but the scores leaves the
    device.  ``metric="fastdtw"`` (``radius`` 1 .. 8): the first array is the FastDTW distance, the reference's own figure."""
    import knode
    import krod_native as kn
    if key_points is None:
        raise kn.KrError("evaluate_bank: key_points is required (a tip-only run keeps the states at the key points only)")
    score = {"reference": reference, "point": point, "metric": metric, "radius": radius}
    rows, networks, net_of_rod, bnd, kp_idx, score_ref, score_point = knode._named(
        knode._bank_call_inputs, robot, robots, controls, True, score, None, None, key_points, True)
    score_metric, score_radius = knode._score_metric(score)
    out = knode._run_batch(robot._native(), controls, dtype, "euler", False, 0.0, 0, True, True, rows, networks, None, net_of_rod, None, bnd,
                           kp_idx, score_ref, score_point, scores_only=True, score_metric=score_metric, score_radius=score_radius)
    return out["dtw"], out["mse_kp"]


def evaluate(robot_eval, torch_robot, controls, reference, eval_len=None, tip_index=-1, exact=False):
    """physics_train.py:136-167: put the current weights of `torch_robot` into the NumPy-side robot,
    roll it out in closed loop over `controls` and score the tip path against `reference[:, :3, tip]` with FastDTW
    (radius 1, what the reference calls; ``exact=True``: the exact DTW).  Returns (dtw, traj[T, 25, N])."""
    from knode import simulate
    if torch_robot is not None:
        nn_model = torch_robot.nn_models
        robot_eval.nn_model = nn_model
        robot_eval.param_ls = [t.detach().cpu().numpy() for _, t in nn_model.state_dict().items()]
        robot_eval.nn_path = "whatever"  # forces the robot to use the MLP (physics_train.py:144)
    controls = np.asarray(controls)
    n = len(controls) if eval_len is None else eval_len
    traj = simulate(robot_eval, controls[:n])[:n, :25]
    metric = dtw_distance if exact else fastdtw_distance
    return metric(traj[:, :3, tip_index], np.asarray(reference)[:n, :3, tip_index]), traj
