"""Device evaluation metrics (kr_dtw_batch, kr_pose_mse_batch, knode.simulate_batch(score=...)) on the MI355X.

The reference of every comparison is the host code the kernels replace: ``krod_eval.dtw_distance`` (exact DTW, L1 point
distance) - BITWISE, the kernel runs the same additions and minima in the same order - and ``krod_eval.pos_euler_mse``
(SciPy's Euler angles), to 1e-10 relative: the library functions are good to a few 1e-16 on angles of order 1, so a
squared difference of size 1e-4 carries about 1e-12 relative; the bound leaves two orders of margin.
Inputs are seeded random walks of step 0.01."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from gpu_helpers import make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(1, 1), (1, 7), (7, 1), (2, 65), (63, 64), (64, 64), (65, 129), (99, 99), (130, 61), (257, 300)]
B5 = 5
SENTINEL = -12345.5
MODS7 = ["noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    return {N: make_robot(None, N)._native() for N in (10, 33)}


def walk(seed, *shape):
    """Random walk of step 0.01 along axis -2 of [..., T, 3]."""
    return np.cumsum(np.random.default_rng(seed).normal(size=shape) * 0.01, axis=-2)


def host_dtw(a, b):
    from krod_eval import dtw_distance
    b = np.broadcast_to(b, (a.shape[0],) + b.shape[-2:])
    return np.array([dtw_distance(a[r], b[r]) for r in range(a.shape[0])])


def dev(torch, x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype or torch.float64).contiguous()


def assert_bitwise(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = got.view(np.uint64) == want.view(np.uint64)
    assert same.all(), f"{label}: rods {np.flatnonzero(~same).tolist()} differ: {got[~same]} vs {want[~same]}"


# ---------------------------------------------------------------------------
# 1. DTW exactness
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Ta,Tb", PAIRS)
def test_dtw_bitwise_against_host(torch_cuda, handles, Ta, Tb):
    torch, h = torch_cuda, handles[10]
    a, b = walk(100 + Ta, B5, Ta, 3), walk(200 + Tb, B5, Tb, 3) + 0.003
    # fp64, a reference per rod
    assert_bitwise(h.dtw(dev(torch, a), dev(torch, b)).cpu().numpy(), host_dtw(a, b), "fp64")
    # one reference shared by all rods (rod stride 0)
    assert_bitwise(h.dtw(dev(torch, a), dev(torch, b[2])).cpu().numpy(), host_dtw(a, b[2]), "fp64, shared reference")
    # fp32 inputs: fp64 arithmetic on the upcast samples
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    got = h.dtw(dev(torch, a32, torch.float32), dev(torch, b32, torch.float32)).cpu().numpy()
    assert_bitwise(got, host_dtw(a32.astype(np.float64), b32.astype(np.float64)), "fp32 inputs")
    got = h.dtw(dev(torch, a32, torch.float32), dev(torch, b32[1], torch.float32)).cpu().numpy()
    assert_bitwise(got, host_dtw(a32.astype(np.float64), b32[1].astype(np.float64)), "fp32 inputs, shared reference")
    # a sequence against itself
    assert_bitwise(h.dtw(dev(torch, a), dev(torch, a)).cpu().numpy(), np.zeros(B5), "identical sequences")
    if Ta == Tb:
        assert_bitwise(h.dtw(dev(torch, b), dev(torch, b[0])).cpu().numpy()[:1], np.zeros(1), "identical, shared")


# ---------------------------------------------------------------------------
# 2. strided read of a state history
# ---------------------------------------------------------------------------
def test_dtw_reads_a_state_history_in_place(torch_cuda, handles):
    """A history [T+1][B][N][KR_SLOTS], sized exactly, read at one grid point through the strides - as a torch view and
    as the header states it (pointer to slot 12 of the point in states[0], rod stride N KR_SLOTS, step stride
    B N KR_SLOTS) - against the contiguous copy of the same samples; also the last rod at the last grid point."""
    import krod_native as kn
    torch, h = torch_cuda, handles[33]
    N, T, S = 33, 20, kn.KR_SLOTS
    hist = np.cumsum(np.random.default_rng(7).normal(size=(T + 1, B5, N, S)) * 0.01, axis=0)
    ref = walk(8, B5, 17, 3)
    hist_d, ref_d = dev(torch, hist), dev(torch, ref)
    assert hist_d.numel() == (T + 1) * B5 * N * S
    for j in (17, N - 1):
        path = hist[:, :, j, 12:15].transpose(1, 0, 2)  # [B, T+1, 3]
        want = host_dtw(path, ref)
        packed = h.dtw(dev(torch, path), ref_d).cpu().numpy()
        view = h.dtw(hist_d[:, :, j, 12:15].permute(1, 0, 2), ref_d).cpu().numpy()
        raw = torch.full((B5,), SENTINEL, dtype=torch.float64, device=DEV)
        kn.check(h.lib.kr_dtw_batch(h._h, B5, C.c_void_p(hist_d.data_ptr() + 8 * (j * S + 12)), T + 1, N * S, B5 * N * S,
                                    kn._ptr(ref_d), 17, 17 * 3, 3, kn._ptr(raw), kn.KR_F64, kn._stream()))
        assert_bitwise(packed, want, f"grid point {j}, contiguous copy")
        assert_bitwise(view, packed, f"grid point {j}, torch view")
        assert_bitwise(raw.cpu().numpy(), packed, f"grid point {j}, raw strides")
        # the history as the SECOND sequence
        assert_bitwise(h.dtw(ref_d, hist_d[:, :, j, 12:15].permute(1, 0, 2)).cpu().numpy(), host_dtw(ref, path), f"grid point {j}, as b")


# ---------------------------------------------------------------------------
# 3. rods are independent
# ---------------------------------------------------------------------------
def test_dtw_rod_in_batch_equals_rod_alone(torch_cuda, handles):
    torch, h = torch_cuda, handles[10]
    a, b = walk(31, B5, 130, 3), walk(32, B5, 99, 3)
    batch = h.dtw(dev(torch, a), dev(torch, b)).cpu().numpy()
    for r in range(B5):
        alone = h.dtw(dev(torch, a[r:r + 1]), dev(torch, b[r:r + 1])).cpu().numpy()
        assert_bitwise(alone, batch[r:r + 1], f"rod {r}")
    assert len(set(batch.tolist())) == B5  # distinct data, distinct distances


# ---------------------------------------------------------------------------
# 4. limits
# ---------------------------------------------------------------------------
def test_dtw_long_sequences_exact(torch_cuda, handles):
    torch, h = torch_cuda, handles[10]
    a, b = walk(41, 2, 2048, 3), walk(42, 2, 1500, 3)
    assert_bitwise(h.dtw(dev(torch, a), dev(torch, b)).cpu().numpy(), host_dtw(a, b), "(2048, 1500)")


def test_dtw_beyond_the_limit_is_refused(torch_cuda, handles):
    import krod_native as kn
    torch, h = torch_cuda, handles[10]
    L = kn.KR_DTW_MAX_LEN
    long_d, short_d = dev(torch, walk(43, 2, L + 1, 3)), dev(torch, walk(44, 2, 9, 3))
    for a, b in ((long_d, short_d), (short_d, long_d)):
        out = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
        with pytest.raises(kn.KrError, match=str(L)) as e:
            h.dtw(a, b, out=out)
        assert e.value.code == kn.KR_E_UNSUPPORTED
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all()
    # the limit itself is served
    a = walk(45, 1, L, 3)
    assert_bitwise(h.dtw(dev(torch, a), dev(torch, a[:, :5])).cpu().numpy(), host_dtw(a, a[:, :5]), "Ta = limit")


# ---------------------------------------------------------------------------
# 5. pose MSE
# ---------------------------------------------------------------------------
def poses(seed, R, T, N, angles=None):
    """Trajectories [R, T, 7, N]: positions a random walk, quaternions from zyx angles with |b| <= 1.2 scaled by
    0.5 .. 2 (non-unit); ``angles``: perturb these by N(0, 0.05) instead of drawing new ones.  Returns (traj, angles)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    if angles is None:
        ang = rng.uniform(-1.0, 1.0, size=(R, T, N, 3)) * np.array([2.5, 1.1, 2.5])  # (away from the +-pi seam of atan2)
    else:
        ang = np.broadcast_to(angles, (R,) + angles.shape[1:]) + rng.normal(size=(R, T, N, 3)) * 0.05
        ang[..., 1] = np.clip(ang[..., 1], -1.2, 1.2)
    q = Rotation.from_euler("zyx", ang.reshape(-1, 3)).as_quat(scalar_first=True).reshape(R, T, N, 4)
    q = q * rng.uniform(0.5, 2.0, size=(R, T, N, 1))
    p = np.cumsum(rng.normal(size=(R, T, N, 3)) * 0.01, axis=1)
    return np.concatenate([p, q], axis=-1).transpose(0, 1, 3, 2).copy(), ang


@pytest.mark.parametrize("ref_B", ["shared", "per rod"])
@pytest.mark.parametrize("T", [1, 3, 17])
@pytest.mark.parametrize("N", [10, 33])
def test_pose_mse_against_host(torch_cuda, handles, N, T, ref_B):
    from krod_eval import pos_euler_mse
    torch, h = torch_cuda, handles[N]
    R = 1 if ref_B == "shared" else B5
    ref, ang = poses(1000 + N + T, R, T, N)
    traj, ang2 = poses(2000 + N + T, B5, T, N, angles=ang)
    rms = float(np.sqrt(np.mean((ang2 - ang) ** 2)))
    assert rms >= 1e-2, rms
    for dtype, label in ((torch.float64, "fp64"), (torch.float32, "fp32 inputs")):
        if dtype == torch.float32:  # the metric of the rounded inputs
            traj_h, ref_h = traj.astype(np.float32).astype(np.float64), ref.astype(np.float32).astype(np.float64)
        else:
            traj_h, ref_h = traj, ref
        want = np.array([pos_euler_mse(traj_h[r], ref_h[r % R]) for r in range(B5)])
        st, rst = h.pack_poses(traj, dtype), h.pack_poses(ref, dtype)
        assert st.shape == (T, B5, N, 28) and rst.shape == (T, R, N, 28)
        mse, parts = h.pose_mse(st, rst)
        mse2, parts2 = h.pose_mse(st, rst)
        got, pr = mse.cpu().numpy(), parts.cpu().numpy()
        err = float(np.max(np.abs(got - want) / want))
        print(f"N={N} T={T} {ref_B} {label}: max relative error {err:.2e} (bound 1e-10)")
        assert err <= 1e-10, (got, want)
        assert np.all(np.abs(pr.sum(1) - got * (6 * T * N) / 1000.0) <= 1e-14 * pr.sum(1))
        assert np.all(pr > 0)
        assert_bitwise(mse2.cpu().numpy(), got, "second call")
        assert_bitwise(parts2.cpu().numpy().ravel(), pr.ravel(), "second call, parts")


def test_pos_euler_mse_batch_and_dtw_distance_batch(torch_cuda):
    """The krod_eval front ends (host arrays in, NumPy out) agree with their one-rod host functions."""
    from krod_eval import dtw_distance_batch, pos_euler_mse, pos_euler_mse_batch
    robot = make_robot(None, 10)
    ref, ang = poses(51, 1, 5, 10)
    traj, _ = poses(52, 3, 5, 10, angles=ang)
    got = pos_euler_mse_batch(robot, traj, ref[0])
    want = np.array([pos_euler_mse(traj[r], ref[0]) for r in range(3)])
    assert np.max(np.abs(got - want) / want) <= 1e-10
    got = pos_euler_mse_batch(robot, traj, np.repeat(ref, 3, axis=0))
    assert np.max(np.abs(got - want) / want) <= 1e-10
    a, b = walk(53, 3, 40, 3), walk(54, 3, 70, 3)
    assert_bitwise(dtw_distance_batch(robot, a, b), host_dtw(a, b), "dtw_distance_batch")
    assert_bitwise(dtw_distance_batch(robot, a, b[1]), host_dtw(a, b[1]), "dtw_distance_batch, shared")


# ---------------------------------------------------------------------------
# 6. end to end: the eight model variants scored in the simulate call
# ---------------------------------------------------------------------------
def test_simulate_batch_scores_the_eight_mods(torch_cuda):
    from knode import simulate_batch
    from krod_eval import dtw_distance, evaluate_batch, pos_euler_mse
    g = load_golden("sim_misc")
    robots = [make_robot(m, 10) for m in MODS7] + [make_robot(None, 10)]
    ctl = np.stack([g[f"mod_{m}_ctl"] for m in MODS7] + [g["random_ctl"][:16]])
    carrier = make_robot(None, 10)
    first = simulate_batch(carrier, ctl, robots=robots)
    assert np.all(first["status"] == 0)
    ref = first["traj"][7, :16]
    out = simulate_batch(carrier, ctl, robots=robots, score={"reference": ref})
    assert out["dtw"].dtype == np.float64 and out["dtw"].shape == (8,) and out["mse"].shape == (8,)
    want_dtw = np.array([dtw_distance(out["traj"][b, :16, :3, 9], ref[:, :3, 9]) for b in range(8)])
    assert_bitwise(out["dtw"], want_dtw, "dtw")
    want_mse = np.array([pos_euler_mse(out["traj"][b, :16], ref) for b in range(8)])
    err = np.abs(out["mse"][:7] - want_mse[:7]) / want_mse[:7]
    print(f"end to end: mse max relative error {err.max():.2e} (bound 1e-10); dtw {out['dtw']}; mse {out['mse']}")
    assert err.max() <= 1e-10
    assert out["dtw"][7] == 0.0 and out["mse"][7] == 0.0 and want_mse[7] == 0.0
    assert np.all(out["dtw"][:7] > 0) and np.all(out["mse"][:7] > 0)
    # no trajectory leaves the device, same numbers
    lean = simulate_batch(carrier, ctl, robots=robots, score={"reference": ref}, return_states=False)
    assert "traj" not in lean
    assert_bitwise(lean["dtw"], out["dtw"], "return_states=False, dtw")
    assert_bitwise(lean["mse"], out["mse"], "return_states=False, mse")
    d, m = evaluate_batch(carrier, robots, ctl, ref)
    assert_bitwise(d, out["dtw"], "evaluate_batch, dtw")
    assert_bitwise(m, out["mse"], "evaluate_batch, mse")
    # another grid point, a reference per rod
    out5 = simulate_batch(carrier, ctl, robots=robots, score={"reference": np.repeat(ref[None], 8, axis=0), "point": 5})
    want5 = np.array([dtw_distance(out5["traj"][b, :16, :3, 5], ref[:, :3, 5]) for b in range(8)])
    assert_bitwise(out5["dtw"], want5, "dtw at grid point 5")
    assert_bitwise(out5["mse"], out["mse"], "mse, reference per rod")


# ---------------------------------------------------------------------------
# 7. argument errors leave the outputs alone
# ---------------------------------------------------------------------------
def test_argument_errors_leave_outputs_untouched(torch_cuda, handles):
    import krod_native as kn
    torch, h = torch_cuda, handles[10]
    lib, S = h.lib, kn._stream()
    a, b = dev(torch, walk(61, 2, 9, 3)), dev(torch, walk(62, 2, 7, 3))
    dist = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    pa, pb, pd = kn._ptr(a), kn._ptr(b), kn._ptr(dist)
    dtw_bad = {
        "null a": (h._h, 2, None, 9, 27, 3, pb, 7, 21, 3, pd, kn.KR_F64),
        "null b": (h._h, 2, pa, 9, 27, 3, None, 7, 21, 3, pd, kn.KR_F64),
        "null dist": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, None, kn.KR_F64),
        "B = 0": (h._h, 0, pa, 9, 27, 3, pb, 7, 21, 3, pd, kn.KR_F64),
        "Ta = 0": (h._h, 2, pa, 0, 27, 3, pb, 7, 21, 3, pd, kn.KR_F64),
        "Tb < 0": (h._h, 2, pa, 9, 27, 3, pb, -1, 21, 3, pd, kn.KR_F64),
        "negative rod stride": (h._h, 2, pa, 9, -27, 3, pb, 7, 21, 3, pd, kn.KR_F64),
        "negative step stride": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, -3, pd, kn.KR_F64),
        "dtype": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, pd, 2),
    }
    for label, args in dtw_bad.items():
        assert lib.kr_dtw_batch(*args, S) == kn.KR_E_ARG, label
        assert lib.kr_last_error(), label
    T, N = 3, 10
    ref, ang = poses(63, 1, T, N)
    st, rst = h.pack_poses(poses(64, 2, T, N, angles=ang)[0], torch.float64), h.pack_poses(ref, torch.float64)
    mse = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    parts = torch.full((2, 2), SENTINEL, dtype=torch.float64, device=DEV)
    ps, pr, pm, pp = kn._ptr(st), kn._ptr(rst), kn._ptr(mse), kn._ptr(parts)
    mse_bad = {
        "null states": (h._h, 2, T, None, pr, 1, pm, pp, kn.KR_F64),
        "null ref": (h._h, 2, T, ps, None, 1, pm, pp, kn.KR_F64),
        "null mse": (h._h, 2, T, ps, pr, 1, None, pp, kn.KR_F64),
        "B = 0": (h._h, 0, T, ps, pr, 1, pm, pp, kn.KR_F64),
        "T = 0": (h._h, 2, 0, ps, pr, 1, pm, pp, kn.KR_F64),
        "ref_B = 0": (h._h, 2, T, ps, pr, 0, pm, pp, kn.KR_F64),
        "ref_B = 3": (h._h, 2, T, ps, pr, 3, pm, pp, kn.KR_F64),
        "dtype": (h._h, 2, T, ps, pr, 1, pm, pp, -1),
    }
    for label, args in mse_bad.items():
        assert lib.kr_pose_mse_batch(*args, S) == kn.KR_E_ARG, label
        assert lib.kr_last_error(), label
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == SENTINEL).all() and (mse.cpu().numpy() == SENTINEL).all()
    assert (parts.cpu().numpy() == SENTINEL).all()
    # parts is optional
    kn.check(lib.kr_pose_mse_batch(h._h, 2, T, ps, pr, 1, pm, None, kn.KR_F64, S))
    torch.cuda.synchronize()
    assert (parts.cpu().numpy() == SENTINEL).all() and not (mse.cpu().numpy() == SENTINEL).any()
