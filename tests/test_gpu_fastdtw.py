"""FastDTW on the MI355X (kr_fastdtw_batch, Handle.fastdtw, score={"metric": "fastdtw"}) against the host statement of
the algorithm, ``krod_eval.fastdtw_path`` - BITWISE: distance, path length and path.  The kernel runs the same
additions, the same comparisons in the same order and the same window per level, so there is no tolerance anywhere in
this file.  Cases and their shared host results: ``tests/fastdtw_cases.py``; tests/test_fastdtw_cpu.py asserts that its
random walks separate FastDTW from the exact DTW, so a kernel that returned ``kr_dtw_batch``'s distance cannot pass."""
import ctypes as C

import numpy as np
import pytest

import fastdtw_cases as fc
from conftest import load_golden
from gpu_helpers import inject, make_robot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = fc.B16
SENTINEL = -12345.5
ISENT = -777
MODS7 = ["noair", "nsw", "short", "damping", "dampstiff", "lengthstiff", "youngs"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    return {N: make_robot(None, N)._native() for N in (10, 33)}


def dev(torch, x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype or torch.float64).contiguous()


def assert_bitwise(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = got.view(np.uint64) == want.view(np.uint64)
    assert same.all(), f"{label}: rods {np.flatnonzero(~same).tolist()} differ: {got[~same]} vs {want[~same]}"


def assert_paths(steps, plen, want_paths, label, width):
    """steps[B, width, 2], plen[B] of the device against the host's paths; entries past the length stay as allocated (0)."""
    steps, plen = steps.cpu().numpy(), plen.cpu().numpy()
    assert steps.shape[1:] == (width, 2)
    for r, want in enumerate(want_paths):
        assert plen[r] == len(want), f"{label}: rod {r}: path length {plen[r]}, host {len(want)}"
        assert np.array_equal(steps[r, :plen[r]], want), f"{label}: rod {r}: path differs"
        assert not steps[r, plen[r]:].any(), f"{label}: rod {r}: entries past the path were written"


# ---------------------------------------------------------------------------
# 1. bitwise against the host, every shape and kind
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("Ta,Tb,radius", fc.CASES)
def test_fastdtw_bitwise_against_host(torch_cuda, handles, Ta, Tb, radius, kind):
    torch, h = torch_cuda, handles[10]
    a, b = fc.sequences(kind, B, Ta, Tb)
    want, want_paths = fc.host(kind, B, Ta, Tb, radius)
    ad, bd = dev(torch, a), dev(torch, b)
    dist, steps, plen = h.fastdtw(ad, bd, radius=radius, path=True)
    assert_bitwise(dist.cpu().numpy(), want, "distance")
    assert_paths(steps, plen, want_paths, "path", Ta + Tb - 1)
    # without the path (no walk back on level 0): the same distance
    assert_bitwise(h.fastdtw(ad, bd, radius=radius).cpu().numpy(), want, "distance, path = NULL")


@pytest.mark.parametrize("Ta,Tb,radius", [(5, 4, 2), (17, 33, 1), (64, 65, 1), (101, 101, 1), (101, 101, 3), (130, 67, 1)])
def test_fastdtw_fp32_inputs(torch_cuda, handles, Ta, Tb, radius):
    """fp32 inputs: the fp64 result on the upcast samples, bit for bit - every level's means are fp64."""
    torch, h = torch_cuda, handles[10]
    for kind in fc.KINDS:
        a, b = fc.sequences(kind, B, Ta, Tb)
        want, want_paths = fc.host(kind, B, Ta, Tb, radius, single=True)
        dist, steps, plen = h.fastdtw(dev(torch, a, torch.float32), dev(torch, b, torch.float32), radius=radius, path=True)
        assert_bitwise(dist.cpu().numpy(), want, f"{kind}, fp32 inputs")
        assert_paths(steps, plen, want_paths, f"{kind}, fp32 inputs", Ta + Tb - 1)


# ---------------------------------------------------------------------------
# 2. addressing: a state history in place, a shared reference
# ---------------------------------------------------------------------------
def test_fastdtw_reads_a_state_history_in_place(torch_cuda, handles):
    """One grid point of states[T+1][B][N][KR_SLOTS], sized exactly, through a torch view and through the raw strides the
    header states (pointer to slot 12 of the point in states[0], rod stride N KR_SLOTS, step stride B N KR_SLOTS), as the
    first and as the second sequence; also the last rod at the last grid point."""
    import krod_native as kn
    from krod_eval import fastdtw_path
    torch, h = torch_cuda, handles[33]
    N, T, S, R = 33, 40, kn.KR_SLOTS, 5
    hist = np.cumsum(np.random.default_rng(7).normal(size=(T + 1, R, N, S)) * 0.01, axis=0)
    ref, _ = fc.sequences("walk", R, 37, 1)
    hist_d, ref_d = dev(torch, hist), dev(torch, ref)
    assert hist_d.numel() == (T + 1) * R * N * S
    for j in (17, N - 1):
        path = hist[:, :, j, 12:15].transpose(1, 0, 2)  # [R, T + 1, 3]
        res = [fastdtw_path(path[r], ref[r]) for r in range(R)]
        want = np.array([d for d, _ in res])
        view = hist_d[:, :, j, 12:15].permute(1, 0, 2)
        dist, steps, plen = h.fastdtw(view, ref_d, path=True)
        assert_bitwise(dist.cpu().numpy(), want, f"grid point {j}, torch view")
        assert_paths(steps, plen, [np.asarray(p) for _, p in res], f"grid point {j}", T + 37)
        raw = torch.full((R,), SENTINEL, dtype=torch.float64, device=DEV)
        assert h.lib.kr_fastdtw_ws_bytes(R, T + 1, 37, 1) == 0
        kn.check(h.lib.kr_fastdtw_batch(h._h, R, C.c_void_p(hist_d.data_ptr() + 8 * (j * S + 12)), T + 1, N * S, R * N * S,
                                        kn._ptr(ref_d), 37, 37 * 3, 3, 1, kn._ptr(raw), None, None, None, kn.KR_F64, kn._stream()))
        assert_bitwise(raw.cpu().numpy(), want, f"grid point {j}, raw strides")
        back = np.array([fastdtw_path(ref[r], path[r])[0] for r in range(R)])
        assert_bitwise(h.fastdtw(ref_d, view).cpu().numpy(), back, f"grid point {j}, as b")


def test_fastdtw_shared_reference(torch_cuda, handles):
    """b_rod_stride = 0: one reference for all rods."""
    from krod_eval import fastdtw_distance_batch, fastdtw_path
    torch, h = torch_cuda, handles[10]
    for kind, (Ta, Tb) in (("walk", (101, 101)), ("ints", (17, 33)), ("sine", (65, 64))):
        a, b = fc.sequences(kind, B, Ta, Tb)
        res = [fastdtw_path(a[r], b[3]) for r in range(B)]
        dist, steps, plen = h.fastdtw(dev(torch, a), dev(torch, b[3]), path=True)
        assert_bitwise(dist.cpu().numpy(), [d for d, _ in res], f"{kind}, shared reference")
        assert_paths(steps, plen, [np.asarray(p) for _, p in res], f"{kind}, shared reference", Ta + Tb - 1)
    # the krod_eval front end (host arrays in, NumPy out)
    a, b = fc.sequences("walk", B, 63, 129)
    want, want_paths = fc.host("walk", B, 63, 129, 1)
    got, paths = fastdtw_distance_batch(make_robot(None, 10), a, b, return_path=True)
    assert_bitwise(got, want, "fastdtw_distance_batch")
    assert all(np.array_equal(p, w) for p, w in zip(paths, want_paths))
    assert_bitwise(fastdtw_distance_batch(make_robot(None, 10), a, b), want, "fastdtw_distance_batch, distance only")


# ---------------------------------------------------------------------------
# 3. rods are independent
# ---------------------------------------------------------------------------
def test_fastdtw_rod_in_batch_equals_rod_alone(torch_cuda, handles):
    torch, h = torch_cuda, handles[10]
    a, b = fc.sequences("walk", B, 130, 67)
    dist, steps, plen = h.fastdtw(dev(torch, a), dev(torch, b), path=True)
    dist, steps, plen = dist.cpu().numpy(), steps.cpu().numpy(), plen.cpu().numpy()
    for r in (0, 7, B - 1):
        d1, s1, n1 = h.fastdtw(dev(torch, a[r:r + 1]), dev(torch, b[r:r + 1]), path=True)
        assert_bitwise(d1.cpu().numpy(), dist[r:r + 1], f"rod {r}")
        assert n1.cpu().numpy()[0] == plen[r] and np.array_equal(s1.cpu().numpy()[0], steps[r])
    assert len(set(dist.tolist())) == B  # distinct data, distinct distances


def test_fastdtw_1024_rods(torch_cuda, handles):
    """B = 1024 cycling over 32 distinct 101 x 101 pairs: every rod equals its pair's host value (32 host evaluations)."""
    torch, h = torch_cuda, handles[10]
    a16, b16 = fc.sequences("walk", B, 101, 101)
    a2, b2 = fc.sequences("sine", B, 101, 101)
    w1, p1 = fc.host("walk", B, 101, 101, 1)
    w2, p2 = fc.host("sine", B, 101, 101, 1)
    a, b, want, paths = np.concatenate([a16, a2]), np.concatenate([b16, b2]), np.concatenate([w1, w2]), p1 + p2
    idx = np.arange(1024) % 32
    dist, steps, plen = h.fastdtw(dev(torch, a[idx]), dev(torch, b[idx]), path=True)
    assert_bitwise(dist.cpu().numpy(), want[idx], "1024 rods")
    assert_paths(steps, plen, [paths[i] for i in idx], "1024 rods", 201)
    assert_bitwise(h.fastdtw(dev(torch, a[idx]), dev(torch, b[idx])).cpu().numpy(), want[idx], "1024 rods, distance only")


# ---------------------------------------------------------------------------
# 4. a rod that is not finite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Ta,Tb", [(101, 101), (5, 4), (700, 300)])
def test_fastdtw_non_finite_rod(torch_cuda, handles, Ta, Tb):
    """One rod with a NaN sample in a, one with an inf sample in b: NaN and path length 0 for those, every other rod bit
    for bit the clean call's, and the call returns normally.  (700 x 300: the back-pointers are in the workspace.)"""
    torch, h = torch_cuda, handles[10]
    R = 6
    a, b = fc.sequences("walk", R, Ta, Tb)
    clean = h.fastdtw(dev(torch, a), dev(torch, b), path=True)
    a2, b2 = a.copy(), b.copy()
    a2[1, Ta - 1, 2] = np.nan
    b2[4, Tb // 2, 0] = np.inf
    got = h.fastdtw(dev(torch, a2), dev(torch, b2), path=True)
    torch.cuda.synchronize()
    d0, s0, n0 = (t.cpu().numpy() for t in clean)
    d1, s1, n1 = (t.cpu().numpy() for t in got)
    sick, well = [1, 4], [0, 2, 3, 5]
    assert np.isnan(d1[sick]).all() and (n1[sick] == 0).all() and not s1[sick].any()
    assert_bitwise(d1[well], d0[well], "healthy rods")
    assert np.array_equal(n1[well], n0[well]) and np.array_equal(s1[well], s0[well])
    assert np.isfinite(d0).all() and (n0 > 0).all()
    assert np.isnan(h.fastdtw(dev(torch, a2), dev(torch, b2)).cpu().numpy()[sick]).all()


# ---------------------------------------------------------------------------
# 5. refusals and limits
# ---------------------------------------------------------------------------
def test_fastdtw_refusals_leave_outputs_untouched(torch_cuda, handles):
    import krod_native as kn
    torch, h = torch_cuda, handles[10]
    lib, S, L = h.lib, kn._stream(), kn.KR_FASTDTW_MAX_LEN
    a, b = dev(torch, fc.sequences("walk", 2, 9, 7)[0]), dev(torch, fc.sequences("walk", 2, 9, 7)[1])
    big = dev(torch, np.zeros((2, L + 1, 3)))
    dist = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    steps = torch.full((2, L + 9, 2), ISENT, dtype=torch.int32, device=DEV)
    plen = torch.full((2,), ISENT, dtype=torch.int32, device=DEV)
    ws = torch.zeros((max(int(lib.kr_fastdtw_ws_bytes(2, L, L, 1)), 16),), dtype=torch.uint8, device=DEV)
    pa, pb, pg, pd, ps, pl, pw = (kn._ptr(t) for t in (a, b, big, dist, steps, plen, ws))
    F = kn.KR_F64
    arg = {
        "null handle": (None, 2, pa, 9, 27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "null a": (h._h, 2, None, 9, 27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "null b": (h._h, 2, pa, 9, 27, 3, None, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "null dist": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, 1, None, ps, pl, pw, F),
        "B = 0": (h._h, 0, pa, 9, 27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "Ta = 0": (h._h, 2, pa, 0, 27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "Tb < 0": (h._h, 2, pa, 9, 27, 3, pb, -1, 21, 3, 1, pd, ps, pl, pw, F),
        "negative rod stride": (h._h, 2, pa, 9, -27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "negative step stride": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, -3, 1, pd, ps, pl, pw, F),
        "radius 0": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, 0, pd, ps, pl, pw, F),
        "radius -1": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, -1, pd, ps, pl, pw, F),
        "path without path_len": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, 1, pd, ps, None, pw, F),
        "path_len without path": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, 1, pd, None, pl, pw, F),
        "no workspace where one is needed": (h._h, 2, pg, L, 3 * (L + 1), 3, pg, L, 3 * (L + 1), 3, 1, pd, ps, pl, None, F),
        "dtype": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, 2),
    }
    unsupported = {
        "radius 9": (h._h, 2, pa, 9, 27, 3, pb, 7, 21, 3, kn.KR_FASTDTW_MAX_RADIUS + 1, pd, ps, pl, pw, F),
        "Ta beyond the limit": (h._h, 2, pg, L + 1, 3 * (L + 1), 3, pb, 7, 21, 3, 1, pd, ps, pl, pw, F),
        "Tb beyond the limit": (h._h, 2, pa, 9, 27, 3, pg, L + 1, 3 * (L + 1), 3, 1, pd, ps, pl, pw, F),
    }
    assert int(lib.kr_fastdtw_ws_bytes(2, L, L, 1)) > 0
    for table, code in ((arg, kn.KR_E_ARG), (unsupported, kn.KR_E_UNSUPPORTED)):
        for label, args in table.items():
            assert lib.kr_fastdtw_batch(*args, S) == code, label
            assert lib.kr_last_error(), label
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == SENTINEL).all()
    assert (steps.cpu().numpy() == ISENT).all() and (plen.cpu().numpy() == ISENT).all()
    # the Python front end raises with the code
    with pytest.raises(kn.KrError, match=str(L)) as e:
        h.fastdtw(big, b)
    assert e.value.code == kn.KR_E_UNSUPPORTED


def test_fastdtw_the_limit_itself_is_served(torch_cuda, handles):
    """One rod of KR_FASTDTW_MAX_LEN samples a side, distance only (the back-pointers of level 0 are in the workspace);
    the host needs well under 10 s for it.  Also a mid-sized batch that takes the workspace, with paths."""
    import krod_native as kn
    torch, h = torch_cuda, handles[10]
    L = kn.KR_FASTDTW_MAX_LEN
    assert int(h.lib.kr_fastdtw_ws_bytes(1, L, L, 1)) > 0
    a, b = fc.sequences("walk", 1, L, L)
    want, _ = fc.host("walk", 1, L, L, 1)
    assert_bitwise(h.fastdtw(dev(torch, a), dev(torch, b)).cpu().numpy(), want, f"{L} x {L}")
    assert int(h.lib.kr_fastdtw_ws_bytes(3, 700, 300, 2)) > 0
    a, b = fc.sequences("walk", 3, 700, 300)
    want, want_paths = fc.host("walk", 3, 700, 300, 2)
    dist, steps, plen = h.fastdtw(dev(torch, a), dev(torch, b), radius=2, path=True)
    assert_bitwise(dist.cpu().numpy(), want, "700 x 300, radius 2")
    assert_paths(steps, plen, want_paths, "700 x 300, radius 2", 999)


@pytest.mark.parametrize("Ta,Tb", [(1, 1), (1, 5), (2, 2), (3, 3), (4, 5), (5, 4), (8, 8), (8, 3)])
def test_fastdtw_radius_covering_the_table_is_the_exact_dtw(torch_cuda, handles, Ta, Tb):
    """radius >= max(Ta, Tb): no level restricts anything, the distance is kr_dtw_batch's bit for bit."""
    torch, h = torch_cuda, handles[10]
    for kind in fc.KINDS:
        a, b = fc.sequences(kind, B, Ta, Tb)
        ad, bd = dev(torch, a), dev(torch, b)
        for radius in range(max(Ta, Tb), 9):
            assert_bitwise(h.fastdtw(ad, bd, radius=radius).cpu().numpy(), h.dtw(ad, bd).cpu().numpy(), f"{kind}, radius {radius}")


# ---------------------------------------------------------------------------
# 6. through Python: the scored simulate calls
# ---------------------------------------------------------------------------
def test_simulate_batch_scores_the_eight_mods_with_fastdtw(torch_cuda):
    from knode import simulate_batch
    from krod_eval import dtw_distance, evaluate_batch, fastdtw_distance
    g = load_golden("sim_misc")
    robots = [make_robot(m, 10) for m in MODS7] + [make_robot(None, 10)]
    ctl = np.stack([g[f"mod_{m}_ctl"] for m in MODS7] + [g["random_ctl"][:16]])
    carrier = make_robot(None, 10)
    first = simulate_batch(carrier, ctl, robots=robots)
    assert np.all(first["status"] == 0)
    ref = first["traj"][7, :16]
    out = simulate_batch(carrier, ctl, robots=robots, score={"reference": ref, "metric": "fastdtw"})
    assert out["dtw_metric"] == "fastdtw" and out["dtw"].dtype == np.float64 and out["dtw"].shape == (8,)
    want = np.array([fastdtw_distance(out["traj"][b, :16, :3, 9], ref[:, :3, 9]) for b in range(8)])
    assert_bitwise(out["dtw"], want, "fastdtw")
    out2 = simulate_batch(carrier, ctl, robots=robots, score={"reference": ref, "metric": "fastdtw", "radius": 2, "point": 5})
    want2 = np.array([fastdtw_distance(out2["traj"][b, :16, :3, 5], ref[:, :3, 5], 2) for b in range(8)])
    assert_bitwise(out2["dtw"], want2, "fastdtw, radius 2 at grid point 5")
    # the default call still returns the exact value, and says so
    exact = simulate_batch(carrier, ctl, robots=robots, score={"reference": ref})
    assert exact["dtw_metric"] == "dtw"
    assert_bitwise(exact["dtw"], [dtw_distance(exact["traj"][b, :16, :3, 9], ref[:, :3, 9]) for b in range(8)], "dtw")
    assert_bitwise(exact["mse"], out["mse"], "mse does not depend on the metric")
    d, m = evaluate_batch(carrier, robots, ctl, ref, metric="fastdtw")
    assert_bitwise(d, out["dtw"], "evaluate_batch, fastdtw")
    assert_bitwise(m, out["mse"], "evaluate_batch, mse")


def test_evaluate_bank_scores_key_points_with_fastdtw(torch_cuda):
    """A tip-only key-point run scored by evaluate_bank(metric="fastdtw") against the same run scored from its full
    history (simulate_bank with the states kept).  Six rods of N = 20 with the networks of a bank of three
    (tests/bank_keypoints_cases.py); the reference is the network-free rod's own run."""
    import bank_keypoints_cases as cases
    from knode import simulate_bank, simulate_batch
    from krod_eval import evaluate_bank, fastdtw_distance
    case, which = cases.CASE_SMALL, 3
    N, T = case["N"], case["T"]
    robots = []
    for row in case["rows"]:
        r = make_robot(row[0], N)
        inject(r, cases.bank(which)[cases.net_index(which, row[3])])
        robots.append(r)
    carrier = make_robot(None, N)
    ctl = np.stack([cases.banks.controls(T)] * len(robots))
    ref = simulate_batch(make_robot(None, N), ctl[:1])["traj"][0]  # [T + 1, 25, N]
    full = simulate_bank(carrier, robots, ctl, score={"reference": ref, "metric": "fastdtw"})
    assert full["dtw_metric"] == "fastdtw" and np.all(full["status"] == 0)
    want = np.array([fastdtw_distance(full["traj"][b, :, :3, -1], ref[:, :3, -1]) for b in range(len(robots))])
    assert_bitwise(full["dtw"], want, "simulate_bank, full history")
    assert np.all(want > 0)
    d, _ = evaluate_bank(carrier, robots, ctl, ref, [2, 6, 9, -1], metric="fastdtw")
    assert_bitwise(d, full["dtw"], "evaluate_bank, key points")
    d_exact, _ = evaluate_bank(carrier, robots, ctl, ref, [2, 6, 9, -1])
    assert np.all(d_exact <= d)
