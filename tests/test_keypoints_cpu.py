"""Key-point records (kr_simulate_batch_keypoints, kr_keypoints_check, kr_pose_mse_points_batch), host side (no GPU):
the C ABI surface, the rule of the point set - 1 <= K <= 16 grid points, strictly increasing, each in [0, N), the first
bad entry named - through the handle-free check, the validation of ``knode.simulate_batch(..., key_points=...)``, which
raises before anything touches a device or the library, and the layout of the result's ``kp``."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "knode_rod.h")


@pytest.fixture(scope="module")
def kn():
    import krod_native as kn
    if not os.path.exists(kn.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as ge
        ge.build()
    kn.load()
    return kn


def preset_robot(mod, N=10):
    from cosserat_ode import CosseratRod
    from knode import setup_robot
    r = CosseratRod(use_fsolve=True)
    setup_robot(r, mod)
    r.N = N
    r.compute_intermediate_terms()
    return r


def header_proto(name):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert proto, f"{name} is not declared in include/knode_rod.h"
    return [a.split()[-1].lstrip("*") for a in proto.group(1).split(",")]


def test_symbols_declared_exported_and_bound(kn):
    text = open(HEADER).read()
    assert re.search(r"#define\s+KR_KEYPOINTS_MAX\s+16\b", text) and kn.KR_KEYPOINTS_MAX == 16
    lib = kn.load()
    vp, i64, i32p = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)
    want = {
        "kr_keypoints_check": (["N", "K", "idx_host"], [ctypes.c_int, ctypes.c_int, i32p]),
        "kr_simulate_batch_keypoints": (
            ["h", "t", "T", "scheme", "ctl", "bnd", "K", "idx_host", "kp", "states", "ring", "G", "tip", "tol", "maxit", "status",
             "use_nn", "state_prev_init", "dtype", "stream"],
            [vp, vp, i64, ctypes.c_int, vp, vp, ctypes.c_int, i32p, vp, vp, ctypes.c_int, vp, vp, ctypes.c_double, ctypes.c_int,
             vp, ctypes.c_int, vp, ctypes.c_int, vp]),
        "kr_pose_mse_points_batch": (
            ["h", "B", "T", "P", "records", "ref_records", "ref_B", "mse", "parts", "dtype", "stream"],
            [vp, i64, i64, i64, vp, vp, i64, vp, vp, ctypes.c_int, vp]),
    }
    for name, (args, types) in want.items():
        assert header_proto(name) == args, (name, header_proto(name))
        assert hasattr(ctypes.CDLL(kn.LIB_PATH), name), f"{name} is not exported by the library"
        assert name in kn.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == types, name
    # the key-point call is the boundary call with K, idx_host, kp behind bnd; the points form of the MSE has P behind T
    b = list(lib.kr_simulate_batch_boundary.argtypes)
    assert want["kr_simulate_batch_keypoints"][1] == b[:6] + [ctypes.c_int, i32p, vp] + b[6:]
    m = list(lib.kr_pose_mse_batch.argtypes)
    assert want["kr_pose_mse_points_batch"][1] == m[:3] + [i64] + m[3:]


def test_keypoints_check_rule(kn):
    lib = kn.load()

    def chk(N, pts):
        arr = (ctypes.c_int32 * max(len(pts), 1))(*pts)
        return lib.kr_keypoints_check(N, len(pts), arr), lib.kr_last_error().decode()

    for N in (10, 23, 100, 128):
        assert chk(N, [0])[0] == 0
        assert chk(N, [N - 1])[0] == 0
    assert chk(23, list(range(16)))[0] == 0
    assert chk(128, [0, 63, 64, 65, 127])[0] == 0
    assert chk(128, list(range(112, 128)))[0] == 0

    def refused(N, pts, *words):
        rc, msg = chk(N, pts)
        assert rc == kn.KR_E_ARG, (pts, rc)
        assert "kr_keypoints_check" in msg and all(w in msg for w in words), msg

    refused(23, [], "K = 0")
    refused(23, list(range(17)), "K = 17")
    refused(23, [3, 5, 5, 9], "idx[2] = 5", "strictly increasing")      # a duplicate
    refused(23, [3, 9, 7], "idx[2] = 7", "idx[1] = 9")                  # a descending pair
    refused(23, [-1, 4], "idx[0] = -1", "[0, 23)")
    refused(23, [4, 23], "idx[1] = 23", "[0, 23)")
    refused(23, [4, 22, 23, 2], "idx[2] = 23")                          # the FIRST bad entry
    assert lib.kr_keypoints_check(23, 2, None) == kn.KR_E_ARG and "idx" in lib.kr_last_error().decode()


def test_simulate_batch_validates_key_points_on_the_host(kn, monkeypatch):
    import knode
    robot = preset_robot(None)
    monkeypatch.setattr(type(robot), "_native", lambda self: pytest.fail("a device call before validation"))
    monkeypatch.setattr(kn, "load", lambda: pytest.fail("a library call before validation"))
    B, T = 3, 5
    ctl = np.full((B, T, 4), 5.0)

    def refused(word, **kw):
        with pytest.raises(kn.KrError) as e:
            knode.simulate_batch(robot, ctl, **kw)
        assert word in str(e.value), str(e.value)

    refused("key point 10 outside the rod's 10 grid points", key_points=[3, 10])
    refused("key point -11 outside", key_points=[-11])
    refused("0 key points", key_points=[])
    refused("list of integer grid points", key_points=[1.5, 2])
    refused("list of integer grid points", key_points="tip")
    refused("list of integer grid points", key_points=[[1, 2], [3, 4]])
    refused("list of integer grid points", key_points=[True, False])
    refused("not served", key_points=[3, 5], per_robot_nn=True)
    refused("not served", key_points=[3, 5], robots=[robot] * B, per_robot_nn=True)
    with pytest.raises(kn.KrError, match=r"ctl must be \[B, T, 4\]"):
        knode.simulate_batch(robot, ctl[0], key_points=[3])
    # what rides with it is validated as it is alone
    refused("[3, 5, 13]", key_points=[3], base_motion=np.zeros((B, T, 12)))
    refused("[3, 5, 6]", key_points=[3], tip_loads=np.zeros((B, T, 5)))
    # score with tip_only: today's text without key points; with them the score point must be one
    ref = np.zeros((T + 1, 7, 10))
    refused("score needs the state history", tip_only=True, score={"reference": ref})
    refused("score point 9 is not one of the key points [3, 5]", tip_only=True, key_points=[3, 5], score={"reference": ref})
    refused("score point 7 is not one of the key points", tip_only=True, key_points=[3, 5, 9], score={"reference": ref, "point": -3})
    refused("score reference has 4 grid points", tip_only=True, key_points=[3, 9], score={"reference": np.zeros((T, 7, 4))})
    # sorted, de-duplicated, negative indices from the tip
    assert knode._key_points([9, 3, -1, 5, 3, -5], 10).tolist() == [3, 5, 9]
    assert knode._key_points(np.array([-1]), 23).tolist() == [22] and knode._key_points([-1], 23).dtype == np.int32
    assert knode._key_points(list(range(16)) + [-23], 23).tolist() == list(range(16))
    with pytest.raises(kn.KrError, match="17 key points"):
        knode._key_points(range(17), 23)
    # ... and the binding refuses what the call does not take before it calls the library
    H = kn.Handle
    for kw, word in ((dict(table=object(), bank=object(), net_of_rod=[0] * B, bnd=ctl), "bank"),
                     (dict(table=object(), loads=ctl, bnd=ctl), "loads"),
                     (dict(bnd=ctl), "table"), (dict(table=object()), "bnd")):
        with pytest.raises(kn.KrError, match=word):
            H.simulate(object.__new__(H), ctl, None, None, key_points=[3], kp=ctl, **kw)
    with pytest.raises(kn.KrError, match="together"):
        H.simulate(object.__new__(H), ctl, None, None, table=object(), bnd=ctl, key_points=[3])


def test_constant_boundary_comes_from_the_rows(kn):
    import knode
    T = 4
    robots = []
    for b, mod in enumerate([None, "damping", "short"]):
        r = preset_robot(mod)
        r.p0, r.h0 = np.array([0.01 * b, -0.02, 0.03]), np.array([0.98, 0.05 * b, -0.1, 0.02])
        r.q0, r.w0 = np.array([0.01, 0.0, -0.02 * b]), np.array([0.05, -0.03, 0.02])
        r.F_tip, r.M_tip = np.array([0.1 * (b + 1), -0.2, 0.3 * b]), np.array([1e-3 * b, 2e-3, -1e-3 * (b + 1)])
        robots.append(r)
    rows = [r._params() for r in robots]
    base = knode._base_of_rows(rows, T)
    assert base.shape == (3, T, 13) and base.dtype == np.float64
    bnd = knode._boundary(base, None, rows)
    for b, r in enumerate(robots):
        want = np.concatenate([r.p0, r.h0, r.q0, r.w0, r.F_tip, r.M_tip])
        assert np.array_equal(bnd[b], np.tile(want, (T, 1)))


def test_result_layout():
    """``kp`` is ``traj[:, :, :, key_points]``: packed records (q w v u p h n m, three pad slots) to the reference's rows."""
    import knode
    T, B, N = 4, 3, 10
    idx = [2, 6, 9]
    rng = np.random.default_rng(16)
    traj = rng.normal(size=(B, T + 1, 25, N))                    # reference row order: p h n m q w v u
    packed = np.zeros((T + 1, B, N, 28))
    packed[..., 12:25] = traj[:, :, 0:13].transpose(1, 0, 3, 2)  # p h n m
    packed[..., 0:12] = traj[:, :, 13:25].transpose(1, 0, 3, 2)  # q w v u
    kp = knode._kp_rows(packed[:, :, idx])
    assert kp.shape == (B, T + 1, 25, len(idx)) and kp.flags["C_CONTIGUOUS"]
    assert np.array_equal(kp, traj[:, :, :, idx])
