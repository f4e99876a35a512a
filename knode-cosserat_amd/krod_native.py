"""ctypes binding of libknode_rod.so (C ABI: include/knode_rod.h).

This module is the only place where the shared library is touched.  It fails
loudly: if the library is missing or a symbol is absent, importing the solver
classes raises - there is no CPU fallback anywhere in this package.

torch is used only as the owner of device memory and streams; every pointer
handed to the library is ``tensor.data_ptr()`` of a contiguous CUDA(HIP) tensor
and every call is queued on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KR_LIB_PATH") or os.path.join(_HERE, "lib", "libknode_rod.so")

KR_SLOTS = 28
KR_F32, KR_F64 = 0, 1
KR_EULER, KR_RK4 = 0, 1
ACT_NONE, ACT_TANH, ACT_SOFTPLUS, ACT_RELU, ACT_ELU = range(5)
ST_CONVERGED, ST_MAXIT, ST_NONFINITE = 0, 1, 2
KR_MAX_LAYERS = 8
KR_DTW_MAX_LEN = 4096
KR_FASTDTW_MAX_LEN, KR_FASTDTW_MAX_RADIUS = 1024, 8  # kr_fastdtw_batch: samples per sequence, radius
KR_SOFTDTW_MAX_LEN = 1024  # kr_softdtw_batch: samples per sequence
SOFTDTW_COSTS = {"l1": 0, "sq": 1}  # kr_softdtw_batch's point costs (krod_eval.SOFTDTW_COSTS)
KR_BND = 19  # p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3) per rod and step (kr_simulate_batch_boundary)
KR_PAR = 43  # material parameters a step adjoint can differentiate (kr_step_vjp_par_batch), in the order of PAR_BLOCKS
# name, shape, offset into g_par[..., KR_PAR]: the order and row-major layout of struct kr_params (del_t and N are not differentiated)
PAR_BLOCKS = (("E", (), 0), ("r", (), 1), ("rho", (), 2), ("L", (), 3), ("vstar", (3,), 4), ("g", (3,), 7), ("Bse", (3, 3), 10),
              ("Bbt", (3, 3), 19), ("C", (3,), 28), ("tendon_dirs", (4, 3), 31))
KR_KEYPOINTS_MAX = 16  # key points per call (kr_simulate_batch_keypoints)
KR_E_ARG, KR_E_UNSUPPORTED = -1, -4
KR_E_HIP, KR_E_STATE = -2, -3

# reference row (0..24 of [y; z]) -> packed slot, see knode_rod.h
ROW_TO_SLOT = np.array([12 + r for r in range(13)] + [r - 13 for r in range(13, 19)] + [6 + (r - 19) for r in range(19, 25)])


class KrParams(C.Structure):
    _fields_ = [
        ("L", C.c_double), ("N", C.c_int32), ("nn_input_history", C.c_int32),
        ("E", C.c_double), ("r", C.c_double), ("rho", C.c_double),
        ("vstar", C.c_double * 3), ("g", C.c_double * 3), ("Bse", C.c_double * 9), ("Bbt", C.c_double * 9),
        ("C", C.c_double * 3), ("del_t", C.c_double), ("F_tip", C.c_double * 3), ("M_tip", C.c_double * 3),
        ("tendon_dirs", C.c_double * 12), ("p0", C.c_double * 3), ("h0", C.c_double * 4),
        ("q0", C.c_double * 3), ("w0", C.c_double * 3),
    ]


class KrDerived(C.Structure):
    _fields_ = [
        ("A", C.c_double), ("G", C.c_double), ("ds", C.c_double), ("c0", C.c_double), ("c1", C.c_double),
        ("c2", C.c_double), ("rhoA", C.c_double),
        ("J", C.c_double * 9), ("Kse", C.c_double * 9), ("Kbt", C.c_double * 9),
        ("Kse_plus_c0_Bse_inv", C.c_double * 9), ("Kbt_plus_c0_Bbt_inv", C.c_double * 9),
        ("Kse_vstar", C.c_double * 3), ("rhoAg", C.c_double * 3), ("rhoJ", C.c_double * 9),
    ]


_vp = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
_dbl = C.c_double


class KrTrainBankNet(C.Structure):
    """kr_train_bank_net: one training of a bank; every pointer is a device address."""
    _fields_ = [
        ("S", C.c_int64), ("ds", C.c_double),
        ("params", _vp), ("grads", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp),
        ("lower", _vp), ("sched", _vp), ("x", _vp), ("base", _vp), ("target_rows", _vp), ("loss_log", _vp),
    ]


_PROTOS = {
    "kr_last_error": (C.c_char_p, []),
    "kr_version": (_int, []),
    "kr_default_params": (_int, [C.POINTER(KrParams)]),
    "kr_apply_preset": (_int, [C.POINTER(KrParams), C.c_char_p]),
    "kr_apply_preset_original": (_int, [C.POINTER(KrParams), C.c_char_p]),
    "kr_create": (_int, [C.POINTER(KrParams), _int, C.POINTER(_vp)]),
    "kr_destroy": (_int, [_vp]),
    "kr_set_option": (_int, [_vp, C.c_char_p, _int]),
    "kr_get_option": (_int, [_vp, C.c_char_p, C.POINTER(C.c_int)]),
    "kr_debug_buffer": (_int, [_vp, _vp]),
    "kr_set_params": (_int, [_vp, C.POINTER(KrParams)]),
    "kr_get_derived": (_int, [_vp, C.POINTER(KrDerived)]),
    "kr_derive": (_int, [C.POINTER(KrParams), C.POINTER(KrDerived)]),
    "kr_mlp_eval_batch": (_int, [_vp, _i64, _vp, _vp, _int, _vp]),
    "kr_mlp_input_jacobian_batch": (_int, [_vp, _i64, _vp, _vp, _int, _vp]),
    "kr_set_mlp": (_int, [_vp, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_vp), _int, _vp]),
    "kr_ode_batch": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "kr_ode_vjp_batch": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_ode_jacobian_batch": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _int, _vp, _int, _vp]),
    "kr_state_init_straight": (_int, [_vp, _i64, _vp, _int, _vp]),
    "kr_state_pack": (_int, [_vp, _i64, _vp, _vp, _vp, _int, _vp]),
    "kr_state_unpack": (_int, [_vp, _i64, _vp, _vp, _vp, _int, _vp]),
    "kr_state_unpack50": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_state_tip": (_int, [_vp, _i64, _vp, _vp, _int, _vp]),
    "kr_residual_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _vp]),
    "kr_simulate_prepare": (_int, [_vp, _i64, _int]),
    "kr_residual_mid_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "kr_step_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, C.c_double, _int, _vp, _vp, _int, _vp, _int, _int, _vp]),
    "kr_simulate_batch": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp, _int, _vp, _int, _vp]),
    "kr_param_table_check": (_int, [C.POINTER(KrParams), _i64, C.POINTER(KrParams), C.POINTER(_i64)]),
    "kr_param_table_create": (_int, [_vp, _i64, C.POINTER(KrParams), C.POINTER(_vp)]),
    "kr_param_table_destroy": (_int, [_vp]),
    "kr_state_init_straight_table": (_int, [_vp, _vp, _vp, _int, _vp]),
    "kr_simulate_batch_table": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp, _int, _vp, _int, _vp]),
    "kr_simulate_batch_loads": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp, _int, _vp, _int,
                                       _vp]),
    "kr_simulate_batch_boundary": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp, _int, _vp, _int,
                                          _vp]),
    "kr_keypoints_check": (_int, [_int, _int, C.POINTER(C.c_int32)]),
    "kr_simulate_batch_keypoints": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _int, C.POINTER(C.c_int32), _vp, _vp, _int, _vp, _vp,
                                           C.c_double, _int, _vp, _int, _vp, _int, _vp]),
    "kr_mlp_bank_check": (_int, [C.POINTER(KrParams), _int, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kr_mlp_bank_create": (_int, [_vp, _int, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_vp), _int, _vp,
                                  C.POINTER(_vp)]),
    "kr_mlp_bank_destroy": (_int, [_vp]),
    "kr_mlp_bank_repack": (_int, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _int, _vp]),
    "kr_simulate_batch_bank_keypoints": (_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i64, _int, _vp, _vp, _int, C.POINTER(C.c_int32),
                                                _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp, _vp, _int, _vp]),
    "kr_simulate_batch_bank": (_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i64, _int, _vp, _vp, _int, _vp, _vp, C.c_double, _int, _vp,
                                      _vp, _int, _vp]),
    "kr_next_segment_physics": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _int, _vp]),
    "kr_mlp_ws_bytes": (C.c_size_t, [_int, C.POINTER(C.c_int32), _i64]),
    "kr_mlp_forward": (_int, [_vp, _i64, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_vp), _vp, _int, _vp, _vp, _vp]),
    "kr_mlp_forward_loss": (_int, [_vp, _i64, _int, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_vp),
                                   _vp, _int, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "kr_mlp_backward": (_int, [_vp, _i64, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_vp), _vp, _int, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "kr_loss_fwd_bwd": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "kr_gather_targets": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "kr_adam_step": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double,
                            C.c_double, _i64, _i64, _vp]),
    "kr_adam_plateau_step": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double,
                                    C.c_double, _i64, _i64, _i64, C.c_double, _int, C.c_double, C.c_double, _vp, _vp]),
    "kr_train_epoch": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp,
                              C.c_double, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, _i64, C.c_double,
                              _int, C.c_double, C.c_double, _vp, _int, _int, _vp]),
    "kr_train_epochs": (_int, [_vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp,
                               C.c_double, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, _i64, C.c_double,
                               _int, C.c_double, C.c_double, _vp, _int, _vp]),
    "kr_train_bank_check": (_int, [_int, C.POINTER(KrTrainBankNet), _int, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _int,
                                   _dbl]),
    "kr_train_bank_create": (_int, [_vp, _int, C.POINTER(KrTrainBankNet), _int, _int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    _int, _dbl, C.POINTER(_vp)]),
    "kr_train_bank_epochs": (_int, [_vp, _vp, _i64, _i64, _dbl, _dbl, _dbl, _dbl, _dbl, _int, _dbl, _dbl, _i64, _int, _vp]),
    "kr_train_bank_destroy": (_int, [_vp]),
    "kr_loss_rows_fwd_bwd": (_int, [_vp, _i64, _int, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "kr_estimate_ws_bytes": (C.c_size_t, [_i64, _int]),
    "kr_estimate_state": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "kr_dtw_batch": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _int, _vp]),
    "kr_fastdtw_ws_bytes": (C.c_size_t, [_i64, _i64, _i64, _int]),
    "kr_fastdtw_batch": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_softdtw_ws_bytes": (C.c_size_t, [_i64, _i64, _i64, _int]),
    "kr_softdtw_batch": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _dbl, _int, _vp, _vp, _i64, _i64, _vp, _int, _vp]),
    "kr_pose_mse_batch": (_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _int, _vp]),
    "kr_pose_mse_points_batch": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _int, _vp]),
    "kr_step_vjp_nn_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_simulate_vjp_nn_batch": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_step_vjp_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "kr_simulate_vjp_batch": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "kr_step_vjp_par_batch": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_simulate_vjp_par_batch": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_step_vjp_table_batch": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_simulate_vjp_table_batch": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int, _vp]),
    "kr_step_vjp_bank_batch": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "kr_simulate_vjp_bank_batch": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int,
                                          _vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOS)

_lib = None


class KrError(RuntimeError):
    code = 0


def load():
    """dlopen the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KrError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C knode-cosserat_amd/csrc`.  There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so both sides share one HIP runtime)
    except Exception:  # pragma: no cover - torch is optional for pure C users
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().kr_last_error()
        err = KrError(f"libknode_rod error {rc}: {msg.decode() if msg else '?'}")
        err.code = rc
        raise err


def split_par(g_par):
    """``g_par[..., KR_PAR]`` (array or tensor) -> dict of views by parameter name, shaped ``[..., *shape]`` (``PAR_BLOCKS``)."""
    lead = tuple(g_par.shape[:-1])
    out = {}
    for name, shape, off in PAR_BLOCKS:
        n = int(np.prod(shape)) if shape else 1
        out[name] = g_par[..., off:off + n].reshape(lead + shape)
    return out


def dtype_code(t) -> int:
    import torch
    if t in (torch.float32, np.float32, "f32"):
        return KR_F32
    if t in (torch.float64, np.float64, "f64"):
        return KR_F64
    raise KrError(f"unsupported dtype {t}")


def _ptr(t):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise KrError("libknode_rod works on device memory only: tensor is on " + str(t.device))
    if not t.is_contiguous():
        raise KrError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dtw_view(t, B, name):
    """(rod stride, step stride, samples) in elements of a device tensor read by ``Handle.dtw``: ``[B, T, 3]`` or, shared
    by all rods, ``[T, 3]`` - any view (a slice of a state history, an expanded tensor) whose 3 components are adjacent."""
    if not t.is_cuda:
        raise KrError("libknode_rod works on device memory only: tensor is on " + str(t.device))
    if t.dim() == 2:
        t = t.unsqueeze(0).expand(B, -1, -1)
    if t.dim() != 3 or t.shape[0] != B or t.shape[2] != 3 or t.shape[1] < 1:
        raise KrError(f"dtw: sequence {name} must be [B, T, 3] or [T, 3] with B = {B}, T >= 1; got {tuple(t.shape)}")
    rod, step, comp = t.stride()
    if comp != 1 or rod < 0 or step < 0:
        raise KrError(f"dtw: sequence {name}: the 3 components must be adjacent and the strides >= 0 (strides {t.stride()})")
    return (0 if B == 1 else rod), (0 if t.shape[1] == 1 else step), t.shape[1]


def softdtw_args(gamma, cost, Ta=1, Tb=1):
    """(gamma, cost code) of a soft-DTW call, checked on the host as ``kr_softdtw_batch`` checks them (no device, no
    library): gamma finite and > 0, cost ``"l1"`` or ``"sq"``, at most ``KR_SOFTDTW_MAX_LEN`` samples per sequence."""
    try:
        gamma = float(gamma)
    except (TypeError, ValueError):
        raise KrError(f"softdtw: gamma must be a number; got {gamma!r}") from None
    if not (np.isfinite(gamma) and gamma > 0.0):
        raise KrError(f"softdtw: gamma must be finite and > 0; got {gamma}")
    if not isinstance(cost, str) or cost not in SOFTDTW_COSTS:
        raise KrError(f"softdtw: cost must be one of {sorted(SOFTDTW_COSTS)}; got {cost!r}")
    if Ta > KR_SOFTDTW_MAX_LEN or Tb > KR_SOFTDTW_MAX_LEN:
        err = KrError(f"softdtw: sequences of {Ta} and {Tb} samples: at most {KR_SOFTDTW_MAX_LEN} samples per sequence are served")
        err.code = KR_E_UNSUPPORTED
        raise err
    return gamma, SOFTDTW_COSTS[cost]


def derive(params: KrParams) -> KrDerived:
    """Host-only derivation of the dependent terms (no GPU needed)."""
    d = KrDerived()
    check(load().kr_derive(C.byref(params), C.byref(d)))
    return d


def params_from_dict(d: dict) -> KrParams:
    lib = load()
    p = KrParams()
    check(lib.kr_default_params(C.byref(p)))
    for k, v in d.items():
        cur = getattr(p, k)
        if isinstance(cur, C.Array):
            arr = np.asarray(v, dtype=np.float64).reshape(-1)
            if arr.size != len(cur):
                raise KrError(f"parameter {k}: expected {len(cur)} values, got {arr.size}")
            for i, x in enumerate(arr):
                cur[i] = float(x)
        else:
            setattr(p, k, type(cur)(v))
    return p


def _params_array(rows):
    rows = list(rows)
    arr = (KrParams * max(len(rows), 1))()
    for i, r in enumerate(rows):
        if not isinstance(r, KrParams):
            raise KrError(f"parameter table: row {i} is not a KrParams")
        C.memmove(C.byref(arr, i * C.sizeof(KrParams)), C.byref(r), C.sizeof(KrParams))
    return arr, len(rows)


def param_table_check(base: KrParams, rows):
    """Host-only (no GPU): may ``rows`` (sequence of KrParams) ride in one launch with ``base``?  Returns
    ``(rc, bad_rod, message)``: rc 0, or KR_E_ARG / KR_E_UNSUPPORTED with the first offending row and the library's
    message, which names the field."""
    lib = load()
    arr, n = _params_array(rows)
    bad = _i64(-1)
    rc = lib.kr_param_table_check(C.byref(base), n, arr if n else None, C.byref(bad))
    msg = lib.kr_last_error() if rc else b""
    return rc, bad.value, msg.decode() if msg else ""


class ParamTable:
    """Owns one kr_param_table: row b = the parameters of rod b of ``Handle.simulate(..., table=...)``.  Immutable;
    usable as a context manager.  Close it only after the last call that uses it has finished on its stream."""

    def __init__(self, handle: "Handle", rows):
        self.lib = handle.lib
        arr, n = _params_array(rows)
        self.B = n
        self._t = _vp()
        check(self.lib.kr_param_table_create(handle._h, n, arr if n else None, C.byref(self._t)))

    def close(self):
        if getattr(self, "_t", None) is not None and self._t:
            self.lib.kr_param_table_destroy(self._t)
            self._t = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _on_device(x):
    return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))


def _bank_layer(x, k, on_device):
    """One weight or bias array of network k as the library reads it: a float32 host array, or - a bank of device
    sources - the contiguous float32 device tensor itself (never copied)."""
    if not on_device:
        if _on_device(x):
            raise KrError(f"network bank: network {k} holds a device tensor next to host arrays (one kind per bank)")
        return np.ascontiguousarray(x.detach().numpy() if hasattr(x, "detach") else x, dtype=np.float32)
    if not _on_device(x) or str(x.dtype) != "torch.float32" or not x.is_contiguous():
        raise KrError(f"network bank: network {k}: device sources are contiguous float32 device tensors, all of them")
    return x


def _bank_addr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _bank_shape(networks):
    """(dims, acts, per-network float32 arrays) of a sequence of (weights, biases, acts); every network must have the
    shape of the first.  Host only.  The arrays are host arrays or - all of them - device tensors, which are handed
    to the library where they lie."""
    nets = list(networks)
    if not nets:
        return [], [], []
    on_device = bool(nets[0][0]) and _on_device(nets[0][0][0])
    packed, dims0, acts0 = [], None, None
    for k, (weights, biases, acts) in enumerate(nets):
        Ws = [_bank_layer(w, k, on_device) for w in weights]
        bs = [_bank_layer(b, k, on_device) for b in biases]
        if not Ws or len(Ws) != len(bs) or len(Ws) != len(acts) or any(w.ndim != 2 for w in Ws):
            raise KrError(f"network bank: network {k}: malformed layer lists")
        dims = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
        for l in range(len(Ws)):
            if Ws[l].shape[1] != dims[l] or tuple(bs[l].shape) != (dims[l + 1],):
                raise KrError(f"network bank: network {k}, layer {l}: inconsistent shapes {tuple(Ws[l].shape)} / {tuple(bs[l].shape)}")
        acts = [int(a) for a in acts]
        if dims0 is None:
            dims0, acts0 = dims, acts
        elif dims != dims0 or acts != acts0:
            raise KrError(f"network bank: network {k} has layers {dims} / activations {acts}, network 0 {dims0} / {acts0} "
                          "(all networks of a bank share one shape)")
        packed.append((Ws, bs))
    return dims0, acts0, packed


def mlp_bank_check(base: KrParams, K: int, dims, acts):
    """Host-only (no GPU): is a bank of K networks with layer widths ``dims`` and activation codes ``acts`` served for
    rods like ``base``?  Returns ``(rc, message)``; the message names the rule."""
    lib = load()
    n = len(acts)
    dims_c = (C.c_int32 * max(len(dims), 1))(*[int(d) for d in dims])
    acts_c = (C.c_int32 * max(n, 1))(*[int(a) for a in acts])
    rc = lib.kr_mlp_bank_check(C.byref(base), int(K), n, dims_c, acts_c)
    msg = lib.kr_last_error() if rc else b""
    return rc, msg.decode() if msg else ""


class MlpBank:
    """Owns one kr_mlp_bank: K networks of one shape, ``networks[k] = (weights, biases, acts)`` as for
    ``Handle.set_mlp``; rod b of ``Handle.simulate(..., table=, bank=, net_of_rod=)`` evaluates network
    ``net_of_rod[b]``, and with ``bnd=`` / ``key_points=`` beside them the call takes per-step boundary data and
    writes key-point records too.  The arrays are host arrays or - all of them - float32 device tensors.  Changed only
    by ``repack``; usable as a context manager.  Close it only after the last call that uses it has finished on its
    stream."""

    def __init__(self, handle: "Handle", networks):
        self.lib = handle.lib
        self._handle = handle
        dims, acts, packed = _bank_shape(networks)
        self.K = len(packed)
        self.dims, self.acts = tuple(dims), tuple(acts)
        n = len(acts)
        dims_c = (C.c_int32 * max(len(dims), 1))(*dims)
        acts_c = (C.c_int32 * max(n, 1))(*acts)
        Wp, bp, on_device = self._sources(packed)
        self._b = _vp()
        # (the library has read the arrays, host or device, when create returns: `packed` need not outlive this call)
        check(self.lib.kr_mlp_bank_create(handle._h, self.K, n, dims_c, acts_c, Wp, bp, on_device, _stream(), C.byref(self._b)))

    def _sources(self, packed):
        n = len(self.acts)
        Wp = (_vp * max(self.K * n, 1))(*[_bank_addr(w) for Ws, _ in packed for w in Ws])
        bp = (_vp * max(self.K * n, 1))(*[_bank_addr(b) for _, bs in packed for b in bs])
        return Wp, bp, int(bool(packed) and _on_device(packed[0][0][0]))

    def repack(self, networks):
        """New weights for all K networks, in place: ``networks`` as for the constructor and of the bank's shape.  The
        result is bit-identical to a fresh bank.  Nothing is allocated; device tensors are read where they lie by
        launches ordered on the current stream (no synchronisation, no host copy) and must stay unchanged until those
        have run.  Calls queued behind it see the new weights."""
        if not self._b:
            raise KrError("network bank: repack of a closed bank")
        dims, acts, packed = _bank_shape(networks)
        if len(packed) != self.K or tuple(dims) != self.dims or tuple(acts) != self.acts:
            raise KrError(f"network bank: repack takes {self.K} networks of layers {list(self.dims)} / activations {list(self.acts)}; "
                          f"got {len(packed)} of {dims} / {acts}")
        Wp, bp, on_device = self._sources(packed)
        check(self.lib.kr_mlp_bank_repack(self._handle._h, self._b, Wp, bp, on_device, _stream()))
        return self

    def close(self):
        if getattr(self, "_b", None) is not None and self._b:
            self.lib.kr_mlp_bank_destroy(self._b)
            self._b = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# Handle.simulate, per kind of call: what it says beside bank= / net_of_rod=, beside loads=, and when what it needs is missing
_SIM_RULES = {
    "keypoints": (None,
                  "key_points= together with loads=: a key-point call takes bnd (its last six columns are the tip wrench)",
                  "a key-point call needs table= and bnd= (a caller with a fixed boundary repeats the rows' values)"),
    "boundary": (None,
                 "bnd= together with loads=: the last six columns of bnd are the tip wrench",
                 "a boundary call needs table= (a table of identical rows when only the boundary varies)"),
    "loads": ("loads= together with bank=: per-step tip loads ride with a network bank in bnd= (the last six columns of bnd are "
              "the tip wrench)", None,
              "a loads call needs table= (a table of identical rows when only the loads vary)"),
    "bank": (None, None, "a bank call needs table=, bank= and net_of_rod= together"),
}


class Handle:
    """Owns one kr_handle (one device, one parameter set)."""

    def __init__(self, params: KrParams, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise KrError("no HIP device visible: the rod solver runs on MI355X only (no CPU fallback)")
        self.lib = load()
        self.device = device
        torch.cuda.set_device(device)
        torch.cuda.current_stream()  # make sure torch's context exists on this device
        self._h = _vp()
        check(self.lib.kr_create(C.byref(params), device, C.byref(self._h)))
        self.N = params.N
        self._mlp_keep = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.kr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters --------------------------------------------------------
    def set_params(self, params: KrParams):
        check(self.lib.kr_set_params(self._h, C.byref(params)))
        self.N = params.N

    def derived(self) -> KrDerived:
        d = KrDerived()
        check(self.lib.kr_get_derived(self._h, C.byref(d)))
        return d

    def set_mlp(self, weights, biases, acts):
        """weights[k]: float32 [out, in] numpy arrays (nn.Linear layout)."""
        n = len(weights)
        if n == 0:
            check(self.lib.kr_set_mlp(self._h, 0, None, None, None, None, 0, _stream()))
            return
        Ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        bs = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
        dims = (C.c_int32 * (n + 1))(*([Ws[0].shape[1]] + [w.shape[0] for w in Ws]))
        for k in range(n):
            if Ws[k].shape[1] != dims[k] or bs[k].shape != (dims[k + 1],):
                raise KrError(f"MLP layer {k}: inconsistent shapes {Ws[k].shape} / {bs[k].shape}")
        acts_c = (C.c_int32 * n)(*[int(a) for a in acts])
        Wp = (_vp * n)(*[w.ctypes.data for w in Ws])
        bp = (_vp * n)(*[b.ctypes.data for b in bs])
        check(self.lib.kr_set_mlp(self._h, n, dims, acts_c, Wp, bp, 0, _stream()))

    def set_mlp_device(self, weights, biases, acts):
        """``set_mlp`` from float32 CUDA tensors (``kr_set_mlp`` with device sources, packed by one launch on the current
        stream).  The sources must stay valid and unmodified until that stream reaches the pack launch: keep the tensors
        alive and write to them on the same stream only."""
        import torch
        n = len(weights)
        for k in range(n):
            for t in (weights[k], biases[k]):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                    raise KrError(f"set_mlp_device: layer {k}: contiguous float32 CUDA tensors are needed")
        dims = (C.c_int32 * (n + 1))(*([weights[0].shape[1]] + [w.shape[0] for w in weights]))
        for k in range(n):
            if weights[k].dim() != 2 or weights[k].shape[1] != dims[k] or tuple(biases[k].shape) != (dims[k + 1],):
                raise KrError(f"MLP layer {k}: inconsistent shapes {tuple(weights[k].shape)} / {tuple(biases[k].shape)}")
        acts_c = (C.c_int32 * n)(*[int(a) for a in acts])
        Wp = (_vp * n)(*[w.data_ptr() for w in weights])
        bp = (_vp * n)(*[b.data_ptr() for b in biases])
        check(self.lib.kr_set_mlp(self._h, n, dims, acts_c, Wp, bp, 1, _stream()))

    # -- kernels -------------------------------------------------------------
    def ode_batch(self, y, yh, zh, tf, use_nn=False):
        import torch
        Q = y.shape[0]
        dys = torch.empty((Q, 19), dtype=y.dtype, device=y.device)
        z = torch.empty((Q, 6), dtype=y.dtype, device=y.device)
        check(self.lib.kr_ode_batch(self._h, Q, _ptr(y), _ptr(yh), _ptr(zh), _ptr(tf), _ptr(dys), _ptr(z),
                                    int(bool(use_nn)), dtype_code(y.dtype), _stream()))
        return dys, z

    def ode_vjp(self, y, yh, zh, tf, g_dys, g_z, cut=False, need=(True, True, True, True)):
        """J^T g of the physics of ``ode_batch`` with respect to (y, yh, zh, tf); entries not needed come back None."""
        import torch
        Q = y.shape[0]
        outs = [torch.empty((Q, n), dtype=y.dtype, device=y.device) if w else None for n, w in zip((19, 19, 6, 3), need)]
        check(self.lib.kr_ode_vjp_batch(self._h, Q, _ptr(y), _ptr(yh), _ptr(zh), _ptr(tf), _ptr(g_dys), _ptr(g_z),
                                        int(bool(cut)), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]),
                                        dtype_code(y.dtype), _stream()))
        return outs

    def ode_jacobian(self, y, yh, zh, tf, cut=False):
        """[Q, 25, 19] Jacobian d(dys, z) / dy of the physics of ``ode_batch``."""
        import torch
        Q = y.shape[0]
        jac = torch.empty((Q, 25, 19), dtype=y.dtype, device=y.device)
        check(self.lib.kr_ode_jacobian_batch(self._h, Q, _ptr(y), _ptr(yh), _ptr(zh), _ptr(tf), int(bool(cut)),
                                             _ptr(jac), dtype_code(y.dtype), _stream()))
        return jac

    def new_state(self, B, dtype, n_slots=1):
        import torch
        shape = (n_slots, B, self.N, KR_SLOTS) if n_slots > 1 else (B, self.N, KR_SLOTS)
        return torch.zeros(shape, dtype=dtype, device=f"cuda:{self.device}")

    def param_table(self, rows) -> ParamTable:
        return ParamTable(self, rows)

    def mlp_bank(self, networks) -> MlpBank:
        return MlpBank(self, networks)

    def init_straight(self, state, table=None):
        B = state.shape[0]
        if table is not None:  # rod b takes its length from row b
            if B != table.B:
                raise KrError(f"state holds {B} rods, the parameter table {table.B}")
            check(self.lib.kr_state_init_straight_table(self._h, table._t, _ptr(state), dtype_code(state.dtype), _stream()))
            return state
        check(self.lib.kr_state_init_straight(self._h, B, _ptr(state), dtype_code(state.dtype), _stream()))
        return state

    def pack(self, y_fm, z_fm, state=None):
        B = y_fm.shape[0]
        if state is None:
            state = self.new_state(B, y_fm.dtype)
        check(self.lib.kr_state_pack(self._h, B, _ptr(y_fm), _ptr(z_fm), _ptr(state), dtype_code(y_fm.dtype), _stream()))
        return state

    def unpack(self, state):
        import torch
        B = state.shape[0]
        y = torch.empty((B, 19, self.N), dtype=state.dtype, device=state.device)
        z = torch.empty((B, 6, self.N), dtype=state.dtype, device=state.device)
        check(self.lib.kr_state_unpack(self._h, B, _ptr(state), _ptr(y), _ptr(z), dtype_code(state.dtype), _stream()))
        return y, z

    def unpack50(self, state, m1, m2, out=None):
        import torch
        B = state.shape[0]
        if out is None:
            out = torch.empty((B, 50, self.N), dtype=state.dtype, device=state.device)
        check(self.lib.kr_state_unpack50(self._h, B, _ptr(state), _ptr(m1), _ptr(m2), _ptr(out),
                                         dtype_code(state.dtype), _stream()))
        return out

    def tip(self, state):
        import torch
        B = state.shape[0]
        out = torch.empty((B, 3), dtype=state.dtype, device=state.device)
        check(self.lib.kr_state_tip(self._h, B, _ptr(state), _ptr(out), dtype_code(state.dtype), _stream()))
        return out

    def residual(self, G, prev, cur, nxt, tensions, scheme=KR_EULER, use_nn=False, hist_is_explicit=False):
        import torch
        B = G.shape[0]
        r = torch.empty((B, 6), dtype=G.dtype, device=G.device)
        check(self.lib.kr_residual_batch(self._h, B, scheme, _ptr(G), _ptr(prev), _ptr(cur), _ptr(nxt), _ptr(tensions),
                                         _ptr(r), int(bool(use_nn)), int(bool(hist_is_explicit)),
                                         dtype_code(G.dtype), _stream()))
        return r

    def residual_mid(self, G, hist, hist_mid, nxt, tensions, scheme=KR_RK4, use_nn=False):
        """Residual sweep from explicit histories; ``hist_mid`` (may be None) = the caller's midpoint histories."""
        import torch
        B = G.shape[0]
        r = torch.empty((B, 6), dtype=G.dtype, device=G.device)
        check(self.lib.kr_residual_mid_batch(self._h, B, scheme, _ptr(G), _ptr(hist), _ptr(hist_mid), _ptr(nxt),
                                             _ptr(tensions), _ptr(r), int(bool(use_nn)), dtype_code(G.dtype), _stream()))
        return r

    def mlp_eval(self, x):
        import torch
        Q = x.shape[0]
        out = torch.empty((Q, 25), dtype=x.dtype, device=x.device)
        check(self.lib.kr_mlp_eval_batch(self._h, Q, _ptr(x), _ptr(out), dtype_code(x.dtype), _stream()))
        return out

    def mlp_input_jacobian(self, x):
        """``jac[Q, 25, 28]`` = dNN/dx of the handle's MLP at the rows ``x[Q, 28]`` (``kr_mlp_input_jacobian_batch``): fp64
        arithmetic on the matrix cores whatever the dtype of ``x``, which is that of the result."""
        import torch
        if x.dim() != 2 or x.shape[1] != 28 or x.shape[0] < 1:
            raise KrError(f"mlp_input_jacobian: x must be [Q, 28] with Q >= 1; got {tuple(x.shape)}")
        x = x.contiguous()
        jac = torch.empty((x.shape[0], 25, 28), dtype=x.dtype, device=x.device)
        check(self.lib.kr_mlp_input_jacobian_batch(self._h, x.shape[0], _ptr(x), _ptr(jac), dtype_code(x.dtype), _stream()))
        return jac

    def step(self, prev, cur, nxt, G, tensions, scheme=KR_EULER, tol=0.0, maxit=0, status=None, iters=None,
             use_nn=False, prev2=None, predictor=-1):
        B = G.shape[0]
        check(self.lib.kr_step_batch(self._h, B, scheme, _ptr(prev), _ptr(cur), _ptr(nxt), _ptr(G), _ptr(tensions),
                                     float(tol), int(maxit), _ptr(status), _ptr(iters), int(bool(use_nn)),
                                     _ptr(prev2), int(predictor), dtype_code(G.dtype), _stream()))

    def simulate_prepare(self, B, dtype):
        """One-time host work of the first ``simulate`` call for batches of B rods, ahead of time (launches nothing)."""
        check(self.lib.kr_simulate_prepare(self._h, int(B), dtype_code(dtype)))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        check(self.lib.kr_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_option(self, name: str, value: int):
        check(self.lib.kr_set_option(self._h, name.encode(), int(value)))

    def simulate(self, ctl, states, G, ring=False, tip=None, status=None, scheme=KR_EULER, tol=0.0, maxit=0,
                 use_nn=False, prev_init=None, table=None, bank=None, net_of_rod=None, loads=None, bnd=None, key_points=None,
                 kp=None):
        B, T = ctl.shape[0], ctl.shape[1]
        banked = bank is not None or net_of_rod is not None
        kind = ("keypoints" if key_points is not None or kp is not None else "boundary" if bnd is not None else
                "loads" if loads is not None else "bank" if banked else "table" if table is not None else "handle")
        # the exclusion rules and the shared checks, in the order a caller with two mistakes hears of them
        no_bank, no_loads, needs = _SIM_RULES.get(kind, (None, None, None))
        if no_bank and banked:
            raise KrError(no_bank)
        if no_loads and loads is not None:
            raise KrError(no_loads)
        # bnd= (and key_points= / kp=) beside a bank: kr_simulate_batch_bank_keypoints, checked as each part is alone
        with_bank = banked and kind in ("keypoints", "boundary")
        if with_bank and (bank is None or net_of_rod is None or not isinstance(bank, MlpBank)):
            raise KrError("bnd= / key_points= together with a bank need bank= (an MlpBank) and net_of_rod= together")
        if needs and (table is None or (kind == "keypoints" and bnd is None) or (kind == "bank" and (bank is None or net_of_rod is None))):
            raise KrError(needs)
        if kind == "keypoints" and (key_points is None or kp is None):
            raise KrError("a key-point call needs key_points= and kp= together")
        if table is not None and B != table.B:
            raise KrError(f"ctl holds {B} rods, the parameter table {table.B}")
        # rod b, step t: loads[b, t] = F_tip (3), M_tip (3), or bnd[b, t] = p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3),
        # in place of its row's
        name, hist, width = ("loads", loads, 6) if kind == "loads" else ("bnd", bnd, KR_BND)
        if kind in ("keypoints", "boundary", "loads") and (tuple(hist.shape) != (B, T, width) or hist.dtype != ctl.dtype or not hist.is_contiguous()):
            raise KrError(f"{name} must be a contiguous [{B}, {T}, {width}] tensor of {ctl.dtype}; got {tuple(hist.shape)} {hist.dtype}")
        if kind in ("keypoints", "bank"):
            idx = np.ascontiguousarray(np.asarray(key_points if kind == "keypoints" else net_of_rod).reshape(-1), dtype=np.int32)
            idx_p, K = idx.ctypes.data_as(C.POINTER(C.c_int32)), int(idx.size)
        if with_bank:  # rod b: row b of the table, network net_of_rod[b] of the bank
            nets = np.ascontiguousarray(np.asarray(net_of_rod).reshape(-1), dtype=np.int32)
            if nets.size != B:
                raise KrError(f"ctl holds {B} rods, net_of_rod {nets.size}")
        if kind == "keypoints" and (tuple(kp.shape) != (T, B, K, KR_SLOTS) or kp.dtype != ctl.dtype or not kp.is_contiguous()):
            # kp[t, b, k] receives the complete record of grid point key_points[k] of the state step t writes
            raise KrError(f"kp must be a contiguous [{T}, {B}, {K}, {KR_SLOTS}] tensor of {ctl.dtype}; got {tuple(kp.shape)} {kp.dtype}")
        if kind == "bank" and K != B:  # rod b: row b of the table, network net_of_rod[b] of the bank
            raise KrError(f"ctl holds {B} rods, net_of_rod {K}")
        # one argument list per kind around what all share
        lib, h, nn = self.lib, self._h, int(bool(use_nn))
        head = (T, scheme, _ptr(ctl))
        mid = (_ptr(states), int(bool(ring)), _ptr(G), _ptr(tip), float(tol), int(maxit), _ptr(status))
        end = (_ptr(prev_init), dtype_code(ctl.dtype), _stream())
        if kind == "handle":
            rc = lib.kr_simulate_batch(h, B, *head, *mid, nn, *end)
        elif kind == "table":  # rod b takes row b of the table instead of the handle's parameters
            rc = lib.kr_simulate_batch_table(h, table._t, *head, *mid, nn, *end)
        elif kind == "loads":
            rc = lib.kr_simulate_batch_loads(h, table._t, *head, _ptr(loads), *mid, nn, *end)
        elif with_bank:  # (a bank's networks are on: no use_nn; a boundary call is the key-point call with K = 0)
            points = (K, idx_p, _ptr(kp)) if kind == "keypoints" else (0, None, None)
            rc = lib.kr_simulate_batch_bank_keypoints(h, table._t, bank._b, nets.ctypes.data_as(C.POINTER(C.c_int32)), *head, _ptr(bnd),
                                                      *points, *mid, *end)
        elif kind == "boundary":
            rc = lib.kr_simulate_batch_boundary(h, table._t, *head, _ptr(bnd), *mid, nn, *end)
        elif kind == "keypoints":
            rc = lib.kr_simulate_batch_keypoints(h, table._t, *head, _ptr(bnd), K, idx_p, _ptr(kp), *mid, nn, *end)
        else:  # (a bank's networks are on: no use_nn)
            rc = lib.kr_simulate_batch_bank(h, table._t, bank._b, idx_p, *head, *mid, *end)
        check(rc)

    # -- gradients -----------------------------------------------------------------
    def _step_vjp_out(self, who, prev, cur, nxt, tensions, g_next, need_bnd, need_par=False, use_nn=False, need_rows=None):
        """The shape checks of a step adjoint (``who``: the method named in the messages) -> (B, the argument list the three C
        calls share, up to ``g_bnd``, and the dict of fresh outputs - with ``g_par`` under ``need_par``, with ``nn_x`` and
        ``nn_g`` where ``need_rows`` is not None)."""
        import torch
        B = cur.shape[0]
        for name, t in (("prev", prev), ("cur", cur), ("nxt", nxt), ("g_next", g_next)):
            if tuple(t.shape) != (B, self.N, KR_SLOTS) or t.dtype != cur.dtype:
                raise KrError(f"{who}: {name} must be [{B}, {self.N}, {KR_SLOTS}] of {cur.dtype}; got {tuple(t.shape)} {t.dtype}")
        if tuple(tensions.shape) != (B, 4) or tensions.dtype != cur.dtype:
            raise KrError(f"{who}: tensions must be [{B}, 4] of {cur.dtype}; got {tuple(tensions.shape)} {tensions.dtype}")
        new = lambda *shape, dtype=cur.dtype: torch.empty(shape, dtype=dtype, device=cur.device)
        out = dict(g_cur=new(B, self.N, KR_SLOTS), g_prev=new(B, self.N, KR_SLOTS), g_tensions=new(B, 4),
                   g_bnd=new(B, KR_BND) if need_bnd else None, resid=new(B, dtype=torch.float64), status=new(B, dtype=torch.int32))
        if need_par:
            if use_nn:
                raise KrError(f"{who}: need_par is served with the MLP off only (kr_{who}_par_batch)")
            out["g_par"] = new(B, KR_PAR)
        if need_rows is not None:
            out["nn_x"], out["nn_g"] = (new(B, self.N - 1, 32), new(B, self.N - 1, 32)) if need_rows else (None, None)
        head = (_ptr(prev), _ptr(cur), _ptr(nxt), _ptr(tensions), _ptr(g_next), _ptr(out["g_cur"]), _ptr(out["g_prev"]),
                _ptr(out["g_tensions"]), _ptr(out["g_bnd"]))
        return B, head, out

    def _simulate_vjp_out(self, who, ctl, states, g_states, prev_init, need_bnd, need_par=False, use_nn=False, need_rows=None):
        """The same for a rollout adjoint -> (B, T, the shared argument list up to ``g_bnd``, the dict of fresh outputs)."""
        import torch
        if ctl.dim() != 3 or ctl.shape[2] != 4 or ctl.shape[1] < 1:
            raise KrError(f"{who}: ctl must be [B, T, 4] with T >= 1; got {tuple(ctl.shape)}")
        B, T = ctl.shape[0], ctl.shape[1]
        for name, t in (("states", states), ("g_states", g_states)):
            if tuple(t.shape) != (T + 1, B, self.N, KR_SLOTS) or t.dtype != ctl.dtype:
                raise KrError(f"{who}: {name} must be the full history [{T + 1}, {B}, {self.N}, {KR_SLOTS}] of {ctl.dtype} (a "
                              f"ring of three states does not hold what the backward pass reads); got {tuple(t.shape)} {t.dtype}")
        if prev_init is not None and (tuple(prev_init.shape) != (B, self.N, KR_SLOTS) or prev_init.dtype != ctl.dtype):
            raise KrError(f"{who}: prev_init must be [{B}, {self.N}, {KR_SLOTS}] of {ctl.dtype}")
        new = lambda *shape, dtype=ctl.dtype: torch.empty(shape, dtype=dtype, device=ctl.device)
        out = dict(g_ctl=new(B, T, 4), g_bnd=new(B, KR_BND) if need_bnd else None,
                   g_prev_init=new(B, self.N, KR_SLOTS) if prev_init is not None else None,
                   resid=new(B, T, dtype=torch.float64), status=new(B, T, dtype=torch.int32))
        if need_par:
            if use_nn:
                raise KrError(f"{who}: need_par is served with the MLP off only (kr_{who}_par_batch)")
            out["g_par"] = new(B, KR_PAR)
        if need_rows is not None:
            out["nn_x"], out["nn_g"] = (new(T, B, self.N - 1, 32), new(T, B, self.N - 1, 32)) if need_rows else (None, None)
        head = (_ptr(ctl), _ptr(states), _ptr(prev_init), _ptr(g_states), _ptr(out["g_prev_init"]), _ptr(out["g_ctl"]), _ptr(out["g_bnd"]))
        return B, T, head, out

    def step_vjp(self, prev, cur, nxt, tensions, g_next, scheme=KR_EULER, use_nn=False, need_bnd=True, need_par=False):
        """Adjoint of one solved step (``kr_step_vjp_batch``): the cotangent ``g_next[B, N, KR_SLOTS]`` of ``nxt`` ->
        dict with ``g_cur``, ``g_prev`` ``[B, N, KR_SLOTS]``, ``g_tensions[B, 4]``, ``g_bnd[B, KR_BND]`` (None without
        ``need_bnd``), ``resid[B]`` (float64) and ``status[B]`` (int32), all on the device.  ``prev`` may be ``cur``.
        ``need_par``: the call goes through ``kr_step_vjp_par_batch`` (MLP off only) and the dict gains ``g_par[B, KR_PAR]``,
        the gradient of the rod's material parameters (``PAR_BLOCKS``; ``split_par``)."""
        B, head, out = self._step_vjp_out("step_vjp", prev, cur, nxt, tensions, g_next, need_bnd, need_par, use_nn)
        tail = (_ptr(out["resid"]), _ptr(out["status"]))
        if need_par:
            check(self.lib.kr_step_vjp_par_batch(self._h, B, scheme, *head, _ptr(out["g_par"]), *tail, dtype_code(cur.dtype), _stream()))
        else:
            check(self.lib.kr_step_vjp_batch(self._h, B, scheme, *head, *tail, int(bool(use_nn)), dtype_code(cur.dtype), _stream()))
        return out

    def simulate_vjp(self, ctl, states, g_states, prev_init=None, scheme=KR_EULER, use_nn=False, need_bnd=True, need_par=False):
        """Backward pass over a stored rollout (``kr_simulate_vjp_batch``): ``ctl[B, T, 4]``, the full history
        ``states[T + 1, B, N, KR_SLOTS]`` of the forward call (not a ring) and ``g_states`` of the same shape, in/out: the
        direct dL/dstates on entry, the total adjoint on return.  Returns dict with ``g_ctl[B, T, 4]``, ``g_bnd[B, KR_BND]``
        (None without ``need_bnd``), ``g_prev_init`` (None unless ``prev_init`` is given), ``resid[B, T]``, ``status[B, T]``.
        ``need_par``: the call goes through ``kr_simulate_vjp_par_batch`` (MLP off only) and the dict gains
        ``g_par[B, KR_PAR]``, the gradient of the rod's material parameters summed over the steps."""
        B, T, head, out = self._simulate_vjp_out("simulate_vjp", ctl, states, g_states, prev_init, need_bnd, need_par, use_nn)
        tail = (_ptr(out["resid"]), _ptr(out["status"]))
        if need_par:
            check(self.lib.kr_simulate_vjp_par_batch(self._h, B, T, scheme, *head, _ptr(out["g_par"]), *tail, dtype_code(ctl.dtype),
                                                     _stream()))
        else:
            check(self.lib.kr_simulate_vjp_batch(self._h, B, T, scheme, *head, *tail, int(bool(use_nn)), dtype_code(ctl.dtype), _stream()))
        return out

    def step_vjp_table(self, table, prev, cur, nxt, tensions, g_next, need_bnd=True, need_par=False):
        """``step_vjp`` of a heterogeneous batch (``kr_step_vjp_table_batch``, MLP off): rod b takes row b of ``table`` (a
        ``ParamTable`` of B rows) in place of the handle's parameters.  The same dict; ``g_par[B, KR_PAR]`` with ``need_par``
        is the gradient of row b's parameters.  ``g_bnd[b]`` is the gradient with respect to the boundary values rod b's
        step used (record 0 of ``nxt`` holds them), whether they came from its row, a ``loads=`` or a ``bnd=`` history."""
        if table is None or not isinstance(table, ParamTable):
            raise KrError("step_vjp_table: table must be a ParamTable")
        if cur.shape[0] != table.B:
            raise KrError(f"step_vjp_table: cur holds {cur.shape[0]} rods, the parameter table {table.B}")
        B, head, out = self._step_vjp_out("step_vjp_table", prev, cur, nxt, tensions, g_next, need_bnd, need_par)
        check(self.lib.kr_step_vjp_table_batch(self._h, table._t, KR_EULER, *head, _ptr(out.get("g_par")), _ptr(out["resid"]),
                                               _ptr(out["status"]), dtype_code(cur.dtype), _stream()))
        return out

    def simulate_vjp_table(self, table, ctl, states, g_states, prev_init=None, need_bnd=True, bnd_per_step=False, need_par=False):
        """``simulate_vjp`` of a heterogeneous batch (``kr_simulate_vjp_table_batch``, MLP off): rod b takes row b of
        ``table``.  The same dict; ``g_bnd`` is ``[B, KR_BND]``, summed over the steps, or - ``bnd_per_step`` -
        ``[B, T, KR_BND]``: entry ``[b, t]`` is the gradient with respect to ``bnd[b, t]`` of ``simulate(..., bnd=)``, its
        last six columns with respect to ``loads[b, t]`` of ``simulate(..., loads=)``.  ``g_par[B, KR_PAR]`` is per rod."""
        import torch
        if table is None or not isinstance(table, ParamTable):
            raise KrError("simulate_vjp_table: table must be a ParamTable")
        if ctl.dim() == 3 and ctl.shape[0] != table.B:
            raise KrError(f"simulate_vjp_table: ctl holds {ctl.shape[0]} rods, the parameter table {table.B}")
        B, T, head, out = self._simulate_vjp_out("simulate_vjp_table", ctl, states, g_states, prev_init, need_bnd, need_par)
        if need_bnd and bnd_per_step:
            out["g_bnd"] = torch.empty((B, T, KR_BND), dtype=ctl.dtype, device=ctl.device)
            head = head[:-1] + (_ptr(out["g_bnd"]),)
        check(self.lib.kr_simulate_vjp_table_batch(self._h, table._t, T, KR_EULER, *head, int(bool(bnd_per_step)), _ptr(out.get("g_par")),
                                                   _ptr(out["resid"]), _ptr(out["status"]), dtype_code(ctl.dtype), _stream()))
        return out

    def step_vjp_nn(self, prev, cur, nxt, tensions, g_next, scheme=KR_EULER, need_bnd=True, need_rows=True):
        """``step_vjp`` for the model with the handle's MLP on (``kr_step_vjp_nn_batch``): the same dict, plus ``nn_x``,
        ``nn_g`` ``[B, N - 1, 32]`` (None without ``need_rows``) - the network's input at every stored point and the
        cotangent that reaches its output there, the rows of the weight gradient."""
        B, head, out = self._step_vjp_out("step_vjp_nn", prev, cur, nxt, tensions, g_next, need_bnd, need_rows=bool(need_rows))
        check(self.lib.kr_step_vjp_nn_batch(self._h, B, scheme, *head, _ptr(out["resid"]), _ptr(out["status"]), _ptr(out["nn_x"]),
                                            _ptr(out["nn_g"]), dtype_code(cur.dtype), _stream()))
        return out

    def simulate_vjp_nn(self, ctl, states, g_states, prev_init=None, scheme=KR_EULER, need_bnd=True, need_rows=True):
        """``simulate_vjp`` for the model with the handle's MLP on (``kr_simulate_vjp_nn_batch``): the same dict, plus
        ``nn_x``, ``nn_g`` ``[T, B, N - 1, 32]`` (None without ``need_rows``), the rows of the weight gradient per step."""
        B, T, head, out = self._simulate_vjp_out("simulate_vjp_nn", ctl, states, g_states, prev_init, need_bnd, need_rows=bool(need_rows))
        check(self.lib.kr_simulate_vjp_nn_batch(self._h, B, T, scheme, *head, _ptr(out["resid"]), _ptr(out["status"]), _ptr(out["nn_x"]),
                                                _ptr(out["nn_g"]), dtype_code(ctl.dtype), _stream()))
        return out

    def _bank_args(self, who, table, bank, net_of_rod, B):
        """The checks the two bank adjoints share -> the int32 index array (kept alive by the caller) and its pointer."""
        if table is None or not isinstance(table, ParamTable):
            raise KrError(f"{who}: table must be a ParamTable")
        if bank is None or not isinstance(bank, MlpBank) or net_of_rod is None:
            raise KrError(f"{who}: bank must be an MlpBank, with net_of_rod")
        if B != table.B:
            raise KrError(f"{who}: the states hold {B} rods, the parameter table {table.B}")
        nets = np.ascontiguousarray(np.asarray(net_of_rod).reshape(-1), dtype=np.int32)
        if nets.size != B:
            raise KrError(f"{who}: the states hold {B} rods, net_of_rod {nets.size}")
        return nets, nets.ctypes.data_as(C.POINTER(C.c_int32))

    def step_vjp_bank(self, table, bank, net_of_rod, prev, cur, nxt, tensions, g_next, scheme=KR_EULER, need_bnd=True, need_rows=True):
        """``step_vjp_nn`` of a heterogeneous batch (``kr_step_vjp_bank_batch``): rod b takes row b of ``table`` and network
        ``net_of_rod[b]`` of ``bank`` (an ``MlpBank``) in place of the handle's parameters and network.  The dict of
        ``step_vjp_nn``; ``nn_x``, ``nn_g`` ``[B, N - 1, 32]`` are in rod order - the rows of network k's weight gradient are
        those of the rods with ``net_of_rod[b] == k``."""
        nets, nets_p = self._bank_args("step_vjp_bank", table, bank, net_of_rod, cur.shape[0])
        B, head, out = self._step_vjp_out("step_vjp_bank", prev, cur, nxt, tensions, g_next, need_bnd, need_rows=bool(need_rows))
        check(self.lib.kr_step_vjp_bank_batch(self._h, table._t, bank._b, nets_p, scheme, *head, _ptr(out["resid"]), _ptr(out["status"]),
                                              _ptr(out["nn_x"]), _ptr(out["nn_g"]), dtype_code(cur.dtype), _stream()))
        return out

    def simulate_vjp_bank(self, table, bank, net_of_rod, ctl, states, g_states, prev_init=None, scheme=KR_EULER, need_bnd=True,
                          bnd_per_step=False, need_rows=True):
        """``simulate_vjp_nn`` of a heterogeneous batch (``kr_simulate_vjp_bank_batch``): the backward side of
        ``simulate(..., bank=, net_of_rod=)`` without and with ``bnd=``.  The dict of ``simulate_vjp_nn``; ``g_bnd`` is
        ``[B, KR_BND]``, summed over the steps, or - ``bnd_per_step`` - ``[B, T, KR_BND]`` as in ``simulate_vjp_table``;
        ``nn_x``, ``nn_g`` ``[T, B, N - 1, 32]`` are in rod order."""
        import torch
        B, T, head, out = self._simulate_vjp_out("simulate_vjp_bank", ctl, states, g_states, prev_init, need_bnd, need_rows=bool(need_rows))
        nets, nets_p = self._bank_args("simulate_vjp_bank", table, bank, net_of_rod, B)
        if need_bnd and bnd_per_step:
            out["g_bnd"] = torch.empty((B, T, KR_BND), dtype=ctl.dtype, device=ctl.device)
            head = head[:-1] + (_ptr(out["g_bnd"]),)
        check(self.lib.kr_simulate_vjp_bank_batch(self._h, table._t, bank._b, nets_p, T, scheme, *head, int(bool(bnd_per_step)),
                                                  _ptr(out["resid"]), _ptr(out["status"]), _ptr(out["nn_x"]), _ptr(out["nn_g"]),
                                                  dtype_code(ctl.dtype), _stream()))
        return out

    # -- evaluation metrics ------------------------------------------------------
    def dtw(self, a, b, out=None):
        """Exact DTW distance (L1 point distance) of every rod's path ``a[b]`` to ``b[b]``: device tensors ``[B, Ta, 3]`` and
        ``[B, Tb, 3]`` or ``[Tb, 3]`` (one path for all rods) of one dtype; views are read in place through their strides -
        ``states[:T, :, j, 12:15].permute(1, 0, 2)`` is grid point j of a state history, ``tip`` the tip path of
        ``simulate``.  Returns float64 ``[B]`` on the device; bit-identical to ``krod_eval.dtw_distance`` per rod."""
        import torch
        if a.dim() != 3:
            raise KrError(f"dtw: sequence a must be [B, Ta, 3]; got {tuple(a.shape)}")
        if a.dtype != b.dtype:
            raise KrError(f"dtw: a is {a.dtype}, b {b.dtype}")
        B = a.shape[0]
        ars, ass, Ta = _dtw_view(a, B, "a")
        brs, bss, Tb = _dtw_view(b, B, "b")
        if out is None:
            out = torch.empty((B,), dtype=torch.float64, device=a.device)
        check(self.lib.kr_dtw_batch(self._h, B, C.c_void_p(a.data_ptr()), Ta, ars, ass, C.c_void_p(b.data_ptr()), Tb, brs, bss,
                                    _ptr(out), dtype_code(a.dtype), _stream()))
        return out

    def fastdtw(self, a, b, radius=1, path=False, out=None):
        """FastDTW distance (L1 point distance, ``radius``) of every rod's path ``a[b]`` to ``b[b]`` - the reference's
        ``fastdtw(a, b)[0]`` at radius 1: the sequences are given as for ``dtw`` (views are read in place).  Returns float64
        ``[B]`` on the device, bit-identical to ``krod_eval.fastdtw_distance`` per rod; a rod with a non-finite sample gets NaN.
        ``path=True``: ``(dist, path, path_len)`` with ``path`` int32 ``[B, Ta + Tb - 1, 2]``, the level-0 warp path of rod b
        in its first ``path_len[b]`` entries (``krod_eval.fastdtw_path``; the rest is zero here).  The workspace is allocated
        here (``kr_fastdtw_ws_bytes``)."""
        import torch
        if a.dim() != 3:
            raise KrError(f"fastdtw: sequence a must be [B, Ta, 3]; got {tuple(a.shape)}")
        if a.dtype != b.dtype:
            raise KrError(f"fastdtw: a is {a.dtype}, b {b.dtype}")
        B = a.shape[0]
        ars, ass, Ta = _dtw_view(a, B, "a")
        brs, bss, Tb = _dtw_view(b, B, "b")
        radius = int(radius)
        if out is None:
            out = torch.empty((B,), dtype=torch.float64, device=a.device)
        steps = plen = None
        if path:
            steps = torch.zeros((B, Ta + Tb - 1, 2), dtype=torch.int32, device=a.device)
            plen = torch.zeros((B,), dtype=torch.int32, device=a.device)
        nbytes = int(self.lib.kr_fastdtw_ws_bytes(B, Ta, Tb, radius))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=a.device) if nbytes else None
        check(self.lib.kr_fastdtw_batch(self._h, B, C.c_void_p(a.data_ptr()), Ta, ars, ass, C.c_void_p(b.data_ptr()), Tb, brs, bss,
                                        radius, _ptr(out), _ptr(steps), _ptr(plen), _ptr(ws), dtype_code(a.dtype), _stream()))
        return (out, steps, plen) if path else out

    def softdtw(self, a, b, gamma, cost="l1", grad=False, g_out=None):
        """Soft-DTW of every rod's path ``a[b]`` to ``b[b]`` (``kr_softdtw_batch``; ``krod_eval.softdtw_grad`` is its
        statement): the sequences are given as for ``dtw`` (views are read in place), ``cost`` is ``"l1"`` (the metric's own
        point distance) or ``"sq"``.  Returns ``value``, float64 ``[B]`` on the device; with ``grad=True`` or a ``g_out``
        ``(value, g_a)``, ``g_a[B, Ta, 3]`` = d value[b] / d a[b] in the dtype of ``a``.  ``g_out``: a ``[B, Ta, 3]`` view
        the gradient is WRITTEN into through its strides (3 adjacent components; nothing else of its storage is touched) -
        ``g[1:, :, N - 1, 12:15].permute(1, 0, 2)`` of a zeroed ``g[T + 1, B, N, KR_SLOTS]`` seeds ``simulate_vjp*`` with
        the loss's cotangent in the same launch.  A rod with a non-finite sample gets NaN in both.  The workspace is
        allocated here (``kr_softdtw_ws_bytes``)."""
        import torch
        if a.dim() != 3:
            raise KrError(f"softdtw: sequence a must be [B, Ta, 3]; got {tuple(a.shape)}")
        if a.dtype != b.dtype:
            raise KrError(f"softdtw: a is {a.dtype}, b {b.dtype}")
        B = a.shape[0]
        ars, ass, Ta = _dtw_view(a, B, "a")
        brs, bss, Tb = _dtw_view(b, B, "b")
        gamma, code = softdtw_args(gamma, cost, Ta, Tb)
        want = bool(grad) or g_out is not None
        grs = gss = 0
        if want:
            if g_out is None:
                g_out = torch.empty((B, Ta, 3), dtype=a.dtype, device=a.device)
            if not g_out.is_cuda or g_out.device != a.device or g_out.dtype != a.dtype or tuple(g_out.shape) != (B, Ta, 3):
                raise KrError(f"softdtw: g_out must be a [{B}, {Ta}, 3] view of {a.dtype} on {a.device}; got "
                              f"{tuple(g_out.shape)} of {g_out.dtype} on {g_out.device}")
            grs, gss, comp = g_out.stride()
            # (a stride torch leaves arbitrary for an extent of 1 is not used by the kernel either)
            grs, gss = (grs if B > 1 else max(grs, 1)), (gss if Ta > 1 else max(gss, 1))
            if comp != 1 or grs <= 0 or gss <= 0:
                raise KrError(f"softdtw: g_out: the 3 components must be adjacent and the strides > 0 (strides {g_out.stride()})")
        value = torch.empty((B,), dtype=torch.float64, device=a.device)
        nbytes = int(self.lib.kr_softdtw_ws_bytes(B, Ta, Tb, int(want)))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=a.device) if nbytes else None
        check(self.lib.kr_softdtw_batch(self._h, B, C.c_void_p(a.data_ptr()), Ta, ars, ass, C.c_void_p(b.data_ptr()), Tb, brs, bss,
                                        gamma, code, _ptr(value), C.c_void_p(g_out.data_ptr()) if want else None, grs, gss,
                                        _ptr(ws), dtype_code(a.dtype), _stream()))
        return (value, g_out) if want else value

    def pose_mse(self, states, ref_states):
        """Position + zyx-Euler MSE x 1000 of every rod over packed states ``[T, B, N, KR_SLOTS]`` (the first T slots of a
        state history) against ``ref_states`` ``[T, B, N, KR_SLOTS]`` or ``[T, 1, N, KR_SLOTS]`` (one reference for all rods).
        Returns ``(mse[B], parts[B, 2])``, float64 on the device; parts = the position and the Euler sum of squares."""
        import torch
        if states.dim() != 4 or ref_states.dim() != 4 or states.shape[2:] != (self.N, KR_SLOTS) or \
                ref_states.shape[2:] != (self.N, KR_SLOTS) or ref_states.shape[0] != states.shape[0]:
            raise KrError(f"pose_mse: states {tuple(states.shape)} / ref_states {tuple(ref_states.shape)}: expected "
                          f"[T, B, {self.N}, {KR_SLOTS}] and [T, B or 1, {self.N}, {KR_SLOTS}]")
        if states.dtype != ref_states.dtype:
            raise KrError(f"pose_mse: states are {states.dtype}, ref_states {ref_states.dtype}")
        T, B = states.shape[0], states.shape[1]
        mse = torch.empty((B,), dtype=torch.float64, device=states.device)
        parts = torch.empty((B, 2), dtype=torch.float64, device=states.device)
        check(self.lib.kr_pose_mse_batch(self._h, B, T, _ptr(states), _ptr(ref_states), ref_states.shape[1], _ptr(mse),
                                         _ptr(parts), dtype_code(states.dtype), _stream()))
        return mse, parts

    def pose_mse_points(self, records, ref_records):
        """``pose_mse`` over P records per rod and step instead of the handle's N grid points: ``records`` ``[T, B, P, KR_SLOTS]``
        (the ``kp`` of a key-point call) against ``ref_records`` ``[T, B or 1, P, KR_SLOTS]``, both contiguous.  Returns
        ``(mse[B], parts[B, 2])``, float64 on the device."""
        import torch
        if records.dim() != 4 or ref_records.dim() != 4 or records.shape[3] != KR_SLOTS or \
                ref_records.shape[2:] != records.shape[2:] or ref_records.shape[0] != records.shape[0]:
            raise KrError(f"pose_mse_points: records {tuple(records.shape)} / ref_records {tuple(ref_records.shape)}: expected "
                          f"[T, B, P, {KR_SLOTS}] and [T, B or 1, P, {KR_SLOTS}]")
        if records.dtype != ref_records.dtype:
            raise KrError(f"pose_mse_points: records are {records.dtype}, ref_records {ref_records.dtype}")
        if not records.is_contiguous() or not ref_records.is_contiguous():
            raise KrError("pose_mse_points: records and ref_records must be contiguous")
        T, B, P = records.shape[0], records.shape[1], records.shape[2]
        mse = torch.empty((B,), dtype=torch.float64, device=records.device)
        parts = torch.empty((B, 2), dtype=torch.float64, device=records.device)
        check(self.lib.kr_pose_mse_points_batch(self._h, B, T, P, _ptr(records), _ptr(ref_records), ref_records.shape[1], _ptr(mse),
                                                _ptr(parts), dtype_code(records.dtype), _stream()))
        return mse, parts

    def pack_poses(self, traj, dtype):
        """Host trajectories ``[R, T, >=7, N]`` (reference row order: p, h, ...) as packed states ``[T, R, N, KR_SLOTS]`` of
        ``dtype`` on the device, by one ``kr_state_pack``; rows a trajectory does not have are zero."""
        import torch
        traj = np.asarray(traj, dtype=np.float64)
        R, T, rows, N = traj.shape
        full = np.zeros((T, R, 25, N))
        full[:, :, :min(rows, 25)] = traj.transpose(1, 0, 2, 3)[:, :, :25]
        dev = f"cuda:{self.device}"
        y = torch.as_tensor(np.ascontiguousarray(full[:, :, :19].reshape(T * R, 19, N)), device=dev).to(dtype).contiguous()
        z = torch.as_tensor(np.ascontiguousarray(full[:, :, 19:].reshape(T * R, 6, N)), device=dev).to(dtype).contiguous()
        return self.pack(y, z).reshape(T, R, N, KR_SLOTS)
