"""ctypes binding of libwaveflow_hip.so (include/waveflow_hip.h).  No fallback: if the library
is missing or a call fails, an exception is raised."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "libwaveflow_hip.so")
# WF_LIB: experiment builds under scratch/variants only (A/B timing scripts).  It is honoured only together with WF_LIB_EXPERIMENT=1 and the
# loaded path is reported on stderr: tests/conftest.py builds and validates the default library, nothing else.
if os.environ.get("WF_LIB") and os.environ.get("WF_LIB_EXPERIMENT") != "1":
    raise ImportError("WF_LIB is set without WF_LIB_EXPERIMENT=1: refusing to load a library other than " + DEFAULT_LIB)
LIB_PATH = os.environ.get("WF_LIB") or DEFAULT_LIB

WF_MAX_DIM, WF_MAX_BC = 16, 4
SPLINE_M, SPLINE_I, SPLINE_B, SPLINE_OB = 0, 1, 2, 3
LAYER_IMADE, LAYER_MADE, LAYER_NSC = 0, 1, 2
BOX_NONE, BOX_MEAN, BOX_FIRST = 0, 1, 2
PRIOR_WAVEFLOW, PRIOR_MFLOW, PRIOR_UNIFORM, PRIOR_NORMAL = 0, 1, 2, 3
KERNEL_AUTO, KERNEL_SCALAR, KERNEL_MFMA, KERNEL_WAVE = 0, 1, 2, 3
ERR_NO_DEVICE = -4
ERR_UNSUPPORTED = -2


class WfError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        L = lib()
        msg = L.wf_strerror(status).decode()
        if status == -3:
            msg += ": " + L.wf_last_hip_error_string().decode()
        super().__init__(f"{what}: {msg} (status {status})")


class BC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("n_derivative", ctypes.c_int32 * WF_MAX_BC), ("value", ctypes.c_float * WF_MAX_BC)]

    @classmethod
    def from_dict(cls, d):
        bc = cls()
        d = {} if d is None else d
        if len(d) > WF_MAX_BC:
            raise ValueError("at most %d boundary constraints per side" % WF_MAX_BC)
        bc.n = len(d)
        for i, (nd, v) in enumerate(d.items()):
            bc.n_derivative[i] = int(nd)
            bc.value[i] = float(v)
        return bc


class ModelDesc(ctypes.Structure):
    _fields_ = [("n_dim", ctypes.c_int32), ("hidden", ctypes.c_int32), ("n_flow_layers", ctypes.c_int32),
                ("layer_kind", ctypes.c_int32), ("box_kind", ctypes.c_int32), ("box_size", ctypes.c_float),
                ("i_degree", ctypes.c_int32), ("i_knots", ctypes.c_int32), ("i_reg", ctypes.c_float),
                ("i_left", BC), ("i_right", BC), ("prior_kind", ctypes.c_int32), ("p_degree", ctypes.c_int32),
                ("p_knots", ctypes.c_int32), ("p_left", BC), ("p_right", BC), ("normal_offset", ctypes.c_float),
                ("n_constrained_left", ctypes.c_int32), ("constrained_left", ctypes.c_int32 * WF_MAX_DIM),
                ("n_mesh", ctypes.c_int32), ("i_reverse_tol", ctypes.c_float), ("i_gate", ctypes.c_int32), ("p_gate", ctypes.c_int32),
                ("nsc_bins", ctypes.c_int32), ("nsc_tail_bound", ctypes.c_float), ("nsc_hidden", ctypes.c_int32), ("nsc_reverse", ctypes.c_int32)]


class SplineDesc(ctypes.Structure):
    """wf_spline_desc (include/waveflow_hip.h)"""
    _fields_ = [("kind", ctypes.c_int32), ("degree", ctypes.c_int32), ("n_internal_knots", ctypes.c_int32), ("n_mesh", ctypes.c_int32),
                ("zero_border", ctypes.c_int32), ("left", BC), ("right", BC)]


class TrainState(ctypes.Structure):
    """wf_train_state (include/waveflow_hip.h)"""
    _fields_ = [("params_dev", ctypes.c_void_p), ("m_dev", ctypes.c_void_p), ("v_dev", ctypes.c_void_p), ("counter_dev", ctypes.c_void_p),
                ("running_average_dev", ctypes.c_void_p), ("loss_ring_dev", ctypes.c_void_p), ("ring_len", ctypes.c_int32), ("defer_eval_tables", ctypes.c_int32)]


_vp, _i32, _i64, _u64, _f32, _str = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_char_p
_ws = [_vp, _i64]          # (workspace_dev, workspace_bytes)
_adam = [_f32] * 4         # (step_size, b1, b2, eps)
_state = ctypes.POINTER(TrainState)
# name -> (restype, argtypes): every function of include/waveflow_hip.h, in its order (tests/test_abi_host.py holds the two against each other)
PROTOTYPES = {
    "wf_tables_build": (_i32, [_i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "wf_strerror": (_str, [_i32]),
    "wf_abi_version": (_i32, []),
    "wf_last_hip_error": (_i32, []),
    "wf_last_hip_error_string": (_str, []),
    "wf_device_count": (_i32, []),
    "wf_model_create": (_i32, [ctypes.POINTER(ModelDesc), _i32, ctypes.POINTER(_vp)]),
    "wf_model_destroy": (None, [_vp]),
    "wf_model_param_count": (_i64, [_vp]),
    "wf_model_n_bases": (_i32, [_vp, _i32]),
    "wf_model_set_params": (_i32, [_vp, _vp, _i64, _vp]),
    "wf_model_set_params_device": (_i32, [_vp, _vp, _i64, _vp]),
    "wf_adam_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64] + _adam + [_vp]),
    "wf_model_set_kernel": (_i32, [_vp, _i32]),
    "wf_logpdf_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "wf_psi_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "wf_psi_antisym_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "wf_logpdf_unsorted_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "wf_inversion_count": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "wf_flow_fwd": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "wf_layer_fwd": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "wf_inverse_fwd": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp]),
    "wf_sample": (_i32, [_vp, _u64, _i64, _vp, _vp, _i32, _vp]),
    "wf_hamiltonian_fwd": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "wf_psi_coord_derivs": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "wf_psi_vjp_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_psi_vjp": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp] + _ws + [_vp]),
    "wf_vqmc_loss_grad": (_i32, [_vp, _vp, _i64, _vp, _i32, _f32, _f32, _vp, _vp] + _ws + [_vp]),
    "wf_vqmc_train_step_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_vqmc_train_step": (_i32, [_vp, _state, _u64, _i64, _vp, _i32] + _adam + [_i32] + _ws + [_vp]),
    "wf_vqmc_train_step_local": (_i32, [_vp, _state, _u64, _i64, _vp, _i32, _f32, _i32, _vp] + _ws + [_vp]),
    "wf_vqmc_train_step_apply": (_i32, [_vp, _state, _vp] + _adam + [_vp]),
    "wf_mle_train_step_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_mle_train_step": (_i32, [_vp, _state, _vp, _i64] + _adam + _ws + [_vp]),
    "wf_logpdf_vjp_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_logpdf_vjp": (_i32, [_vp, _vp, _i64, _vp, _vp] + _ws + [_vp]),
    "wf_logpdf_jac_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_logpdf_jac": (_i32, [_vp, _vp, _i64, _vp, _vp] + _ws + [_vp]),
    "wf_psi_jac_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_psi_jac": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp] + _ws + [_vp]),
    "wf_logpdf_loss_grad": (_i32, [_vp, _vp, _i64, _f32, _vp, _vp] + _ws + [_vp]),
    "wf_vqmc_seeds": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp]),
    "wf_rqs_fwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "wf_nsc_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "wf_nsc_fwd": (_i32, [_vp, _i64, _i32, _i32, _f32, _i32, _vp, _i32, _vp, _vp] + _ws + [_vp]),
    "wf_block_sums": (_i32, [_vp, _i64, _vp] + _ws + [_vp]),
    "wf_block_sums_workspace_bytes": (_i64, [_i64]),
    "wf_spline_create": (_i32, [ctypes.POINTER(SplineDesc), _vp, _vp, _i32, ctypes.POINTER(_vp)]),
    "wf_spline_destroy": (None, [_vp]),
    "wf_spline_n_bases": (_i32, [_vp]),
    "wf_spline_apply": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "wf_spline_reverse": (_i32, [_vp, _vp, _i64, _vp, _f32, _vp, _vp]),
    "wf_spline_enforce_bc": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "wf_spline_remove_bias": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "wf_spline_sample": (_i32, [_vp, _u64, _vp, _i64, _i32, _i32, _vp, _vp]),
}
EXPORTS = list(PROTOTYPES)

_lib = None
# (handle, ids of the prototype tables applied to it).  An id names a table only while the table lives: the tables are the modules' PROTOTYPES
# dicts, which live as long as the process -- pass no temporary dict to bound(), its id can be handed out again
_bound = None


def _apply(L, table):
    for name, (restype, argtypes) in table.items():
        f = getattr(L, name)
        f.restype = restype
        f.argtypes = argtypes


def bound(*tables):
    """The handle of lib() with these prototype tables (a module's PROTOTYPES: one table per header of include/) applied to it, each once
    per handle.  Every module's lib() is one call of this."""
    global _bound
    L = lib()
    if _bound is None or _bound[0] is not L:
        _bound = (L, set())
    for table in tables:
        if id(table) not in _bound[1]:
            _apply(L, table)
            _bound[1].add(id(table))
    return L


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built; run `python -m waveflow_amd.build` (hipcc, gfx950). "
                          "There is no CPU fallback.")
    # PyTorch ships its own libamdhip64.so.7; importing torch first makes this library bind to that same
    # HIP runtime (one runtime per process: streams and device pointers are shared with torch).
    import torch  # noqa: F401
    if LIB_PATH != DEFAULT_LIB:
        import sys
        print(f"waveflow_amd: experiment library {LIB_PATH}", file=sys.stderr)
    L = ctypes.CDLL(LIB_PATH)
    _apply(L, PROTOTYPES)
    if L.wf_abi_version() != 2:
        raise ImportError("libwaveflow_hip ABI version mismatch")
    _lib = L
    return L


def check(status, what):
    if status < 0:
        raise WfError(status, what)
    return status


def call(name, *args):
    """One library call, checked: the entry's status or value (a byte count, a basis count), WfError when it is negative."""
    return check(getattr(lib(), name)(*args), name)


def ptr(t):
    """Device pointer of a torch tensor; NULL for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def stream_ptr(device=None):
    """torch's current HIP stream on `device` (default: the current device) as the `stream` argument."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
