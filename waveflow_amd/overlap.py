"""Overlaps between wavefunctions, measured on the device: the ctypes surface of include/waveflow_overlap.h (PROTOTYPES, OverlapAcc), the
device-side `Accumulator`, the host-side `Totals`, and `accumulate`, `penalise`, `measure` and `overlap_matrix` on top of them.

A Waveflow psi is normalised by construction, so on walkers x ~ |psi|^2 from psi's own exact sampler S_k = <psi_k|psi> = E[psi_k(x) / psi(x)]
is a one-sided estimator of variance 1 - S_k^2: the library forms r_k = psi_k / (psi + 1e-8) per walker in fp32 and keeps fp64 sums of r_k and
r_k^2 and two counters -- on the device, over any number of steps.  The sums are bitwise reproducible (their order depends on the batch size
alone; no floating-point atomics), so `Totals` of two runs can be compared, merged and all-reduced exactly.

`penalise` turns local energies into those of the penalty method L = E[psi] + sum_k lambda_k S_k^2, whose gradient is 2 E[(e~ - mean e~) O]
with e~_b = e_b + sum_k lambda_k a_k (r_kb - a_k), a_k the batch mean of r_k: what vqmc.sr_natural_gradient and vqmc.spring_direction hand to
their solvers when they are given lower states.

`reference_accumulate` and `reference_penalise` restate the two kernels in numpy (fp32 per operation, fp64 sums in the documented order): they
are what the GPU tests hold the library to.

Everything else runs on the GPU that holds the operands, on torch's current stream; there is no CPU fallback, and arguments are checked before
anything is launched (ValueError).
"""
import ctypes

import numpy as np

from . import _accum, _lib
from ._accum import BLOCK, GRID_BLOCKS   # noqa: F401  (the capped grid of the accumulation kernel: public here since the overlaps were added)

MAX_REFS = 8

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_ws = [_vp, _i64]    # (workspace_dev, workspace_bytes)
_NO_CPU = "the overlaps have no CPU fallback"


class OverlapAcc(ctypes.Structure):
    """wf_overlap_acc (include/waveflow_overlap.h)"""
    _fields_ = [("sums_dev", _vp), ("counts_dev", _vp)]


_acc = ctypes.POINTER(OverlapAcc)
# name -> (restype, argtypes): every function of include/waveflow_overlap.h, in its order (tests/test_overlap_host.py)
PROTOTYPES = {
    "wf_overlap_workspace_bytes": (_i64, [_i64, _i32]),
    "wf_overlap_accumulate": (_i32, [_vp, _vp, _i64, _i64, _i32, _acc, _vp] + _ws + [_vp]),
    "wf_overlap_penalise": (_i32, [_vp, _vp, _i64, _i64, _i32, _vp, _acc, _vp, _vp]),
    "wf_vqmc_overlap_step_workspace_bytes": (_i64, [_vp, _i64, _i32]),
    "wf_vqmc_overlap_step": (_i32, [_vp, _vp, _i32, _acc, _vp, ctypes.c_uint64, _i64, _i32, _vp, _i32, _vp] + _ws + [_vp]),
}


def lib():
    """The handle of _lib.lib() with PROTOTYPES applied to it."""
    return _lib.bound(PROTOTYPES)


# ---- checks: all of them before the first launch, none needs a GPU

def _check_K(K):
    K = int(K)
    if not 1 <= K <= MAX_REFS:
        raise ValueError(f"overlaps are built for 1 .. {MAX_REFS} reference states per call, got {K}")
    return K


def _check_penalty(penalty, K):
    """A float, or one per reference state: finite and >= 0 -> float32 [K]."""
    lam = np.asarray(penalty, dtype=np.float64).reshape(-1)
    if lam.size == 1:
        lam = np.repeat(lam, K)
    if lam.size != K:
        raise ValueError(f"overlap_penalty must be one number or one per lower state ({K}), got {lam.size}")
    if not np.all(np.isfinite(lam)) or np.any(lam < 0):
        raise ValueError(f"overlap_penalty must be finite and >= 0, got {lam.tolist()}")
    return np.ascontiguousarray(lam.astype(np.float32))


def _need_cuda(t, what, device=None):
    if not t.is_cuda or (device is not None and t.device != device):
        raise ValueError(f"{what} must be a cuda tensor on the device of psi: the overlaps have no CPU fallback")


def _check_rows(t, K, B, what, device=None, cuda=True):
    """A float32 cuda matrix [K, B] whose rows are contiguous (a row stride >= B is allowed) -> its row stride.  cuda=False: shape and type
    only (the caller asks _need_cuda once every shape has been looked at)."""
    import torch
    if not hasattr(t, "is_cuda") or t.dim() != 2 or tuple(t.shape) != (K, B):
        raise ValueError(f"{what} must be a torch tensor of shape [{K}, {B}]")
    if t.dtype != torch.float32 or (B > 1 and t.stride(1) != 1) or (K > 1 and t.stride(0) < B):
        raise ValueError(f"{what} must be float32 with contiguous rows, got {t.dtype} with strides {tuple(t.stride())}")
    if cuda:
        _need_cuda(t, what, device)
    return int(t.stride(0)) if K > 1 else max(B, 1)


def _check_vector(t, B, what, device=None, cuda=True):
    import torch
    if not hasattr(t, "is_cuda") or t.dim() != 1 or (B is not None and int(t.shape[0]) != B):
        raise ValueError(f"{what} must be a torch tensor of shape [{'B' if B is None else B}]")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous float32, got {t.dtype}")
    if cuda:
        _need_cuda(t, what, device)
    return int(t.shape[0])


def _check_step(batch, n_dim, K, walkers, out_walkers, ratios):
    """The arguments of one measurement step (core.DeviceModel.overlap_step): `walkers` (read) and `out_walkers` (written) are contiguous
    float32 cuda tensors [batch, n_dim] or None, at most one of them given; `ratios` is a contiguous float32 cuda tensor [K, batch] or None."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"{batch} walkers per step: at least 1")
    _accum.check_step_walkers(batch, n_dim, walkers, out_walkers, _NO_CPU, (("ratios", ratios, (K, batch)),))
    return batch


# ---- host side

class Totals:
    """What an Accumulator held, on the host: sums [K, 2] float64 (sum r_k, sum r_k^2) and counts [2] int64 (walkers counted, walkers
    skipped).  Plain numpy."""

    def __init__(self, K, sums=None, counts=None):
        self.K = _check_K(K)
        for name, given, shape, dtype in (("sums", sums, (self.K, 2), np.float64), ("counts", counts, (2,), np.int64)):
            a = np.zeros(shape, dtype) if given is None else np.array(given, dtype=dtype)
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            setattr(self, name, a)

    def merge(self, other):
        """self += other (another run, another rank): sums in fp64, counts in integers.  ValueError on another number of reference states."""
        if self.K != other.K:
            raise ValueError(f"cannot merge totals of {other.K} reference states into totals of {self.K}")
        self.sums = self.sums + other.sums
        self.counts = self.counts + other.counts
        return self

    def all_reduce(self, group=None):
        """SUM over the ranks of `group`, in place: one all-reduce for the fp64 part, one for the int64 part (distributed._all_reduce_sum), as
        observables.Totals.all_reduce.  Every rank must hold the same K."""
        f, self.counts = _accum.all_reduce_totals(self.sums, self.counts, group)
        self.sums = f.reshape(self.K, 2)
        return self

    def result(self):
        """-> dict: "overlap" [K] (S_k = sum r_k / n), "stderr" [K] (sqrt((<r_k^2> - S_k^2) / n): the walkers of an exact sampler are
        independent), "n" (walkers counted) and "n_skipped".  NaN where nothing was counted."""
        n = int(self.counts[0])
        if n > 0:
            s = self.sums[:, 0] / n
            err = np.sqrt(np.maximum(self.sums[:, 1] / n - s * s, 0.0) / n)
        else:
            s = err = np.full(self.K, np.nan)
        return {"overlap": s, "stderr": err, "n": n, "n_skipped": int(self.counts[1])}


# ---- device side

class Accumulator:
    """The device side of a measurement: two tensors (sums float64 [K, 2], counts int64 [2]) and the wf_overlap_acc that points at them
    (`.c`).  Library calls ADD to them; `reset()` zeroes them, `totals()` copies them to the host (it waits for the device)."""

    def __init__(self, K, device=None):
        import torch
        self.K = _check_K(K)
        self.device = _accum.cuda_device("cuda" if device is None else device, "an Accumulator", _NO_CPU)
        self.sums = torch.zeros(self.K, 2, dtype=torch.float64, device=self.device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.c = OverlapAcc(self.sums.data_ptr(), self.counts.data_ptr())
        self.st = {"x": self.sums, "ws": None}   # what DeviceModel._train_ws asks of a step's state: a device, a workspace that is kept

    def reset(self):
        self.sums.zero_()
        self.counts.zero_()
        return self

    def totals(self):
        return Totals(self.K, self.sums.cpu().numpy(), self.counts.cpu().numpy())


def accumulate(psi, refs, acc=None, ratios=None, workspace=None):
    """wf_overlap_accumulate on psi [B] and refs [K, B] (float32 cuda; the rows of refs contiguous, a row stride above B allowed): adds the
    batch to `acc` (an Accumulator of K states, or None) and writes r_k to `ratios` (float32 cuda [K, B] with the row stride of refs, or
    None).  With neither, ratios are allocated.  -> ratios (None when only `acc` was given)."""
    import torch
    from .core import DeviceModel
    B = _check_vector(psi, None, "psi", cuda=False)
    if not hasattr(refs, "dim") or refs.dim() != 2:
        raise ValueError("refs must be a 2-d torch tensor [K, B]")
    K = _check_K(refs.shape[0])
    ld = _check_rows(refs, K, B, "refs", cuda=False)
    _need_cuda(psi, "psi")
    _need_cuda(refs, "refs", psi.device)
    if acc is None and ratios is None:
        ratios = torch.empty_strided((K, B), (ld, 1), dtype=torch.float32, device=psi.device)
    if ratios is not None and _check_rows(ratios, K, B, "ratios", psi.device) != ld:
        raise ValueError(f"ratios must have the row stride of refs ({ld})")
    if acc is not None and (not isinstance(acc, Accumulator) or acc.K != K or acc.device != psi.device):
        raise ValueError(f"the accumulator must hold {K} reference states on {psi.device}")
    if B == 0:
        return ratios
    L = lib()
    if acc is not None and workspace is None:
        workspace = DeviceModel._workspace(_lib.check(L.wf_overlap_workspace_bytes(B, K), "wf_overlap_workspace_bytes"), psi.device)
    with torch.cuda.device(psi.device):
        _lib.check(L.wf_overlap_accumulate(psi.data_ptr(), refs.data_ptr(), ld, B, K, ctypes.byref(acc.c) if acc is not None else None,
                                           _lib.ptr(ratios), _lib.ptr(workspace), workspace.numel() if workspace is not None else 0,
                                           _lib.stream_ptr(psi.device)), "wf_overlap_accumulate")
    return ratios


def penalise(e_loc, ratios, acc, penalty, out=None):
    """wf_overlap_penalise: e~_b = e_b + sum_k lambda_k a_k (r_kb - a_k) with a_k the mean of r_k in `acc`, which must hold exactly the batch
    of `ratios` [K, B] (as `accumulate` wrote them).  penalty: one number or one per state, >= 0.  -> float32 cuda [B] (`out`, which may be
    e_loc itself; a new tensor by default).  No host read."""
    import torch
    B = _check_vector(e_loc, None, "e_loc", cuda=False)
    if not hasattr(ratios, "dim") or ratios.dim() != 2:
        raise ValueError("ratios must be a 2-d torch tensor [K, B]")
    K = _check_K(ratios.shape[0])
    ld = _check_rows(ratios, K, B, "ratios", cuda=False)
    lam = _check_penalty(penalty, K)
    _need_cuda(e_loc, "e_loc")
    _need_cuda(ratios, "ratios", e_loc.device)
    if not isinstance(acc, Accumulator) or acc.K != K or acc.device != e_loc.device:
        raise ValueError(f"the accumulator must hold {K} reference states on {e_loc.device}")
    if out is None:
        out = torch.empty_like(e_loc)
    else:
        _check_vector(out, B, "out", e_loc.device)
    if B == 0:
        return out
    with torch.cuda.device(e_loc.device):
        _lib.check(lib().wf_overlap_penalise(e_loc.data_ptr(), ratios.data_ptr(), ld, B, K, lam.ctypes.data, ctypes.byref(acc.c), out.data_ptr(),
                                             _lib.stream_ptr(e_loc.device)), "wf_overlap_penalise")
    return out


# ---- the two kernels restated on the host

def reference_accumulate(psi, refs, sums=None, counts=None):
    """The accumulation kernel in numpy on float32 psi [B] and refs [K, B] -> (ratios [K, B] float32, sums [K, 2] float64, counts [2]
    int64): fp32 per operation, the fp64 sums of the batch in the order of the device, added to `sums` / `counts` (zeros by default)."""
    f32, f64 = np.float32, np.float64
    psi = np.ascontiguousarray(psi, dtype=f32).reshape(-1)
    refs = np.asarray(refs, dtype=f32)
    if refs.ndim != 2 or refs.shape[1] != psi.shape[0]:
        raise ValueError(f"refs must have shape [K, {psi.shape[0]}], got {refs.shape}")
    K = _check_K(refs.shape[0])
    sums = np.zeros((K, 2), f64) if sums is None else np.array(sums, dtype=f64)
    counts = np.zeros(2, np.int64) if counts is None else np.array(counts, dtype=np.int64)
    if sums.shape != (K, 2) or counts.shape != (2,):
        raise ValueError(f"sums must have shape ({K}, 2) and counts (2,)")
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / (psi + f32(1e-8)).astype(f32)).astype(f32)
        ratios = (refs * inv[None, :]).astype(f32)
    ok = np.isfinite(psi) & np.isfinite(refs).all(0) & np.isfinite(ratios).all(0)
    if psi.shape[0] > 0:
        for k in range(K):
            r = np.where(ok, ratios[k], f32(0.0)).astype(f64)
            sums[k, 0] += _accum.ordered_sum(r)
            sums[k, 1] += _accum.ordered_sum(r * r)
    counts += np.array([ok.sum(), (~ok).sum()], dtype=np.int64)
    return ratios, sums, counts


def reference_penalise(e_loc, ratios, sums, counts, penalty):
    """The penalty kernel in numpy -> float32 [B]: a_k = sums[k][0] / counts[0]; per walker, in fp64 with k ascending,
    s = e; s = s + (lambda_k a_k) (r_k - a_k); rounded to fp32 once.  A walker with a ratio that is not finite, and every walker when
    counts[0] == 0, keeps its e."""
    f32, f64 = np.float32, np.float64
    e = np.ascontiguousarray(e_loc, dtype=f32).reshape(-1)
    ratios = np.asarray(ratios, dtype=f32)
    if ratios.ndim != 2 or ratios.shape[1] != e.shape[0]:
        raise ValueError(f"ratios must have shape [K, {e.shape[0]}], got {ratios.shape}")
    K = _check_K(ratios.shape[0])
    lam = _check_penalty(penalty, K).astype(f64)
    sums, counts = np.asarray(sums, dtype=f64), np.asarray(counts, dtype=np.int64)
    if sums.shape != (K, 2) or counts.shape != (2,):
        raise ValueError(f"sums must have shape ({K}, 2) and counts (2,)")
    n = int(counts[0])
    if n == 0:
        return e.copy()
    s = e.astype(f64)
    with np.errstate(all="ignore"):
        for k in range(K):
            a = sums[k, 0] / f64(n)
            s = s + (lam[k] * a) * (ratios[k].astype(f64) - a)
        out = s.astype(f32)
    return np.where(np.isfinite(ratios).all(0), out, e)


# ---- measurements

def measure(model, ref_models, n_walkers, batch, seed, exact_sampler=True, use_graph=True, acc=None):
    """ceil(n_walkers / batch) overlap steps of `batch` walkers each (DeviceModel.overlap_step: walkers of `model` from the sampler stream
    `seed`, advanced by a device counter that starts at 0; psi of `model` and of every model of `ref_models` on them), added to `acc`
    (default: a new Accumulator) -> its Totals.  With use_graph the step is captured once (vqmc.capture_step; its warm-up call outside the
    capture is undone) and replayed; the host waits once, at the end.  exact_sampler=False draws from the reference's sampler, whose law is
    not |psi|^2: the estimator is then biased."""
    import torch
    n_walkers, batch = int(n_walkers), int(batch)
    if n_walkers < 1 or batch < 1:
        raise ValueError("n_walkers and batch must be >= 1")
    ref_models = list(ref_models)
    K = _check_K(len(ref_models))
    if acc is None:
        acc = Accumulator(K, f"cuda:{model.device}")
    counter = torch.zeros(1, dtype=torch.int64, device=acc.device)

    def step():
        model.overlap_step(ref_models, acc, counter, seed, batch, exact_sampler=exact_sampler)
    _accum.measure_loop(model, acc, step, -(-n_walkers // batch), model.overlap_step_workspace_bytes(batch, K), (acc.sums, acc.counts, counter),
                        "overlap", use_graph)
    return acc.totals()


def overlap_matrix(models, n_walkers, batch, seed, exact_sampler=True, use_graph=True):
    """The table of overlaps between K models (2 <= K <= 8), each holding its parameters: row i is one `measure` on the walkers of models[i]
    against every model (itself included: the diagonal, 1 up to the 1e-8 regulariser).  -> dict: "raw" [K, K] (raw[i, j] = <psi_j|psi_i>
    estimated on the walkers of i) and "raw_stderr" -- both one-sided estimates of every off-diagonal entry are reported --, "overlap" (the
    symmetric table, (raw + raw^T) / 2), "stderr" (sqrt(err_ij^2 + err_ji^2) / 2), "n" [K] and "n_skipped" [K]."""
    models = list(models)
    K = len(models)
    if not 2 <= K <= MAX_REFS:
        raise ValueError(f"an overlap matrix is built for 2 .. {MAX_REFS} models, got {K}")
    raw, err = np.zeros((K, K)), np.zeros((K, K))
    n, skipped = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for i, m in enumerate(models):
        r = measure(m, models, n_walkers, batch, int(seed) + i, exact_sampler=exact_sampler, use_graph=use_graph).result()
        raw[i], err[i], n[i], skipped[i] = r["overlap"], r["stderr"], r["n"], r["n_skipped"]
    return {"raw": raw, "raw_stderr": err, "overlap": 0.5 * (raw + raw.T), "stderr": 0.5 * np.sqrt(err ** 2 + err.T ** 2), "n": n, "n_skipped": skipped}
