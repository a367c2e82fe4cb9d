"""Stochastic reconfiguration (the natural gradient of variational Monte Carlo) from per-walker Jacobian rows, in its B x B ("minSR") form:
the ctypes surface of include/waveflow_sr.h, and of include/waveflow_sr_step.h (the whole training step on the device: STEP_PROTOTYPES,
SrTrainState; core.DeviceModel.sr_step drives it), and of include/waveflow_sr_spring.h (the SPRING optimiser: SPRING_PROTOTYPES, SpringTrainState,
`matvec`, `apply_add`, `spring_rhs`, `clip_local_energies`, `spring_direction`; core.DeviceModel.spring_step drives the whole step), and of
include/waveflow_sr_cg.h (the same solve without the B x B matrix, for more than MAX_WALKERS walkers: CG_PROTOTYPES, `solve_cg`, `cg_reference`,
and `solver='cg'` of `natural_gradient` and `spring_direction`).

With O[b][k] = d ln psi_b / d theta_k, local energies e, H = I - 1 1^T / B and lambda > 0,
    d = (O^T H O / B + lambda I)^-1 (2 / B) O^T H e  =  (2 / B) O^T H y,    (H O O^T H / B + lambda I) y = H e
-- `gram`, `solve`, `apply`, and `natural_gradient` for the three in a row.  The rows are read twice and never rewritten; lambda is
`damping + relative_damping * trace(Tbar) / B`.  Everything runs on the GPU that holds the rows, on torch's current stream; there is no
CPU fallback, and arguments are checked before anything is launched (ValueError).
"""
import ctypes

from . import _accum, _lib

MAX_WALKERS = 4096   # wf_sr_solve: Tbar is 128 MiB there

_vp, _i32, _i64, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
_ws = [_vp, _i64]    # (workspace_dev, workspace_bytes)
# name -> (restype, argtypes): every function of include/waveflow_sr.h, in its order (tests/test_sr_host.py holds the two against each other)
PROTOTYPES = {
    "wf_sr_workspace_bytes": (_i64, [_i64, _i64]),
    "wf_sr_gram": (_i32, [_vp, _i64, _i64, _i64, _vp] + _ws + [_vp]),
    "wf_sr_solve": (_i32, [_vp, _i64, _vp, _f64, _f64, _vp, _vp] + _ws + [_vp]),
    "wf_sr_apply": (_i32, [_vp, _i64, _i64, _i64, _vp, _f64, _vp] + _ws + [_vp]),
}


class SrTrainState(ctypes.Structure):
    """wf_sr_train_state (include/waveflow_sr_step.h)"""
    _fields_ = [("params_dev", _vp), ("counter_dev", _vp), ("step_size_dev", _vp), ("loss_ring_dev", _vp), ("norm_ring_dev", _vp),
                ("status_dev", _vp), ("ring_len", ctypes.c_int32), ("defer_eval_tables", ctypes.c_int32)]


# name -> (restype, argtypes): every function of include/waveflow_sr_step.h, in its order (tests/test_sr_step_host.py)
STEP_PROTOTYPES = {
    "wf_vqmc_sr_step_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_vqmc_sr_step": (_i32, [_vp, ctypes.POINTER(SrTrainState), ctypes.c_uint64, _i64, _vp, _i32, _f64, _f64, _i32, _vp, _i32] + _ws + [_vp]),
}


class SpringTrainState(ctypes.Structure):
    """wf_spring_train_state (include/waveflow_sr_spring.h): the fields of SrTrainState, then the previous direction and the ring of step sizes"""
    _fields_ = SrTrainState._fields_ + [("phi_dev", _vp), ("eff_ring_dev", _vp)]


# name -> (restype, argtypes): every function of include/waveflow_sr_spring.h, in its order (tests/test_sr_spring_host.py)
SPRING_PROTOTYPES = {
    "wf_sr_matvec": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "wf_sr_apply_add": (_i32, [_vp, _i64, _i64, _i64, _vp, _f64, _vp, _f64, _vp] + _ws + [_vp]),
    "wf_spring_rhs": (_i32, [_vp, _vp, _i64, _vp, _f64, _f64, _vp, _vp, _vp, _vp, _vp]),
    "wf_vqmc_spring_step_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_vqmc_spring_step": (_i32, [_vp, ctypes.POINTER(SpringTrainState), ctypes.c_uint64, _i64, _vp, _i32, _f64, _f64, _f64, _f64, _f64, _i32, _vp, _i32]
                            + _ws + [_vp]),
}

# name -> (restype, argtypes): every function of include/waveflow_sr_cg.h, in its order (tests/test_sr_cg_host.py)
CG_PROTOTYPES = {
    "wf_sr_cg_workspace_bytes": (_i64, [_i64, _i64]),
    "wf_sr_cg_solve": (_i32, [_vp, _i64, _i64, _i64, _vp, _f64, _f64, _f64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp] + _ws + [_vp]),
}
MAX_ROWS = 65536     # the row passes (wf_sr_matvec, wf_sr_apply, wf_sr_cg_solve)
SOLVERS = ('cholesky', 'cg')


class NotPositiveDefinite(ArithmeticError):
    """The Cholesky factorisation of Tbar + lambda I met a pivot that is not positive; `pivot` is its 1-based index."""

    def __init__(self, pivot):
        self.pivot = int(pivot)
        super().__init__(f"stochastic reconfiguration: pivot {self.pivot} of the shifted B x B matrix is not positive (more damping, or non-finite rows)")


class NotConverged(ArithmeticError):
    """solve_cg used its `max_iter` iterations; `iterations` and `residual` (the recurrence's |r| / |rhs|) say where it stood."""

    def __init__(self, iterations, residual, tol):
        self.iterations, self.residual = int(iterations), float(residual)
        super().__init__(f"stochastic reconfiguration: conjugate gradients stood at |r| / |rhs| = {self.residual:.3e} after {self.iterations} "
                         f"iterations (tol {tol:.1e}): more iterations or more damping")


class NotFinite(ArithmeticError):
    """solve_cg met a value that is not finite (rows, right-hand side), a shift that is not positive, or p^T A p <= 0; y is NaN."""

    def __init__(self, iterations):
        self.iterations = int(iterations)
        super().__init__(f"stochastic reconfiguration: conjugate gradients broke down in iteration {self.iterations + 1} (rows or right-hand side "
                         "that are not finite, or a shift that is not positive)")


def lib():
    """The handle of _lib.lib() with PROTOTYPES, STEP_PROTOTYPES, SPRING_PROTOTYPES and CG_PROTOTYPES applied to it."""
    return _lib.bound(PROTOTYPES, STEP_PROTOTYPES, SPRING_PROTOTYPES, CG_PROTOTYPES)


# ---- checks: all of them before the first launch, none needs a GPU

def _check_damping(damping, relative_damping):
    damping, relative_damping = float(damping), float(relative_damping)
    if not damping >= 0.0 or not relative_damping >= 0.0:
        raise ValueError(f"damping and relative_damping must be >= 0, got {damping} and {relative_damping}")
    if damping == 0.0 and relative_damping == 0.0:
        raise ValueError("damping and relative_damping are both zero: the centred B x B matrix is singular without a shift")
    return damping, relative_damping


def _check_step(batch, n_dim, damping, relative_damping, walkers, out_walkers):
    """The arguments of one device-side training step (core.DeviceModel.sr_step) -> (damping, relative_damping); `walkers` (read) and
    `out_walkers` (written) are contiguous float32 cuda tensors [batch, n_dim] or None, and at most one of them is given."""
    damping, relative_damping = _check_damping(damping, relative_damping)
    batch = int(batch)
    if batch < 1 or batch > MAX_WALKERS:
        raise ValueError(f"{batch} walkers per step: the B x B solve is built for 1 .. {MAX_WALKERS}")
    _accum.check_step_walkers(batch, n_dim, walkers, out_walkers, "stochastic reconfiguration has no CPU fallback")
    return damping, relative_damping


def _check_spring(momentum, norm_constraint, clip):
    """-> (momentum in [0, 1), norm cap >= 0, clip factor >= 0) as floats"""
    momentum, norm_constraint, clip = float(momentum), float(norm_constraint), float(clip)
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"momentum must lie in [0, 1), got {momentum}")
    if not norm_constraint >= 0.0:
        raise ValueError(f"the norm constraint must be >= 0 (0: none), got {norm_constraint}")
    if not clip >= 0.0:
        raise ValueError(f"the clip factor must be >= 0 (0: no clipping), got {clip}")
    return momentum, norm_constraint, clip


def _check_solver(solver, tol=1e-8, max_iter=2000, round_iters=32):
    """-> (solver, tol, max_iter, round_iters)"""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    tol = float(tol)
    if not 0.0 < tol < 1.0:
        raise ValueError(f"tol must lie in (0, 1), got {tol}")
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter must be a whole number >= 1, got {max_iter}")
    if int(round_iters) != round_iters or int(round_iters) < 1:
        raise ValueError(f"round_iters must be a whole number >= 1, got {round_iters}")
    return solver, tol, int(max_iter), int(round_iters)


def _check_rows(rows, limit=None):
    """-> (B, P, ld).  float32 cuda [B, P] whose rows are contiguous (a column slice of a wider contiguous matrix is fine: ld is its row stride)."""
    import torch
    if not hasattr(rows, "is_cuda") or rows.dim() != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("rows must be a non-empty 2-d torch tensor [B, P]")
    if rows.dtype != torch.float32:
        raise ValueError(f"rows must be float32, got {rows.dtype}")
    B, P = int(rows.shape[0]), int(rows.shape[1])
    ld = int(rows.stride(0)) if B > 1 else max(int(rows.stride(0)), P)
    if (P > 1 and rows.stride(1) != 1) or ld < P:
        raise ValueError("rows must be contiguous along the parameter axis (stride 1, row stride >= P)")
    if limit is not None and B > limit:
        raise ValueError(f"{B} walkers: the B x B solve is built for at most {limit}")
    if not rows.is_cuda:
        raise ValueError("rows must be a cuda tensor: stochastic reconfiguration has no CPU fallback")
    return B, P, ld


def _check_vector(v, n, dtype, what, device):
    import torch
    if not hasattr(v, "is_cuda") or v.dim() != 1 or v.numel() != n:
        raise ValueError(f"{what} must be a vector of {n} entries")
    if not v.is_cuda or v.device != device:
        raise ValueError(f"{what} must be a cuda tensor on the device of the other operands (no CPU fallback)")
    if dtype is not None and v.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {v.dtype}")
    if dtype is None and not torch.is_floating_point(v):
        raise ValueError(f"{what} must be floating point")


def _check_matrix(T):
    import torch
    if not hasattr(T, "is_cuda") or T.dim() != 2 or T.shape[0] != T.shape[1] or T.shape[0] < 1:
        raise ValueError("T must be a square 2-d torch tensor")
    if T.dtype != torch.float64 or not T.is_contiguous():
        raise ValueError("T must be contiguous float64")
    if not T.is_cuda:
        raise ValueError("T must be a cuda tensor: stochastic reconfiguration has no CPU fallback")
    if T.shape[0] > MAX_WALKERS:
        raise ValueError(f"{T.shape[0]} walkers: the B x B solve is built for at most {MAX_WALKERS}")
    return int(T.shape[0])


# ---- launches

def _workspace(B, P, device):
    from .core import DeviceModel
    nbytes = _lib.check(lib().wf_sr_workspace_bytes(B, P), "wf_sr_workspace_bytes")
    return DeviceModel._workspace(nbytes, device)   # (poisoned under WF_POISON like every workspace)


def _gram(rows, B, P, ld, ws):
    import torch
    T = torch.empty((B, B), dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib().wf_sr_gram(rows.data_ptr(), B, P, ld, T.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(rows.device)), "wf_sr_gram")
    return T


def _solve(T, B, rhs, damping, relative_damping, ws):
    import torch
    y = torch.empty(B, dtype=torch.float64, device=T.device)
    info = torch.empty(1, dtype=torch.int32, device=T.device)
    with torch.cuda.device(T.device):
        _lib.check(lib().wf_sr_solve(T.data_ptr(), B, rhs.data_ptr(), damping, relative_damping, y.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _lib.stream_ptr(T.device)), "wf_sr_solve")
    return y, info


def _apply(rows, B, P, ld, y, scale, ws):
    import torch
    out = torch.empty(P, dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib().wf_sr_apply(rows.data_ptr(), B, P, ld, y.data_ptr(), float(scale), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr(rows.device)), "wf_sr_apply")
    return out


# ---- surface

def gram(rows, workspace=None):
    """Tbar = H (rows rows^T) H / B -> float64 cuda [B, B], exactly symmetric (wf_sr_gram)."""
    B, P, ld = _check_rows(rows)
    return _gram(rows, B, P, ld, workspace if workspace is not None else _workspace(B, P, rows.device))


def solve(T, rhs, damping=0.0, relative_damping=1e-3, workspace=None):
    """(T + lambda I) y = rhs with lambda = damping + relative_damping * trace(T) / B -> (y float64 [B], info int32 cuda [1]).  T (float64 cuda
    [B, B]) is overwritten: its lower triangle holds the Cholesky factor afterwards.  info is 0, or the 1-based index of the first pivot that
    is not positive (y is NaN then); nothing here waits for the device, reading `info` does (wf_sr_solve)."""
    damping, relative_damping = _check_damping(damping, relative_damping)
    B = _check_matrix(T)
    import torch
    _check_vector(rhs, B, torch.float64, "rhs", T.device)
    return _solve(T, B, rhs.contiguous(), damping, relative_damping, workspace if workspace is not None else _workspace(B, 1, T.device))


def apply(rows, y, scale, workspace=None):
    """out[p] = scale * sum_b (y_b - mean y) rows[b][p] -> float32 cuda [P] (wf_sr_apply)."""
    import torch
    B, P, ld = _check_rows(rows)
    _check_vector(y, B, torch.float64, "y", rows.device)
    return _apply(rows, B, P, ld, y.contiguous(), scale, workspace if workspace is not None else _workspace(B, P, rows.device))


def natural_gradient(rows, e_loc, damping=0.0, relative_damping=1e-3, solver='cholesky', tol=1e-8, max_iter=2000):
    """d = (S + lambda I)^-1 g for rows O = d ln psi / d theta [B, P] and local energies e_loc [B]: S = O^T H O / B, g = (2 / B) O^T H e,
    lambda = damping + relative_damping * trace(Tbar) / B -> float32 cuda [P].  Three library calls on the current stream, then one read of the
    solver's status: NotPositiveDefinite if a pivot was not positive.  solver='cg': Tbar is never formed and B may exceed MAX_WALKERS -- solve_cg
    to `tol` within `max_iter` iterations (NotConverged, NotFinite), then the same apply."""
    damping, relative_damping = _check_damping(damping, relative_damping)
    solver, tol, max_iter, _ = _check_solver(solver, tol, max_iter)
    B, P, ld = _check_rows(rows, limit=MAX_WALKERS if solver == 'cholesky' else MAX_ROWS)
    _check_vector(e_loc, B, None, "e_loc", rows.device)
    return _direction(rows, B, P, ld, e_loc.double(), None, 0.0, damping, relative_damping, solver, tol, max_iter)


# ---- SPRING (include/waveflow_sr_spring.h)

def _matvec(rows, B, P, ld, v):
    import torch
    q = torch.empty(B, dtype=torch.float64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib().wf_sr_matvec(rows.data_ptr(), B, P, ld, v.data_ptr(), q.data_ptr(), _lib.stream_ptr(rows.device)), "wf_sr_matvec")
    return q


def _apply_add(rows, B, P, ld, y, scale, prev, mu, out, ws):
    import torch
    with torch.cuda.device(rows.device):
        _lib.check(lib().wf_sr_apply_add(rows.data_ptr(), B, P, ld, y.data_ptr(), float(scale), None if prev is None else prev.data_ptr(), float(mu),
                                         out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(rows.device)), "wf_sr_apply_add")
    return out


def matvec(rows, v):
    """q[b] = sum_p rows[b][p] v[p] -> float64 cuda [B]: fp32 operands, exact products, fp64 sums in a fixed order (wf_sr_matvec)."""
    import torch
    B, P, ld = _check_rows(rows)
    _check_vector(v, P, torch.float32, "v", rows.device)
    return _matvec(rows, B, P, ld, v.contiguous())


def apply_add(rows, y, scale, prev=None, mu=0.0, out=None, workspace=None):
    """out[p] = fl32(mu * prev[p] + scale * sum_b (y_b - mean y) rows[b][p]) -> float32 cuda [P]; prev None or mu 0: the bits of `apply`.
    `out` (float32 cuda [P], contiguous) may be `prev` itself (wf_sr_apply_add)."""
    import torch
    B, P, ld = _check_rows(rows)
    _check_vector(y, B, torch.float64, "y", rows.device)
    mu = _check_spring(mu, 0.0, 0.0)[0]
    for what, t in (("prev", prev), ("out", out)):
        if t is not None:
            _check_vector(t, P, torch.float32, what, rows.device)
            if not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=rows.device)
    return _apply_add(rows, B, P, ld, y.contiguous(), scale, prev, mu, out, workspace if workspace is not None else _workspace(B, P, rows.device))


def spring_rhs(hpsi, psi, q=None, momentum=0.0, clip=0.0):
    """The right-hand side of the SPRING solve as the device step computes it (wf_spring_rhs): hpsi, psi float32 cuda [B], q float64 cuda [B]
    (needed when momentum > 0) -> (e_loc, inv float32 [B], rhs float64 [B], stats float64 [4] = median, mean absolute deviation, clamp bounds)."""
    import torch
    momentum, _, clip = _check_spring(momentum, 0.0, clip)
    if not hasattr(hpsi, "is_cuda") or hpsi.dim() != 1 or hpsi.numel() < 1 or hpsi.numel() > MAX_WALKERS:
        raise ValueError(f"hpsi must be a vector of 1 .. {MAX_WALKERS} entries")
    if not hpsi.is_cuda:
        raise ValueError("hpsi must be a cuda tensor: stochastic reconfiguration has no CPU fallback")
    B, dev = hpsi.numel(), hpsi.device
    _check_vector(hpsi, B, torch.float32, "hpsi", dev)
    _check_vector(psi, B, torch.float32, "psi", dev)
    if momentum != 0.0 and q is None:
        raise ValueError("momentum > 0 needs q = rows @ prev (matvec)")
    if q is not None:
        _check_vector(q, B, torch.float64, "q", dev)
        q = q.contiguous()
    hpsi, psi = hpsi.contiguous(), psi.contiguous()
    e_loc, inv = torch.empty_like(hpsi), torch.empty_like(hpsi)
    rhs, stats = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib().wf_spring_rhs(hpsi.data_ptr(), psi.data_ptr(), B, None if q is None else q.data_ptr(), momentum, clip, e_loc.data_ptr(),
                                       inv.data_ptr(), rhs.data_ptr(), stats.data_ptr(), _lib.stream_ptr(dev)), "wf_spring_rhs")
    return e_loc, inv, rhs, stats


def _median_and_deviation(e32):
    """(c, w) of float32 e_b as float64 scalars: c the median (even B: the mean of the two middle values; values that are not finite count as
    +inf and so sort last), w = mean |e_b - c|."""
    import torch
    B = e32.numel()
    key = torch.where(torch.isfinite(e32), e32, torch.full_like(e32, float("inf"))).sort().values.double()
    c = key[B // 2] if B % 2 else 0.5 * (key[B // 2 - 1] + key[B // 2])
    return c, (e32.double() - c).abs().mean()


def clip_local_energies(e_loc, clip):
    """clamp(e_b, c - k w, c + k w) in float64, c the median of the float32 e_b (even B: the mean of the two middle values; values that are not
    finite sort last), w = mean |e_b - c|; clip == 0: e_loc as float64, unchanged.  The eager counterpart of the device step's clamp."""
    import torch
    e32 = e_loc.float()
    e = e32.double()
    if float(clip) == 0.0:
        return e
    c, w = _median_and_deviation(e32)
    return torch.minimum(torch.maximum(e, c - float(clip) * w), c + float(clip) * w)


def spring_direction(rows, e_loc, prev, momentum, damping=0.0, relative_damping=1e-3, clip=0.0, solver='cholesky', tol=1e-8, max_iter=2000):
    """The SPRING direction d = mu prev + (2 / B) O^T H y with (Tbar + lambda I) y = H (e~ - (mu / 2) O prev), the minimiser of
    (1 / B) |H O d - 2 H e~|^2 + lambda |d - mu prev|^2; e~ = clip_local_energies(e_loc, clip); momentum 0 gives natural_gradient.
    rows [B, P] float32 cuda, e_loc [B], prev float32 cuda [P] (the previous d; zeros at the start) -> float32 cuda [P].  Library calls on the
    current stream, then one read of the solver's status: NotPositiveDefinite if a pivot was not positive.  solver='cg': as in natural_gradient."""
    import torch
    damping, relative_damping = _check_damping(damping, relative_damping)
    momentum, _, clip = _check_spring(momentum, 0.0, clip)
    solver, tol, max_iter, _ = _check_solver(solver, tol, max_iter)
    B, P, ld = _check_rows(rows, limit=MAX_WALKERS if solver == 'cholesky' else MAX_ROWS)
    _check_vector(e_loc, B, None, "e_loc", rows.device)
    _check_vector(prev, P, torch.float32, "prev", rows.device)
    return _direction(rows, B, P, ld, clip_local_energies(e_loc, clip), prev.contiguous(), momentum, damping, relative_damping, solver, tol, max_iter)


def _direction(rows, B, P, ld, e, prev, mu, damping, relative_damping, solver, tol, max_iter):
    """d = mu prev + (2 / B) O^T H y with (Tbar + lambda I) y = H (e - (mu / 2) O prev) for checked operands: e float64 [B], not centred; prev None
    (then mu is 0): the plain natural gradient.  The dense workspace, Gram matrix and Cholesky solve with its pivot check, or solver='cg'."""
    import torch
    ws = _workspace(B, P, rows.device) if solver == 'cholesky' else _cg_workspace(B, P, rows.device)
    r = e if mu == 0.0 else e - (0.5 * mu) * _matvec(rows, B, P, ld, prev)
    info = None
    if solver == 'cg':
        y, _ = _solve_cg(rows, B, P, ld, r - r.mean(), damping, relative_damping, tol, max_iter, 32, False, ws)
    else:
        y, info = _solve(_gram(rows, B, P, ld, ws), B, r - r.mean(), damping, relative_damping, ws)
    if prev is None:
        d = _apply(rows, B, P, ld, y, 2.0 / B, ws)
    else:
        d = _apply_add(rows, B, P, ld, y, 2.0 / B, prev, mu, torch.empty(P, dtype=torch.float32, device=rows.device), ws)
    if info is not None and int(info.item()) != 0:
        raise NotPositiveDefinite(int(info.item()))
    return d


# ---- the matrix-free solve (include/waveflow_sr_cg.h)

def _cg_workspace(B, P, device):
    from .core import DeviceModel
    nbytes = _lib.check(lib().wf_sr_cg_workspace_bytes(B, P), "wf_sr_cg_workspace_bytes")
    return DeviceModel._workspace(nbytes, device)   # (at least wf_sr_apply's: the apply behind the solve uses it too)


def _cg_call(rows, B, P, ld, rhs, damping, relative_damping, tol, n_iter, restart, precondition, y, info, ws):
    """One wf_sr_cg_solve on the current stream: nothing waits, nothing is allocated (capturable)."""
    import torch
    with torch.cuda.device(rows.device):
        _lib.check(lib().wf_sr_cg_solve(rows.data_ptr(), B, P, ld, rhs.data_ptr(), damping, relative_damping, tol, int(n_iter), int(bool(restart)),
                                        int(bool(precondition)), y.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr(rows.device)), "wf_sr_cg_solve")


def _solve_cg(rows, B, P, ld, rhs, damping, relative_damping, tol, max_iter, round_iters, precondition, ws):
    import torch
    y = torch.empty(B, dtype=torch.float64, device=rows.device)
    info = torch.empty(4, dtype=torch.float64, device=rows.device)
    rhs = rhs.contiguous()
    done, restart = 0, True
    while True:
        n = min(round_iters, max_iter - done)
        _cg_call(rows, B, P, ld, rhs, damping, relative_damping, tol, n, restart, precondition, y, info, ws)
        done, restart = done + n, False
        status, iterations, residual, _ = info.cpu().tolist()   # (the round's one wait)
        if status == 0.0:
            return y, info
        if status != 1.0:
            raise NotFinite(iterations)
        if done >= max_iter:
            raise NotConverged(iterations, residual, tol)


def solve_cg(rows, rhs, damping=0.0, relative_damping=1e-3, tol=1e-8, max_iter=2000, round_iters=32, precondition=False, workspace=None):
    """(Tbar + lambda I) y = rhs without Tbar: conjugate gradients, each iteration one O^T (H p) pass and one O z pass over the rows (wf_sr_cg_solve)
    -> (y float64 cuda [B], info float64 cuda [4] = status 0, iterations, the recurrence's |r| / |rhs|, lambda).  rows float32 cuda [B, P] with
    B up to MAX_ROWS, rhs float64 cuda [B], already centred; lambda = damping + relative_damping * trace(Tbar) / B as in `solve`;
    precondition: Jacobi, with the diagonal of Tbar + lambda I -- off by default, and off in natural_gradient / spring_direction: on He's rows
    it costs 9 to 30 times the iterations (Tbar + lambda I is a few large eigenvalues over a cluster at lambda, which plain
    conjugate gradients resolve in tens of steps and which scaling by rows of very different norms takes apart).  Rounds of `round_iters` iterations are enqueued and `info` is read between
    them (one wait per round); NotFinite on status 2, NotConverged when `max_iter` iterations did not reach |r| <= tol |rhs|."""
    import torch
    damping, relative_damping = _check_damping(damping, relative_damping)
    _, tol, max_iter, round_iters = _check_solver('cg', tol, max_iter, round_iters)
    B, P, ld = _check_rows(rows, limit=MAX_ROWS)
    _check_vector(rhs, B, torch.float64, "rhs", rows.device)
    return _solve_cg(rows, B, P, ld, rhs, damping, relative_damping, tol, max_iter, round_iters, precondition,
                     workspace if workspace is not None else _cg_workspace(B, P, rows.device))


def cg_reference(rows, rhs, damping=0.0, relative_damping=1e-3, tol=1e-8, max_iter=2000, precondition=False, history=False):
    """The recurrences of wf_sr_cg_solve in NumPy float64 (sums in NumPy's order, not the device's): rows [B, P] and rhs [B] array-likes
    -> (y float64 [B], info float64 [4] = status, iterations, the recurrence's |r| / |rhs|, lambda); status 1 when `max_iter` iterations did
    not converge.  history=True adds a third result, the list of (recursive, true) relative residuals after every iteration."""
    import numpy as np
    O = np.asarray(rows, dtype=np.float64)
    rhs = np.asarray(rhs, dtype=np.float64)
    B = O.shape[0]
    nan = float("nan")
    obar = O.sum(0) / B
    diag = ((O - obar) ** 2).sum(1) / B                         # the diagonal of Tbar = H O O^T H / B
    lam = float(damping) + float(relative_damping) * diag.sum() / B
    rhs2 = float(rhs @ rhs)
    steps = []
    out = (lambda y, status, it, r2: (y, np.array([status, it, np.sqrt(r2 / rhs2) if rhs2 > 0 else (nan if status == 2 else 0.0), lam]))
           + ((steps,) if history else ()))
    if not (np.isfinite(diag.sum()) and np.isfinite(rhs2) and np.isfinite(lam) and lam > 0.0):
        return out(np.full(B, nan), 2, 0, nan)
    if rhs2 == 0.0 or B == 1:
        return out(rhs / lam, 0, 0, 0.0)
    M = diag + lam if precondition else np.ones(B)

    def tbar(v):
        z = O.T @ (v - v.mean())                                # pass A
        q = O @ z                                               # pass B
        return (q - q.mean()) / B, float(z @ z)
    y, r = np.zeros(B), rhs.copy()
    p = r / M
    rho = float(r @ p)
    r2 = rhs2
    for it in range(1, int(max_iter) + 1):
        tp, zz = tbar(p)
        pAp = zz / B + lam * float(p @ p)
        if not (np.isfinite(pAp) and pAp > 0.0):
            return out(np.full(B, nan), 2, it - 1, r2)
        alpha = rho / pAp
        y = y + alpha * p
        r = r - alpha * (tp + lam * p)
        r2, rz = float(r @ r), float(r @ (r / M))
        if history:
            true = rhs - (tbar(y)[0] + lam * y)
            steps.append((np.sqrt(r2 / rhs2), np.sqrt(float(true @ true) / rhs2)))
        if not (np.isfinite(r2) and np.isfinite(rz)):
            return out(np.full(B, nan), 2, it, r2)
        if r2 <= tol * tol * rhs2:
            return out(y, 0, it, r2)
        p = r / M + (rz / rho) * p
        rho = rz
    return out(y, 1, int(max_iter), r2)
