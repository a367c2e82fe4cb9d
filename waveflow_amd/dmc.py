"""Fixed-node diffusion Monte Carlo with a fixed population, on the device: the ctypes surface of include/waveflow_dmc.h (PROTOTYPES,
DmcState), the three model-free calls `propose`, `accept` and `reconfigure`, the device-side `State` of a run, and `run` on top of
DeviceModel.dmc_init / DeviceModel.dmc_step.  The header states every formula; `philox_block`, `stream_id` and `comb_reference` restate the
random streams and the comb on the host (plain Python integers and numpy), which is what the tests hold the device to.

In one dimension the nodes of the antisymmetric ground state are the coincidence planes x_i = x_j, and a walker never leaves its ordering,
so the fixed-node energy is the exact eigenvalue for any reasonable psi: for 1-D soft-Coulomb He in the box of 10 that is -1.8161
(scratch/he1d_exact.py).  The comb runs every generation and the global weight is dropped, so the trial energy cancels out of the walk.

Everything runs on the GPU that holds the operands, on torch's current stream; there is no CPU fallback, and arguments are checked before
anything is launched (ValueError).
"""
import ctypes
import warnings

import numpy as np

from . import _accum, _lib

MAX_WALKERS = 1 << 20
RECORD = ("sum_w", "sum_w_e", "sum_w_e2", "accepted", "left_domain", "not_finite")
RING_RECORD = RECORD + ("e_growth", "e_trial")
STATS = ("w_max", "w_int", "stride", "offset", "max_multiplicity")
# imaginary time a population needs to forget the variational distribution: the gap of 1-D He to the next antisymmetric state is 0.176,
# a decay time of 5.7 a.u.; a run equilibrated for 3 a.u. landed 2 sigma high
HE_DECAY_TIME, MIN_EQUILIBRATION = 5.7, 30.0

_vp, _i32, _i64, _u64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
_ws = [_vp, _i64]    # (workspace_dev, workspace_bytes)


class DmcState(ctypes.Structure):
    """wf_dmc_state (include/waveflow_dmc.h)"""
    _fields_ = [("x_dev", _vp), ("psi_dev", _vp), ("grad_dev", _vp), ("e_loc_dev", _vp), ("counter_dev", _vp), ("e_trial_dev", _vp),
                ("ring_dev", _vp), ("status_dev", _vp), ("ring_len", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_state = ctypes.POINTER(DmcState)
# name -> (restype, argtypes): every function of include/waveflow_dmc.h, in its order (tests/test_dmc_host.py)
PROTOTYPES = {
    "wf_dmc_propose": (_i32, [_vp, _vp, _vp, _i64, _i32, _f32, _f64, _i32, _u64, _u64, _vp, _vp, _vp, _vp]),
    "wf_dmc_accept_workspace_bytes": (_i64, [_i64]),
    "wf_dmc_accept": (_i32, [_vp] * 9 + [_i64, _i32, _vp, _i32, _f64, _i32, _f64, _vp, _u64, _u64] + [_vp] * 5 + _ws + [_vp]),
    "wf_dmc_reconfigure_workspace_bytes": (_i64, [_i64, _i32]),
    "wf_dmc_reconfigure": (_i32, [_vp] * 5 + [_i64, _i32, _u64, _u64, _vp, _vp, _vp] + _ws + [_vp]),
    "wf_vqmc_dmc_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_vqmc_dmc_init": (_i32, [_vp, _state, _u64, _i64, _vp, _i32, _i32, _vp, _i32] + _ws + [_vp]),
    "wf_vqmc_dmc_step": (_i32, [_vp, _state, _u64, _i64, _vp, _i32, _f64, _i32, _f64] + _ws + [_vp]),
}


def lib():
    """The handle of _lib.lib() with PROTOTYPES applied to it."""
    return _lib.bound(PROTOTYPES)


# ---- the host's restatement of the random streams and of the comb

_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def stream_id(purpose, step, b=0):
    """The 64-bit stream id of the header: 2^63 | purpose << 60 | (step mod 2^40) << 20 | b."""
    return (1 << 63) | (int(purpose) << 60) | ((int(step) & ((1 << 40) - 1)) << 20) | int(b)


def philox_block(seed, stream, block=0):
    """The four 32-bit words of Philox4x32-10 for key `seed`, counter (block, 0, stream low, stream high): wf::Philox::refill."""
    seed, stream = int(seed) & _M64, int(stream) & _M64
    k0, k1 = seed & _M32, seed >> 32
    a = [int(block) & _M32, 0, stream & _M32, stream >> 32]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * a[0], 0xCD9E8D57 * a[2]
        a = [(p1 >> 32) ^ a[1] ^ k0, p1 & _M32, (p0 >> 32) ^ a[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return a


def comb_rand64(seed, step, purpose=2):
    """The comb's 64 random bits: word 0 << 32 | word 1 of block 0 of its stream (purpose 3, an init's comb: step 0)."""
    w = philox_block(seed, stream_id(purpose, 0 if purpose == 3 else step, 0))
    return (w[0] << 32) | w[1]


def comb_reference(w, rand64):
    """The comb of the header on the host -> (src int32 [B], (w_max, W_int, S, r, largest multiplicity), ok).  numpy uint64 prefix sums,
    searchsorted(side="right") for `the smallest j with C[j] > tooth`, Python integers for r."""
    w = np.asarray(w, dtype=np.float64)
    B = w.size
    valid = np.isfinite(w) & (w > 0)
    if not valid.any():
        return np.arange(B, dtype=np.int32), (0.0, 0, 0, 0, 1), False
    w_max = float(w[valid].max())
    scale = np.float64(4294967296.0) / np.float64(w_max)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.where(valid, w, 0.0) * scale
    q = np.where(t < 8589934592.0, np.where(valid, t, 0.0), 8589934592.0).astype(np.uint64)
    q[~valid] = 0
    C = np.cumsum(q, dtype=np.uint64)
    W = int(C[-1])
    S = W // B
    r = (int(rand64) * S) >> 64
    teeth = np.arange(B, dtype=np.uint64) * np.uint64(S) + np.uint64(r)   # (< W <= 2^53: no wrap)
    src = np.clip(np.searchsorted(C, teeth, side="right"), 0, B - 1).astype(np.int32)
    return src, (w_max, W, S, r, int(np.bincount(src, minlength=B).max())), True


# ---- checks: all of them before the first launch, none needs a GPU

def _check_tau(tau, e_cut=0.0):
    tau, e_cut = float(tau), float(e_cut)
    if not (np.isfinite(tau) and tau > 0.0):
        raise ValueError(f"the time step tau must be finite and positive, got {tau}")
    if not (np.isfinite(e_cut) and e_cut >= 0.0):
        raise ValueError(f"e_cut must be finite and >= 0 (0: no energy cut), got {e_cut}")
    return tau, e_cut


def _check_walkers(n):
    n = int(n)
    if not 1 <= n <= MAX_WALKERS:
        raise ValueError(f"a population holds 1 .. {MAX_WALKERS} walkers, got {n}")
    return n


def _float_tensor(t, shape, what, device=None, dtype=None):
    _accum.check_float_tensor(t, shape, what, "DMC has no CPU fallback", device, " on the device of the walkers", dtype)


def _check_state_arrays(x, psi, grad, e_loc=None):
    if not hasattr(x, "is_cuda") or x.dim() != 2:
        raise ValueError("x must be a 2-d torch tensor [B, D]")
    B, D = int(x.shape[0]), int(x.shape[1])
    if not 2 <= D <= 8:
        raise ValueError(f"DMC is built for 2 .. 8 coordinates per walker, got {D}")
    if B > MAX_WALKERS:
        raise ValueError(f"a population holds at most {MAX_WALKERS} walkers, got {B}")
    _float_tensor(x, (B, D), "x")
    _float_tensor(psi, (B,), "psi", x.device)
    _float_tensor(grad, (B, D), "grad", x.device)
    if e_loc is not None:
        _float_tensor(e_loc, (B,), "e_loc", x.device)
    return B, D


def _u64(v):
    return int(v) & _M64


# ---- the model-free calls

def propose(x, psi, grad, box, tau, seed, step, limit_drift=False, return_chi=False):
    """wf_dmc_propose on x [B, D], psi [B], grad [B, D] (contiguous float32 cuda) -> (x_new [B, D], flag int32 [B][, chi [B, D]])."""
    import torch
    B, D = _check_state_arrays(x, psi, grad)
    tau, _ = _check_tau(tau)
    box = float(box)
    if not (np.isfinite(box) and box > 0.0):
        raise ValueError(f"the box must be finite and positive, got {box}")
    x_new = torch.empty_like(x)
    flag = torch.empty(B, dtype=torch.int32, device=x.device)
    chi = torch.empty_like(x) if return_chi else None
    if B:
        with torch.cuda.device(x.device):
            _lib.check(lib().wf_dmc_propose(x.data_ptr(), psi.data_ptr(), grad.data_ptr(), B, D, box, tau, int(bool(limit_drift)), _u64(seed), _u64(step),
                                            x_new.data_ptr(), flag.data_ptr(), _lib.ptr(chi), _lib.stream_ptr(x.device)), "wf_dmc_propose")
    return (x_new, flag, chi) if return_chi else (x_new, flag)


def accept(x, psi, grad, e_loc, x_new, psi_new, grad_new, hdiag_new, flag, protons, tau, e_trial, seed, step, limit_drift=False, e_cut=0.0,
           details=False):
    """wf_dmc_accept: the state x, psi, grad, e_loc is updated IN PLACE -> (w float64 [B], record float64 [6][, logA float64 [B], u [B],
    accepted int32 [B]] with details).  e_trial: one float64 on the device, or a number."""
    import torch
    from .core import DeviceModel
    B, D = _check_state_arrays(x, psi, grad, e_loc)
    tau, e_cut = _check_tau(tau, e_cut)
    dev = x.device
    _float_tensor(x_new, (B, D), "x_new", dev)
    _float_tensor(psi_new, (B,), "psi_new", dev)
    _float_tensor(grad_new, (B, D), "grad_new", dev)
    _float_tensor(hdiag_new, (B, D), "hdiag_new", dev)
    _float_tensor(flag, (B,), "flag", dev, torch.int32)
    pr, n_pr = DeviceModel._protons(protons)
    if n_pr > 8:
        raise ValueError(f"at most 8 protons, got {n_pr}")
    if not hasattr(e_trial, "is_cuda"):
        e_trial = torch.tensor([float(e_trial)], dtype=torch.float64, device=dev)
    _float_tensor(e_trial, (1,), "e_trial", dev, torch.float64)
    w = torch.empty(B, dtype=torch.float64, device=dev)
    record = torch.zeros(len(RECORD), dtype=torch.float64, device=dev)
    logA = torch.empty(B, dtype=torch.float64, device=dev) if details else None
    u = torch.empty(B, dtype=torch.float32, device=dev) if details else None
    acc = torch.empty(B, dtype=torch.int32, device=dev) if details else None
    if B:
        L = lib()
        ws = DeviceModel._workspace(_lib.check(L.wf_dmc_accept_workspace_bytes(B), "wf_dmc_accept_workspace_bytes"), dev)
        with torch.cuda.device(dev):
            _lib.check(L.wf_dmc_accept(x.data_ptr(), psi.data_ptr(), grad.data_ptr(), e_loc.data_ptr(), x_new.data_ptr(), psi_new.data_ptr(),
                                       grad_new.data_ptr(), hdiag_new.data_ptr(), flag.data_ptr(), B, D, pr, n_pr, tau, int(bool(limit_drift)), e_cut,
                                       e_trial.data_ptr(), _u64(seed), _u64(step), w.data_ptr(), record.data_ptr(), _lib.ptr(logA), _lib.ptr(u),
                                       _lib.ptr(acc), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "wf_dmc_accept")
    return (w, record, logA, u, acc) if details else (w, record)


def reconfigure(x, psi, grad, e_loc, w, seed, step, status=None):
    """wf_dmc_reconfigure: the comb.  x, psi, grad, e_loc are gathered IN PLACE (through a workspace), w is reset to 1 -> (src int32 [B],
    stats int64 [5]: word 0 holds the bits of the float64 w_max -- stats[:1].view(torch.float64) --, then W_int, S, r, the largest multiplicity).
    status: one int64 on the device, incremented when no weight is finite and positive."""
    import torch
    from .core import DeviceModel
    B, D = _check_state_arrays(x, psi, grad, e_loc)
    dev = x.device
    _float_tensor(w, (B,), "w", dev, torch.float64)
    if status is not None:
        _float_tensor(status, (1,), "status", dev, torch.int64)
    src = torch.empty(B, dtype=torch.int32, device=dev)
    stats = torch.zeros(len(STATS), dtype=torch.int64, device=dev)
    if B:
        L = lib()
        ws = DeviceModel._workspace(_lib.check(L.wf_dmc_reconfigure_workspace_bytes(B, D), "wf_dmc_reconfigure_workspace_bytes"), dev)
        with torch.cuda.device(dev):
            _lib.check(L.wf_dmc_reconfigure(x.data_ptr(), psi.data_ptr(), grad.data_ptr(), e_loc.data_ptr(), w.data_ptr(), B, D, _u64(seed), _u64(step),
                                            src.data_ptr(), stats.data_ptr(), _lib.ptr(status), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                       "wf_dmc_reconfigure")
    return src, stats


# ---- with a model

class State:
    """The device side of a population: x [n, D], psi [n], grad [n, D], e_loc [n] (float32), counter and status (int64 [1]), e_trial
    (float64 [1]), ring (float64 [ring_len, 8], columns RING_RECORD; generation g in row g mod ring_len) and the wf_dmc_state that points at
    them (`.c`).  DeviceModel.make_dmc_state builds one."""

    def __init__(self, n_walkers, D, ring_len, device):
        import torch
        self.n, self.D, self.ring_len = _check_walkers(n_walkers), int(D), int(ring_len)
        if not 2 <= self.D <= 8:
            raise ValueError(f"DMC is built for 2 .. 8 coordinates per walker, got {self.D}")
        if not 1 <= self.ring_len < 1 << 31:
            raise ValueError(f"ring_len must be at least 1, got {ring_len}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("a DMC state lives on a cuda device: DMC has no CPU fallback")
        z = dict(device=self.device)
        self.x = torch.zeros(self.n, self.D, dtype=torch.float32, **z)
        self.psi = torch.zeros(self.n, dtype=torch.float32, **z)
        self.grad = torch.zeros(self.n, self.D, dtype=torch.float32, **z)
        self.e_loc = torch.zeros(self.n, dtype=torch.float32, **z)
        self.counter = torch.zeros(1, dtype=torch.int64, **z)
        self.status = torch.zeros(1, dtype=torch.int64, **z)
        self.e_trial = torch.zeros(1, dtype=torch.float64, **z)
        self.ring = torch.zeros(self.ring_len, len(RING_RECORD), dtype=torch.float64, **z)
        self.c = DmcState(self.x.data_ptr(), self.psi.data_ptr(), self.grad.data_ptr(), self.e_loc.data_ptr(), self.counter.data_ptr(),
                          self.e_trial.data_ptr(), self.ring.data_ptr(), self.status.data_ptr(), self.ring_len, 0)
        self.st = {"x": self.x, "ws": None}   # what DeviceModel._train_ws asks of a step's state: a device, a workspace that is kept

    def tensors(self):
        return (self.x, self.psi, self.grad, self.e_loc, self.counter, self.status, self.e_trial, self.ring)


def blocked_mean(values, n_blocks=20):
    """Mean of a correlated series and its standard error from `n_blocks` consecutive blocks of equal length (a remainder at the front is
    dropped from the error, not from the mean) -> (mean, stderr)."""
    v = np.asarray(values, dtype=np.float64)
    n_blocks = int(n_blocks)
    if n_blocks < 2 or v.size < n_blocks:
        raise ValueError(f"{v.size} values do not make {n_blocks} blocks (at least 2 blocks of at least one value)")
    per = v.size // n_blocks
    blocks = v[v.size - per * n_blocks:].reshape(n_blocks, per).mean(axis=1)
    return float(v.mean()), float(blocks.std(ddof=1) / np.sqrt(n_blocks))


def _check_run(n_walkers, tau, n_steps, n_equil, e_cut, n_blocks):
    n_walkers = _check_walkers(n_walkers)
    tau, e_cut = _check_tau(tau, e_cut)
    n_steps, n_equil, n_blocks = int(n_steps), int(n_equil), int(n_blocks)
    if n_equil < 0:
        raise ValueError(f"n_equil must be >= 0, got {n_equil}")
    if n_blocks < 2 or n_steps < n_blocks:
        raise ValueError(f"n_steps must be at least the {n_blocks} blocks of the error bar (at least 2), got {n_steps}")
    if tau * n_equil < MIN_EQUILIBRATION * (1.0 - 1e-12):   # (0.05 * 600 and its like are 30 up to rounding)
        warnings.warn(f"equilibration of {tau * n_equil:.3g} a.u. of imaginary time (tau * n_equil) is below {MIN_EQUILIBRATION:g} a.u.: the excited "
                      f"antisymmetric states of He decay with a time constant of {HE_DECAY_TIME} a.u. (gap 0.176), and a population that has not "
                      f"forgotten |psi|^2 reports an energy that is too high", RuntimeWarning, stacklevel=3)
    return n_walkers, tau, n_steps, n_equil, e_cut, n_blocks


def run(model, protons, n_walkers, tau, n_steps, n_equil, seed, exact_sampler=True, limit_drift=False, e_cut=0.0, use_graph=True, n_blocks=20,
        forward_walk=None):
    """A fixed-node DMC run: `n_walkers` walkers from |psi|^2 (DeviceModel.dmc_init), n_equil generations that are
    discarded, then n_steps measured ones (DeviceModel.dmc_step).  With use_graph the step is captured once (vqmc.capture_step; its warm-up
    call outside the capture is undone) and replayed; the host waits once, at the end.  -> dict:
      e_mixed, e_growth   per measured generation: sum w e / sum w, and E_T - log(sum w / n) / tau
      e_dmc, e_dmc_stderr mean of e_mixed and its blocking error over n_blocks blocks;  e_growth_mean, e_growth_stderr likewise
      acceptance          accepted moves / moves over the measured generations
      left_domain, not_finite   moves rejected for leaving the domain / for a value that is not finite (measured generations)
      status              combs that found no usable weight (0 in a healthy run);  generations: the device's counter;  ring: every record.
    tau * n_equil below 30 a.u. draws a RuntimeWarning (the He decay time is 5.7 a.u.); the run goes on.
    forward_walk: a dmc_observables.ForwardWalk for this population (model.make_forward_walk), or None.  With one, every generation is
    DeviceModel.dmc_fw_step (the same walk, bit for bit), the tracker's accumulators are zeroed behind the equilibration, and the dict gains
    "forward_walk": dmc_observables.result(forward_walk, n_blocks) -- per lag V_en, V_ee with blocking errors, densities, the pair distribution
    and the surviving share of ancestors.  n_slots * stride * tau below the decay time draws a RuntimeWarning."""
    import torch
    n_walkers, tau, n_steps, n_equil, e_cut, n_blocks = _check_run(n_walkers, tau, n_steps, n_equil, e_cut, n_blocks)
    fw = forward_walk
    if fw is not None:
        from . import dmc_observables
        if not isinstance(fw, dmc_observables.ForwardWalk) or fw.n != n_walkers:
            raise ValueError(f"forward_walk must be a ForwardWalk of {n_walkers} walkers")
        dmc_observables.warn_if_short(fw.n_slots, fw.stride, tau)
    total = n_equil + n_steps
    state = model.make_dmc_state(n_walkers, ring_len=total)
    nbytes = model.dmc_workspace_bytes(n_walkers) if fw is None else model.dmc_fw_workspace_bytes(n_walkers, fw.n_slots)
    state.st["ws"] = model._workspace(nbytes, state.device)   # allocated here, outside the capture
    model.dmc_init(state, seed, protons, exact_sampler=exact_sampler)
    if fw is not None:
        fw.reset()

    def step():
        if fw is None:
            model.dmc_step(state, seed, protons, tau, limit_drift=limit_drift, e_cut=e_cut)
        else:
            model.dmc_fw_step(state, fw, seed, protons, tau, limit_drift=limit_drift, e_cut=e_cut)
    launch = step
    if use_graph:
        from . import vqmc
        held = state.tensors() + (fw.tensors() if fw is not None else ())
        kept = [t.clone() for t in held]

        def warm_up():
            # one step outside the capture (the derivative entry grows the model's scratch there, not inside); what it did is taken back
            step()
            for t, k in zip(held, kept):
                t.copy_(k)
        launch = vqmc.capture_step(model, step, warm_up, "hipGraph capture of the DMC step failed")
    for i in range(total):
        if fw is not None and i == n_equil:
            fw.zero_accumulators()       # (on the stream, between two generations: the tags and the genealogy stay)
        launch()
    torch.cuda.synchronize(state.device)
    ring = state.ring.cpu().numpy()
    rec = ring[n_equil:]
    e_mixed, e_growth = rec[:, 1] / rec[:, 0], rec[:, 6]
    e_dmc, e_err = blocked_mean(e_mixed, n_blocks)
    g_mean, g_err = blocked_mean(e_growth, n_blocks)
    moves = float(n_walkers) * n_steps
    extra = {"forward_walk": dmc_observables.result(fw, n_blocks)} if fw is not None else {}
    return {**extra, "e_mixed": e_mixed, "e_growth": e_growth, "e_dmc": e_dmc, "e_dmc_stderr": e_err, "e_growth_mean": g_mean, "e_growth_stderr": g_err,
            "acceptance": float(rec[:, 3].sum() / moves), "left_domain": int(rec[:, 4].sum()), "not_finite": int(rec[:, 5].sum()),
            "status": int(state.status.item()), "generations": int(state.counter.item()), "ring": ring, "state": state}
