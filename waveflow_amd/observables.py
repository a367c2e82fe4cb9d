"""Observables of a trained psi, measured on the device: the ctypes surface of include/waveflow_observe.h (PROTOTYPES, ObserveAcc), the
device-side `Accumulator`, the host-side `Totals`, and `accumulate`, `local_observables` and `measure` on top of them.

Per walker the library forms five fp32 values (SCALARS): the local energy E_L = H psi / (psi + 1e-8), its kinetic part in the Laplacian form
T_lap = -1/2 lap psi / psi, the kinetic energy in the gradient form T_grad = 1/2 |grad psi / psi|^2, and the electron-nucleus and
electron-electron soft-Coulomb energies V_en and V_ee; E_L = T_lap + V_en + V_ee up to fp32 rounding, and <T_lap> = <T_grad> over |psi|^2.
It keeps fp64 sums of each value and its square, integer histograms of the one-body density (per coordinate column) and of the pair distance,
and four counters -- all on the device, over any number of steps.  The fp64 sums are bitwise reproducible (their order depends on the batch
size alone; no floating-point atomics), so `Totals` of two runs can be compared, merged and all-reduced exactly.

Everything runs on the GPU that holds the operands, on torch's current stream; there is no CPU fallback, and arguments are checked before
anything is launched (ValueError).
"""
import ctypes

import numpy as np

from . import _accum, _lib

SCALARS = ("e_loc", "t_lap", "t_grad", "v_en", "v_ee")
MAX_DENSITY_BINS, MAX_PAIR_BINS = 512, 1024

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_ws = [_vp, _i64]    # (workspace_dev, workspace_bytes)
_NO_CPU = "the observables have no CPU fallback"


class ObserveAcc(ctypes.Structure):
    """wf_observe_acc (include/waveflow_observe.h)"""
    _fields_ = [("sums_dev", _vp), ("counts_dev", _vp), ("density_dev", _vp), ("pair_dev", _vp), ("n_density_bins", ctypes.c_int32),
                ("n_pair_bins", ctypes.c_int32), ("lo", ctypes.c_float), ("hi", ctypes.c_float)]


# name -> (restype, argtypes): every function of include/waveflow_observe.h, in its order (tests/test_observables_host.py)
PROTOTYPES = {
    "wf_observe_workspace_bytes": (_i64, [_i64]),
    "wf_observe_accumulate": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, ctypes.POINTER(ObserveAcc), _vp] + _ws + [_vp]),
    "wf_vqmc_observe_step_workspace_bytes": (_i64, [_vp, _i64]),
    "wf_vqmc_observe_step": (_i32, [_vp, ctypes.POINTER(ObserveAcc), _vp, ctypes.c_uint64, _i64, _vp, _i32, _i32, _vp, _i32, _vp] + _ws + [_vp]),
}


def lib():
    """The handle of _lib.lib() with PROTOTYPES applied to it."""
    return _lib.bound(PROTOTYPES)


# ---- checks: all of them before the first launch, none needs a GPU

def _check_geometry(D, n_density_bins, n_pair_bins, lo, hi):
    D, nd, npair = int(D), int(n_density_bins), int(n_pair_bins)
    if not 2 <= D <= 8:
        raise ValueError(f"observables are built for 2 .. 8 coordinates per walker, got {D}")
    if not 0 <= nd <= MAX_DENSITY_BINS or not 0 <= npair <= MAX_PAIR_BINS:
        raise ValueError(f"bin counts must lie in 0 .. {MAX_DENSITY_BINS} (density) and 0 .. {MAX_PAIR_BINS} (pair), got {nd} and {npair}")
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(np.float32(hi) - np.float32(lo))):
        raise ValueError(f"the range must be finite with lo < hi, got [{lo}, {hi})")
    return D, nd, npair, lo, hi


def _check_step(batch, n_dim, walkers, out_walkers, values):
    """The arguments of one measurement step (core.DeviceModel.observe_step): `walkers` (read) and `out_walkers` (written) are contiguous
    float32 cuda tensors [batch, n_dim] or None, at most one of them given; `values` is a contiguous float32 cuda tensor [batch, 5] or None."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"{batch} walkers per step: at least 1")
    _accum.check_step_walkers(batch, n_dim, walkers, out_walkers, _NO_CPU, (("values", values, (batch, len(SCALARS))),))
    return batch


# ---- host side

class Totals:
    """What an Accumulator held, on the host: sums [5, 2] float64 (sum v, sum v^2 per scalar of SCALARS), counts [4] int64 (walkers counted,
    walkers skipped, coordinates outside the density range, pairs outside the pair range), density [D, n_density_bins] and pair [n_pair_bins]
    int64, and the geometry (D, the bin counts, lo, hi).  Plain numpy."""

    def __init__(self, D, n_density_bins, n_pair_bins, lo, hi, sums=None, counts=None, density=None, pair=None):
        self.D, self.n_density_bins, self.n_pair_bins, self.lo, self.hi = _check_geometry(D, n_density_bins, n_pair_bins, lo, hi)
        shapes = {"sums": ((len(SCALARS), 2), np.float64), "counts": ((4,), np.int64), "density": ((self.D, self.n_density_bins), np.int64),
                  "pair": ((self.n_pair_bins,), np.int64)}
        for name, given in (("sums", sums), ("counts", counts), ("density", density), ("pair", pair)):
            shape, dtype = shapes[name]
            a = np.zeros(shape, dtype) if given is None else np.array(given, dtype=dtype)
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            setattr(self, name, a)

    def geometry(self):
        return (self.D, self.n_density_bins, self.n_pair_bins, self.lo, self.hi)

    def merge(self, other):
        """self += other (another run, another rank): sums in fp64, everything else in integers.  ValueError on a different geometry."""
        if self.geometry() != other.geometry():
            raise ValueError(f"cannot merge totals of geometry {other.geometry()} into {self.geometry()}")
        self.sums = self.sums + other.sums
        self.counts = self.counts + other.counts
        self.density = self.density + other.density
        self.pair = self.pair + other.pair
        return self

    def all_reduce(self, group=None):
        """SUM over the ranks of `group`, in place: one all-reduce for the fp64 part, one for the int64 part (distributed._all_reduce_sum).
        This is how ranks that measured with different seeds combine.  Every rank must hold the same geometry.  The two buffers are host
        tensors under gloo; under any other backend (nccl: RCCL reduces device tensors only) they are moved to the current cuda device,
        reduced there and copied back."""
        f, i = _accum.all_reduce_totals(self.sums, np.concatenate([self.counts, self.density.reshape(-1), self.pair]), group)
        self.sums = f.reshape(len(SCALARS), 2)
        nd = self.D * self.n_density_bins
        self.counts, self.density, self.pair = i[:4].copy(), i[4:4 + nd].reshape(self.D, self.n_density_bins).copy(), i[4 + nd:].copy()
        return self

    def result(self):
        """-> dict.  Per scalar s of SCALARS: s (mean = S1 / n), s + "_variance" ((S2 - n mean^2) / (n - 1)), s + "_stderr" (sqrt(variance / n)).
        n, n_skipped, outside_density, outside_pair: the counters.  density_x (bin centres), density[k] = sum_d counts[d][k] / (n width)
        (integrates to D minus the outside share), density_by_column [D, bins] (each integrates to 1 minus its outside share), pair_r and
        pair[k] = counts[k] / (n width) (integrates to D (D - 1) / 2 minus the outside share).

        The exact samplers draw independent walkers, so the standard error needs no blocking.  The T_grad estimator has infinite variance at
        the nodes of psi -- its integrand goes like 1 / d^2 against a density that goes like d^2 at distance d from a node, so the square of
        the integrand is not integrable -- and its error bar is only indicative; T_lap carries the honest one."""
        n = int(self.counts[0])
        out = {"n": n, "n_skipped": int(self.counts[1]), "outside_density": int(self.counts[2]), "outside_pair": int(self.counts[3])}
        for k, name in enumerate(SCALARS):
            s1, s2 = float(self.sums[k, 0]), float(self.sums[k, 1])
            mean = s1 / n if n > 0 else float("nan")
            var = (s2 - n * mean * mean) / (n - 1) if n > 1 else float("nan")
            out[name] = mean
            out[name + "_variance"] = var
            out[name + "_stderr"] = float(np.sqrt(max(var, 0.0) / n)) if n > 1 else float("nan")
        span = np.float64(self.hi) - np.float64(self.lo)
        norm = float(n) if n > 0 else float("nan")
        if self.n_density_bins > 0:
            w = span / self.n_density_bins
            out["density_x"] = self.lo + (np.arange(self.n_density_bins) + 0.5) * w
            out["density_by_column"] = self.density / (norm * w)
            out["density"] = self.density.sum(axis=0) / (norm * w)
        if self.n_pair_bins > 0:
            w = span / self.n_pair_bins
            out["pair_r"] = (np.arange(self.n_pair_bins) + 0.5) * w
            out["pair"] = self.pair / (norm * w)
        return out

    def arrays(self):
        """The totals as a dict of numpy arrays (np.savez(**totals.arrays()); Totals.from_arrays reads it back)."""
        return {"sums": self.sums, "counts": self.counts, "density_counts": self.density, "pair_counts": self.pair,
                "geometry": np.array([self.D, self.n_density_bins, self.n_pair_bins], dtype=np.int64), "range": np.array([self.lo, self.hi], dtype=np.float32)}

    @classmethod
    def from_arrays(cls, z):
        D, nd, npair = (int(v) for v in z["geometry"])
        return cls(D, nd, npair, float(z["range"][0]), float(z["range"][1]), z["sums"], z["counts"], z["density_counts"], z["pair_counts"])


# ---- device side

class Accumulator:
    """The device side of a measurement: four tensors (sums float64 [5, 2], counts int64 [4], density int64 [D, n_density_bins], pair int64
    [n_pair_bins]) and the wf_observe_acc that points at them (`.c`).  Library calls ADD to them; `reset()` zeroes them, `totals()` copies them
    to the host (it waits for the device).  lo, hi: the density range [lo, hi) -- the pair range is [0, hi - lo) -- for a model built by
    model_factory.get_waveflow_model the box [-box_size, box_size), which is where BoxTransformLayer puts every walker (a coordinate exactly at
    box_size, like anything else outside, is counted in counts[2] and in no bin)."""

    def __init__(self, D, n_density_bins=200, n_pair_bins=200, lo=None, hi=None, device=None, model=None):
        import torch
        if (lo is None or hi is None) and model is None:
            raise ValueError("lo and hi, or the model whose box gives them")
        if lo is None:
            lo = -float(model.desc.box_size)
        if hi is None:
            hi = float(model.desc.box_size)
        self.D, self.n_density_bins, self.n_pair_bins, self.lo, self.hi = _check_geometry(D, n_density_bins, n_pair_bins, lo, hi)
        if device is None:
            device = f"cuda:{model.device}" if model is not None else "cuda"
        self.device = _accum.cuda_device(device, "an Accumulator", _NO_CPU)
        self.sums = torch.zeros(len(SCALARS), 2, dtype=torch.float64, device=self.device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.density = torch.zeros(self.D, self.n_density_bins, dtype=torch.int64, device=self.device)
        self.pair = torch.zeros(self.n_pair_bins, dtype=torch.int64, device=self.device)
        self.c = ObserveAcc(self.sums.data_ptr(), self.counts.data_ptr(), self.density.data_ptr() if self.n_density_bins else None,
                            self.pair.data_ptr() if self.n_pair_bins else None, self.n_density_bins, self.n_pair_bins, self.lo, self.hi)
        self.st = {"x": self.sums, "ws": None}   # what DeviceModel._train_ws asks of a step's state: a device, a workspace that is kept

    def reset(self):
        for t in (self.sums, self.counts, self.density, self.pair):
            t.zero_()
        return self

    def totals(self):
        return Totals(self.D, self.n_density_bins, self.n_pair_bins, self.lo, self.hi, self.sums.cpu().numpy(), self.counts.cpu().numpy(),
                      self.density.cpu().numpy(), self.pair.cpu().numpy())


def accumulate(x, psi, grad, hdiag, protons, acc=None, return_values=False, workspace=None):
    """wf_observe_accumulate on x [B, D], psi [B], grad [B, D], hdiag [B, D] (contiguous float32 cuda, as DeviceModel.psi_derivatives returns
    them) and 1-D proton positions: adds the batch to `acc` (an Accumulator, or None with return_values) and returns the per-walker values
    [B, 5] (float32 cuda, columns in the order of SCALARS; skipped walkers included, as computed) when return_values is set, else None."""
    import torch
    from .core import DeviceModel
    if not hasattr(x, "is_cuda") or x.dim() != 2:
        raise ValueError("x must be a 2-d torch tensor [B, D]")
    B, D = int(x.shape[0]), int(x.shape[1])
    if not 2 <= D <= 8:
        raise ValueError(f"observables are built for 2 .. 8 coordinates per walker, got {D}")
    if not x.is_cuda:
        raise ValueError("x must be a cuda tensor: the observables have no CPU fallback")
    for what, t, width in (("x", x, D), ("psi", psi, 0), ("grad", grad, D), ("hdiag", hdiag, D)):
        _accum.check_float_tensor(t, (B, width) if width else (B,), what, _NO_CPU, x.device, " on the device of the walkers")
    if acc is None and not return_values:
        raise ValueError("nothing to do: neither an accumulator nor return_values")
    if acc is not None and (acc.D != D or acc.device != x.device):
        raise ValueError(f"the accumulator holds {acc.D} columns on {acc.device}, the walkers have {D} on {x.device}")
    pr, n_pr = DeviceModel._protons(protons)
    if n_pr > 8:
        raise ValueError(f"at most 8 protons, got {n_pr}")
    values = torch.empty(B, len(SCALARS), dtype=torch.float32, device=x.device) if return_values else None
    if B == 0:
        return values
    L = lib()
    if acc is not None and workspace is None:
        workspace = DeviceModel._workspace(_lib.check(L.wf_observe_workspace_bytes(B), "wf_observe_workspace_bytes"), x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.wf_observe_accumulate(x.data_ptr(), psi.data_ptr(), grad.data_ptr(), hdiag.data_ptr(), B, D, pr, n_pr,
                                           ctypes.byref(acc.c) if acc is not None else None, _lib.ptr(values),
                                           _lib.ptr(workspace), workspace.numel() if workspace is not None else 0, _lib.stream_ptr(x.device)),
                   "wf_observe_accumulate")
    return values


def local_observables(model, x, protons):
    """The five values of SCALARS per walker -> float32 cuda [B, 5], through model.psi_derivatives(x, hessian_diag=True, return_psi=True)."""
    t, _ = model._to_dev(x)
    grad, hdiag, psi = model.psi_derivatives(t, hessian_diag=True, return_psi=True)
    return accumulate(t, psi, grad, hdiag, protons, return_values=True)


def measure(model, protons, n_walkers, batch, seed, exact_sampler=True, acc=None, use_graph=True):
    """ceil(n_walkers / batch) measurement steps of `batch` walkers each (DeviceModel.observe_step: the sampler stream `seed`, advanced by a
    device counter that starts at 0), added to `acc` (default: a new Accumulator over the model's box) -> its Totals.  With use_graph
    the step is captured once (vqmc.capture_step; its warm-up call outside the capture is undone) and replayed; the host waits once, at the end."""
    import torch
    n_walkers, batch = int(n_walkers), int(batch)
    if n_walkers < 1 or batch < 1:
        raise ValueError("n_walkers and batch must be >= 1")
    if acc is None:
        acc = Accumulator(model.D, model=model)
    counter = torch.zeros(1, dtype=torch.int64, device=acc.device)

    def step():
        model.observe_step(acc, counter, seed, batch, protons, exact_sampler=exact_sampler)
    _accum.measure_loop(model, acc, step, -(-n_walkers // batch), model.observe_step_workspace_bytes(batch),
                        (acc.sums, acc.counts, acc.density, acc.pair, counter), "measurement", use_graph)
    return acc.totals()
