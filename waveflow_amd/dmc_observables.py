"""Observables of a fixed-node DMC walk by forward walking, on the device: the ctypes surface of include/waveflow_dmc_observe.h (PROTOTYPES,
DmcFw), the device-side `ForwardWalk` (the tracker and its accumulators), the model-free `update`, the host's restatement `Reference` /
`reference_update` (numpy integers, which is what the tests hold the device to), and `result` / `extrapolated` on top of them.

The walkers of a DMC generation sample psi Phi_0, so what they average (the mixed estimator) is biased to first order in psi's error for any
quantity that does not commute with H.  Counting an ancestor's configuration once per descendant it has K generations later samples
|Phi_0|^2 instead.  The tracker keeps n_slots tagged generations; accumulator 0 is the mixed estimator, accumulator j the forward-walking one
at a lag of j * stride generations.  The header states the rule.

Everything runs on the GPU that holds the operands, on torch's current stream; there is no CPU fallback, and arguments are checked before
anything is launched (ValueError).
"""
import ctypes
import warnings

import numpy as np

from . import _accum, _lib, dmc, observables

MAX_SLOTS = 16
COUNTS = ("counted", "skipped", "outside_density", "outside_pair")
SERIES = ("sum_v_en", "sum_v_ee", "counted", "distinct")
EMPTY = (1 << 64) - 1

_vp, _i32, _i64, _u64, _f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
_ws = [_vp, _i64]    # (workspace_dev, workspace_bytes)


class DmcFw(ctypes.Structure):
    """wf_dmc_fw (include/waveflow_dmc_observe.h)"""
    _fields_ = [("snap_dev", _vp), ("anc_dev", _vp), ("tag_dev", _vp), ("counts_dev", _vp), ("density_dev", _vp), ("pair_dev", _vp),
                ("sums_dev", _vp), ("measurements_dev", _vp), ("series_dev", _vp), ("n_slots", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("series_len", ctypes.c_int32), ("n_density_bins", ctypes.c_int32), ("n_pair_bins", ctypes.c_int32), ("lo", ctypes.c_float),
                ("hi", ctypes.c_float), ("reserved", ctypes.c_int32)]


_fw = ctypes.POINTER(DmcFw)
# name -> (restype, argtypes): every function of include/waveflow_dmc_observe.h, in its order (tests/test_dmc_observables_host.py)
PROTOTYPES = {
    "wf_dmc_fw_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "wf_dmc_fw_update": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _fw, _vp] + _ws + [_vp]),
    "wf_vqmc_dmc_fw_workspace_bytes": (_i64, [_vp, _i64, _i32]),
    "wf_vqmc_dmc_fw_step": (_i32, [_vp, ctypes.POINTER(dmc.DmcState), _fw, _u64, _i64, _vp, _i32, _f64, _i32, _f64] + _ws + [_vp]),
}


def lib():
    """The handle of _lib.lib() with PROTOTYPES applied to it."""
    return _lib.bound(PROTOTYPES)


# ---- checks: all of them before the first launch, none needs a GPU

def _check_tracker(n_walkers, D, n_slots, stride, n_density_bins, n_pair_bins, lo, hi, series_len):
    n = dmc._check_walkers(n_walkers)
    D, nd, npair, lo, hi = observables._check_geometry(D, n_density_bins, n_pair_bins, lo, hi)
    n_slots, stride, series_len = int(n_slots), int(stride), int(series_len)
    if not 1 <= n_slots <= MAX_SLOTS:
        raise ValueError(f"a tracker holds 1 .. {MAX_SLOTS} tag slots, got {n_slots}")
    if not 1 <= stride < 1 << 31:
        raise ValueError(f"stride must be at least 1 generation, got {stride}")
    if not 1 <= series_len < 1 << 31:
        raise ValueError(f"series_len must be at least 1, got {series_len}")
    return n, D, n_slots, stride, nd, npair, lo, hi, series_len


# ---- device side

class ForwardWalk:
    """The device side of forward walking for a population of n_walkers walkers of D coordinates: the tracker (snap float32 [n_slots, n, D],
    anc int32 [n_slots, n], tag int64 [n_slots], -1: empty), the accumulators (counts int64 [n_slots + 1, 4], density int64 [n_slots + 1, D,
    n_density_bins], pair int64 [n_slots + 1, n_pair_bins], sums float64 [n_slots + 1, 2, 2], measurements int64 [1], series float64
    [series_len, n_slots + 1, 4]) and the wf_dmc_fw that points at them (`.c`).  Row 0 of an accumulator is lag 0, row j lag j * stride
    generations.  DeviceModel.make_forward_walk builds one over the model's box."""

    def __init__(self, n_walkers, D, n_slots, stride, n_density_bins=200, n_pair_bins=200, lo=-10.0, hi=10.0, series_len=4096, device="cuda"):
        import torch
        (self.n, self.D, self.n_slots, self.stride, self.n_density_bins, self.n_pair_bins, self.lo, self.hi,
         self.series_len) = _check_tracker(n_walkers, D, n_slots, stride, n_density_bins, n_pair_bins, lo, hi, series_len)
        self.device = _accum.cuda_device(device, "a ForwardWalk", "forward walking has no CPU fallback")
        z, S = dict(device=self.device), self.n_slots
        self.snap = torch.zeros(S, self.n, self.D, dtype=torch.float32, **z)
        self.anc = torch.zeros(S, self.n, dtype=torch.int32, **z)
        self.tag = torch.full((S,), -1, dtype=torch.int64, **z)
        self.counts = torch.zeros(S + 1, len(COUNTS), dtype=torch.int64, **z)
        self.density = torch.zeros(S + 1, self.D, self.n_density_bins, dtype=torch.int64, **z)
        self.pair = torch.zeros(S + 1, self.n_pair_bins, dtype=torch.int64, **z)
        self.sums = torch.zeros(S + 1, 2, 2, dtype=torch.float64, **z)
        self.measurements = torch.zeros(1, dtype=torch.int64, **z)
        self.series = torch.zeros(self.series_len, S + 1, len(SERIES), dtype=torch.float64, **z)
        self.c = DmcFw(self.snap.data_ptr(), self.anc.data_ptr(), self.tag.data_ptr(), self.counts.data_ptr(),
                       self.density.data_ptr() if self.n_density_bins else None, self.pair.data_ptr() if self.n_pair_bins else None,
                       self.sums.data_ptr(), self.measurements.data_ptr(), self.series.data_ptr(), S, self.stride, self.series_len,
                       self.n_density_bins, self.n_pair_bins, self.lo, self.hi, 0)
        self.st = {"x": self.snap, "ws": None}   # what DeviceModel._train_ws asks of a step's state: a device, a workspace that is kept

    def accumulators(self):
        return (self.counts, self.density, self.pair, self.sums, self.measurements, self.series)

    def tensors(self):
        return (self.snap, self.anc, self.tag) + self.accumulators()

    def zero_accumulators(self):
        """Zeroes the accumulators, the series and the measurement count; the tags and the genealogy stay (legal in the middle of a run)."""
        for t in self.accumulators():
            t.zero_()
        return self

    def reset(self):
        """Every slot empty, everything else zero."""
        self.zero_accumulators()
        self.snap.zero_()
        self.anc.zero_()
        self.tag.fill_(-1)
        return self

    def lags(self):
        """The lag of every accumulator in generations: 0, stride, ..., n_slots * stride."""
        return np.arange(self.n_slots + 1) * self.stride


def _generation_tensor(generation, device):
    import torch
    if not hasattr(generation, "is_cuda"):
        g = int(generation)
        if not 0 <= g < EMPTY:
            raise ValueError(f"the generation must lie in 0 .. 2^64 - 2, got {generation}")
        return torch.tensor([g - (1 << 64) if g >= 1 << 63 else g], dtype=torch.int64, device=device)
    dmc._float_tensor(generation, (1,), "generation", device, torch.int64)
    return generation


def update(x, src, protons, fw, generation, workspace=None):
    """wf_dmc_fw_update: the walkers x [B, D] behind the comb (contiguous float32 cuda), the comb's parent indices src (int32 [B], or None for
    the identity), 1-D proton positions, a ForwardWalk and the generation -- a number, or one int64 on the device (the number of generations
    done, this one included).  Composes the genealogy, measures and retags as the header says; everything it changes lives in `fw`."""
    import torch
    from .core import DeviceModel
    if not hasattr(x, "is_cuda") or x.dim() != 2:
        raise ValueError("x must be a 2-d torch tensor [B, D]")
    B, D = int(x.shape[0]), int(x.shape[1])
    if not isinstance(fw, ForwardWalk):
        raise ValueError("fw must be a ForwardWalk")
    if (B, D) != (fw.n, fw.D):
        raise ValueError(f"the tracker holds {fw.n} walkers of {fw.D} coordinates, x has shape {[B, D]}")
    dmc._float_tensor(x, (B, D), "x", fw.device)
    if src is not None:
        dmc._float_tensor(src, (B,), "src", fw.device, torch.int32)
    pr, n_pr = DeviceModel._protons(protons)
    if n_pr > 8:
        raise ValueError(f"at most 8 protons, got {n_pr}")
    g = _generation_tensor(generation, fw.device)
    L = lib()
    if workspace is None:
        workspace = DeviceModel._workspace(_lib.check(L.wf_dmc_fw_workspace_bytes(B, D, fw.n_slots), "wf_dmc_fw_workspace_bytes"), fw.device)
    with torch.cuda.device(fw.device):
        _lib.check(L.wf_dmc_fw_update(x.data_ptr(), _lib.ptr(src), B, D, pr, n_pr, ctypes.byref(fw.c), g.data_ptr(), workspace.data_ptr(),
                                      workspace.numel(), _lib.stream_ptr(fw.device)), "wf_dmc_fw_update")


# ---- the host's restatement of the update rule

def potentials(x, protons):
    """V_en and V_ee of configurations x [n, D] by the fp32 rule of waveflow_observe.h in numpy float32 (every operation rounded on its own,
    protons outer, then d ascending; pairs i ascending, j < i) -> (v_en, v_ee), float32 [n]."""
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1.0)
    v_en, v_ee = np.zeros(x.shape[0], dtype=np.float32), np.zeros(x.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for p in np.asarray(protons, dtype=np.float32).reshape(-1):
            for d in range(x.shape[1]):
                r = p - x[:, d]
                v_en = v_en - one / np.sqrt(one + r * r)
        for i in range(x.shape[1]):
            for j in range(i):
                r = x[:, i] - x[:, j]
                v_ee = v_ee + one / np.sqrt(one + r * r)
    return v_en, v_ee


class Reference:
    """A tracker on the host, in numpy: the arrays of ForwardWalk under the same names (tag as Python integers, EMPTY: empty; measurements an
    integer).  reference_update advances it."""

    def __init__(self, n_walkers, D, n_slots, stride, n_density_bins, n_pair_bins, lo, hi, series_len):
        (self.n, self.D, self.n_slots, self.stride, self.n_density_bins, self.n_pair_bins, self.lo, self.hi,
         self.series_len) = _check_tracker(n_walkers, D, n_slots, stride, n_density_bins, n_pair_bins, lo, hi, series_len)
        S = self.n_slots
        self.snap = np.zeros((S, self.n, self.D), dtype=np.float32)
        self.anc = np.zeros((S, self.n), dtype=np.int32)
        self.tag = [EMPTY] * S
        self.zero_accumulators()

    def zero_accumulators(self):
        S = self.n_slots
        self.counts = np.zeros((S + 1, len(COUNTS)), dtype=np.int64)
        self.density = np.zeros((S + 1, self.D, self.n_density_bins), dtype=np.int64)
        self.pair = np.zeros((S + 1, self.n_pair_bins), dtype=np.int64)
        self.sums = np.zeros((S + 1, 2, 2), dtype=np.float64)
        self.measurements = 0
        self.series = np.zeros((self.series_len, S + 1, len(SERIES)), dtype=np.float64)
        return self


def _accumulate_reference(ref, lag, cfg, protons):
    """One lag's B configurations into accumulator `lag` -> (sum V_en, sum V_ee, counted); the bin rule of waveflow_observe.h in float32."""
    fin = np.isfinite(cfg).all(axis=1)
    ok = cfg[fin]
    ref.counts[lag, 0] += int(fin.sum())
    ref.counts[lag, 1] += int((~fin).sum())
    width = np.float32(ref.hi) - np.float32(ref.lo)
    if ref.n_density_bins:
        scale = np.float32(ref.n_density_bins) / width
        t = (ok - np.float32(ref.lo)) * scale
        inside = (t >= 0) & (t < np.float32(ref.n_density_bins))
        ref.counts[lag, 2] += int((~inside).sum())
        for d in range(ref.D):
            ref.density[lag, d] += np.bincount(t[inside[:, d], d].astype(np.int64), minlength=ref.n_density_bins)
    if ref.n_pair_bins:
        scale = np.float32(ref.n_pair_bins) / width
        for i in range(ref.D):
            for j in range(i):
                t = np.abs(ok[:, i] - ok[:, j]) * scale
                inside = (t >= 0) & (t < np.float32(ref.n_pair_bins))
                ref.counts[lag, 3] += int((~inside).sum())
                ref.pair[lag] += np.bincount(t[inside].astype(np.int64), minlength=ref.n_pair_bins)
    v_en, v_ee = (v.astype(np.float64) for v in potentials(ok, protons))
    ref.sums[lag] += [[v_en.sum(), (v_en * v_en).sum()], [v_ee.sum(), (v_ee * v_ee).sum()]]
    return float(v_en.sum()), float(v_ee.sum()), int(fin.sum())


def reference_update(ref, x, src, protons, generation):
    """The update of the header on the host: composes, measures and retags `ref` (a Reference) -> the measured configurations of this call as
    a list of (lag, float32 [B, D]), empty when the generation is no multiple of the stride.  Integers throughout; the fp64 sums are numpy's
    (the device's differ from them by the order of summation alone)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, g = ref.n, int(generation)
    if x.shape != (B, ref.D):
        raise ValueError(f"x must have shape {(B, ref.D)}, got {x.shape}")
    j = np.arange(B) if src is None else np.clip(np.asarray(src, dtype=np.int64), 0, B - 1)
    for s in range(ref.n_slots):
        if ref.tag[s] != EMPTY:
            ref.anc[s] = ref.anc[s][j]            # (fancy indexing builds a new array: never in place)
    if g % ref.stride:
        return []
    row = ref.series[ref.measurements % ref.series_len]
    row[:] = 0.0
    measured = [(0, x, B)]
    for s in range(ref.n_slots):
        t = ref.tag[s]
        if t == EMPTY or g < t:
            continue
        lag = (g - t) // ref.stride
        if 1 <= lag <= ref.n_slots:
            measured.append((lag, ref.snap[s][ref.anc[s]], int(np.unique(ref.anc[s]).size)))
    for lag, cfg, distinct in measured:
        s_en, s_ee, n = _accumulate_reference(ref, lag, cfg, protons)
        row[lag] = [s_en, s_ee, n, distinct]
    ref.measurements += 1
    s_star = (g // ref.stride) % ref.n_slots
    ref.snap[s_star] = x
    ref.anc[s_star] = np.arange(B, dtype=np.int32)
    ref.tag[s_star] = g
    return [(lag, cfg.copy()) for lag, cfg, _ in measured]


# ---- results

def _host(fw):
    if isinstance(fw, Reference):
        return (fw.counts, fw.density, fw.pair, fw.sums, int(fw.measurements), fw.series)
    counts, density, pair, sums, measurements, series = (t.cpu().numpy() for t in fw.accumulators())
    return counts, density, pair, sums, int(measurements[0]), series


def result(fw, n_blocks=20):
    """What a ForwardWalk (or a Reference) holds, per lag (arrays of n_slots + 1 entries, index 0 the mixed estimator) -> dict:
      lag (generations), n (configurations counted), n_skipped, outside_density, outside_pair, n_measurements (of the series that served the lag)
      v_en, v_ee                 sum / n over everything accumulated
      v_en_stderr, v_ee_stderr   the blocking error (dmc.blocked_mean, n_blocks blocks) of the per-measurement means sum V / counted kept in the
                                 series; NaN for a lag with fewer than n_blocks measurements in the series
      distinct_fraction          mean over the series of distinct ancestors / counted: the share of the tagged walkers that still have
                                 descendants at that lag (1 for lag 0)
      density_x, density [lags, bins] (sum over the columns), density_by_column [lags, D, bins], pair_r, pair [lags, bins]: normalised as
      observables.Totals.result does, per lag by its own n.
    It waits for the device."""
    counts, density, pair, sums, m, series = _host(fw)
    L, S = fw.series_len, fw.n_slots
    kept = min(m, L)
    rows = series[[(m - kept + i) % L for i in range(kept)]] if kept else series[:0]   # in the order they were measured
    n = counts[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        out = {"lag": np.arange(S + 1) * fw.stride, "n": counts[:, 0].copy(), "n_skipped": counts[:, 1].copy(), "outside_density": counts[:, 2].copy(),
               "outside_pair": counts[:, 3].copy(), "v_en": sums[:, 0, 0] / n, "v_ee": sums[:, 1, 0] / n, "measurements": m}
    err = np.full((2, S + 1), np.nan)
    frac, served = np.full(S + 1, np.nan), np.zeros(S + 1, dtype=np.int64)
    for j in range(S + 1):
        r = rows[rows[:, j, 2] > 0, j] if kept else rows[:0, 0]
        served[j] = r.shape[0]
        if r.shape[0]:
            frac[j] = float((r[:, 3] / r[:, 2]).mean())
        if r.shape[0] >= max(int(n_blocks), 2):
            err[0, j] = dmc.blocked_mean(r[:, 0] / r[:, 2], n_blocks)[1]
            err[1, j] = dmc.blocked_mean(r[:, 1] / r[:, 2], n_blocks)[1]
    out.update(v_en_stderr=err[0], v_ee_stderr=err[1], distinct_fraction=frac, n_measurements=served)
    span = np.float64(fw.hi) - np.float64(fw.lo)
    norm = np.where(n > 0, n, np.nan)
    if fw.n_density_bins:
        w = span / fw.n_density_bins
        out["density_x"] = fw.lo + (np.arange(fw.n_density_bins) + 0.5) * w
        out["density_by_column"] = density / (norm[:, None, None] * w)
        out["density"] = density.sum(axis=1) / (norm[:, None] * w)
    if fw.n_pair_bins:
        w = span / fw.n_pair_bins
        out["pair_r"] = (np.arange(fw.n_pair_bins) + 0.5) * w
        out["pair"] = pair / (norm[:, None] * w)
    return out


def extrapolated(mixed, vmc):
    """The extrapolated estimator 2 * mixed - VMC, which removes the first-order bias of the mixed estimator without any lag: `mixed` is a
    result() dict (its lag 0 is used), `vmc` an observables.Totals of |psi|^2 with the same geometry (or its result()) -> dict with v_en, v_ee
    and, where both sides hold them, density, density_by_column and pair."""
    v = vmc.result() if isinstance(vmc, observables.Totals) else vmc
    out = {"v_en": 2.0 * float(mixed["v_en"][0]) - float(v["v_en"]), "v_ee": 2.0 * float(mixed["v_ee"][0]) - float(v["v_ee"])}
    for name, grid in (("density", "density_x"), ("density_by_column", "density_x"), ("pair", "pair_r")):
        if name in mixed and name in v:
            a, b = np.asarray(mixed[name][0]), np.asarray(v[name])
            if a.shape != b.shape or not np.allclose(mixed[grid], v[grid], rtol=0.0, atol=1e-6):
                raise ValueError(f"{name}: the two sides were binned differently ({a.shape} against {b.shape}, or another range)")
            out[name] = 2.0 * a - b
            out[grid] = np.asarray(mixed[grid])
    return out


def warn_if_short(n_slots, stride, tau):
    """RuntimeWarning when the longest lag n_slots * stride * tau is below the decay time of the excited antisymmetric states of He: the
    forward-walking estimator has then not converged to |Phi_0|^2 at any lag."""
    span = int(n_slots) * int(stride) * float(tau)
    if span < dmc.HE_DECAY_TIME:
        warnings.warn(f"the longest forward-walking lag is {span:.3g} a.u. of imaginary time (n_slots * stride * tau), below the decay time of "
                      f"{dmc.HE_DECAY_TIME} a.u.: no lag has forgotten the mixed distribution", RuntimeWarning, stacklevel=3)
