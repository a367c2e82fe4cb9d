"""The spline closures' shared machinery: knots, initial parameters, the on-disk table cache, and the lazily created wf_spline handle
(include/waveflow_hip.h, wf_spline_*) the closures launch on.  Nothing here touches a GPU before the first closure call."""
import ctypes
import os

import numpy as np

from .. import _lib
from ..flows import as_generator, seed_from
from ..utils import table_cache

NAMES = {_lib.SPLINE_I: "I", _lib.SPLINE_M: "M", _lib.SPLINE_B: "B"}
MAX_BASES = 64
P = _lib.ptr


def make_knots(kind, k, n_internal_knots):
    """The reference's lines (isplines_jax.py:90-92, msplines_jax.py:73-75, bsplines_jax.py:58-60): ends repeated k + 1 times (I, B) or
    k times (M)."""
    internal_knots = np.linspace(0, 1, n_internal_knots)
    if kind == _lib.SPLINE_B:
        internal_knots = np.repeat(internal_knots, ((internal_knots == internal_knots[0]) * k + 1).clip(min=1))
        return np.repeat(internal_knots, ((internal_knots == internal_knots[-1]) * k + 1).clip(min=1))
    rep = k + 1 if kind == _lib.SPLINE_I else k
    internal_knots = np.repeat(internal_knots, ((internal_knots == internal_knots[0]) * rep).clip(min=1))
    return np.repeat(internal_knots, ((internal_knots == internal_knots[-1]) * rep).clip(min=1))


def n_bases(kind, k, n_internal_knots):
    n_knots = len(make_knots(kind, k, n_internal_knots))
    return n_knots - k - 1 if kind == _lib.SPLINE_B else n_knots - k


def check_options(cardinal_splines, use_cached_bases):
    if not cardinal_splines:
        raise NotImplementedError("non-cardinal knots are not built (only cardinal splines can be cached, isplines_jax.py:106-108)")
    if not use_cached_bases:
        raise NotImplementedError("use_cached_bases=False (the closures run on the cached tables) is not built")


def load_tables(kind, k, n_internal_knots, n_mesh, root):
    """Tables as the reference's init_fun gets them: every file found under the reference's names in `root` is loaded, the others are
    built (wf_tables_build, fp64) and saved there.  -> (tables [4][nb][n_mesh], aux or None); for B tables are the orthogonalised
    ones and aux = (plain [4][nb][n_mesh], b_to_ob, ob_to_b)."""
    os.makedirs(root, exist_ok=True)
    names = table_cache.cache_file_names(NAMES[kind], k, n_internal_knots, n_mesh)
    files = list(names["nd"]) + (list(names["ob"]) + [names["b_to_ob"], names["ob_to_b"]] if kind == _lib.SPLINE_B else [])
    paths = [os.path.join(root, f) for f in files]
    if not all(os.path.exists(p) for p in paths):
        from ..core import build_tables
        built = [t for t in build_tables(kind, k, n_internal_knots, n_mesh)]
        if kind == _lib.SPLINE_B:
            ob, b2o, o2b = build_tables(_lib.SPLINE_OB, k, n_internal_knots, n_mesh)
            built = built + [t for t in ob] + [b2o, o2b]
        for p, arr in zip(paths, built):
            if not os.path.exists(p):
                np.save(p, np.ascontiguousarray(arr, dtype=np.float64))
    arrs = [np.load(p).astype(np.float64) for p in paths]
    if kind == _lib.SPLINE_B:
        return np.stack(arrs[4:8]), (np.stack(arrs[:4]), arrs[8], arrs[9])
    return np.stack(arrs[:4]), None


def initial_params(kind, rng, nb, zero_border):
    """Shapes and normalisation of the reference (isplines_jax.py:95-101, msplines_jax.py:79-83, bsplines_jax.py:65-66); the draws
    follow numpy, not JAX's threefry."""
    g = as_generator(rng)
    if kind == _lib.SPLINE_B:
        p = g.uniform(-1, 1, size=(nb,)).astype(np.float32)
        return p / np.sqrt(np.sum(p ** 2))
    p = np.abs(g.uniform(0, 1, size=(nb - 2 if zero_border else nb,)).astype(np.float32))
    return p / p.sum()


class DeviceSpline:
    """One wf_spline, created on the first call on torch's current device (a machine without one raises WfError WF_ERR_NO_DEVICE there)."""

    def __init__(self, kind, k, n_internal_knots, n_mesh, zero_border, left, right, tables, aux):
        self.kind, self.k, self.n_mesh, self.zero_border = kind, k, n_mesh, bool(zero_border)
        self.desc = _lib.SplineDesc(kind, k, n_internal_knots, n_mesh, int(bool(zero_border)), _lib.BC.from_dict(left), _lib.BC.from_dict(right))
        self.nb = tables.shape[1]
        self.nc = self.nb - 2 if zero_border else self.nb
        self.tables = np.ascontiguousarray(tables, dtype=np.float64)
        self.aux = None
        if aux is not None:
            plain, b2o, o2b = aux
            self.aux = np.ascontiguousarray(np.concatenate([np.ravel(plain), np.ravel(b2o), np.ravel(o2b)]), dtype=np.float64)
        self._h = None
        self._L = _lib.lib()

    def handle(self):
        if self._h is None:
            import torch
            dev = torch.cuda.current_device() if torch.cuda.is_available() else 0
            h = ctypes.c_void_p()
            aux = self.aux.ctypes.data if self.aux is not None else None
            _lib.call("wf_spline_create", ctypes.byref(self.desc), self.tables.ctypes.data, aux, dev, ctypes.byref(h))
            self._h, self._dev = h, dev
        return self._h

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            self._L.wf_spline_destroy(self._h)
            self._h = None

    # -- plumbing
    def _t(self, a, shape_last=None):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
        return t.to(device=f"cuda:{self._dev}", dtype=torch.float32).contiguous()

    def _stream(self):
        return _lib.stream_ptr(self._dev)

    def _rows(self, params, width):
        h = self.handle()
        c = self._t(params)
        if c.dim() != 2 or c.shape[1] != width:
            raise ValueError(f"params must be [N, {width}], got {tuple(c.shape)}")
        return h, c

    # -- closures
    def apply(self, params, x, nd=0, grad=False):
        import torch
        h, c = self._rows(params, self.nc)
        xt = self._t(x).reshape(-1)
        if xt.numel() != c.shape[0]:
            raise ValueError("params and x must have the same number of rows")
        y = torch.empty(c.shape[0], device=c.device, dtype=torch.float32)
        dy = torch.empty_like(y) if grad else None
        _lib.call("wf_spline_apply", h, P(c), c.shape[0], P(xt), nd, P(y), P(dy), self._stream())
        return (y, dy) if grad else y

    def reverse(self, params, y, tol):
        import torch
        h, c = self._rows(params, self.nc)
        yt = self._t(y).reshape(-1)
        if yt.numel() != c.shape[0]:
            raise ValueError("params and y must have the same number of rows")
        x = torch.empty(c.shape[0], device=c.device, dtype=torch.float32)
        _lib.call("wf_spline_reverse", h, P(c), c.shape[0], P(yt), float(tol), P(x), self._stream())
        return x

    def rowwise(self, fn, weights):
        import torch
        h = self.handle()
        w = self._t(weights)
        if w.dim() != 2:
            raise ValueError("weights must be [N, nw]")
        out = torch.empty_like(w)
        _lib.call(fn, h, P(w), w.shape[0], w.shape[1], P(out), self._stream())
        return out

    def sample(self, rng, params, num_samples, max_proposals):
        import torch
        h, c = self._rows(params, self.nc)
        x = torch.empty((c.shape[0], int(num_samples)), device=c.device, dtype=torch.float32)
        _lib.call("wf_spline_sample", h, seed_from(rng), P(c), c.shape[0], int(num_samples), int(max_proposals), P(x), self._stream())
        bad = torch.isnan(x).any(dim=1).nonzero()
        if bad.numel():
            raise RuntimeError(f"sample_fun_vec: row {int(bad[0, 0])} exhausted {max_proposals} proposals for a slot (acceptance rate too "
                               f"small for this bound; raise max_proposals)")
        return x


def build_closures(kind, rng, k, n_internal_knots, cardinal_splines, zero_border, use_cached_bases, cached_bases_path_root, n_mesh_points,
                   constraints_dict_left, constraints_dict_right):
    """-> (initial_params, knots, DeviceSpline) for one init_fun call."""
    check_options(cardinal_splines, use_cached_bases)
    nb = n_bases(kind, k, n_internal_knots)
    if nb > MAX_BASES:
        raise _lib.WfError(_lib.ERR_UNSUPPORTED, f"{NAMES[kind]}-spline with {nb} bases (at most {MAX_BASES})")
    for d in (constraints_dict_left or {}, constraints_dict_right or {}):
        if len(d) > _lib.WF_MAX_BC or any(not 0 <= int(nd) <= 3 for nd in d):
            raise ValueError("boundary constraints: at most 4 per side, derivative orders 0..3")
    if kind == _lib.SPLINE_I:
        for nd, v in (constraints_dict_right or {}).items():
            if int(nd) == 0 and v != 1:
                raise ValueError("Only constraint value of 1.0 is supported for the I-spline's right value (isplines_jax.py:174-179)")
    knots = make_knots(kind, k, n_internal_knots)
    params = initial_params(kind, rng, nb, zero_border)
    tables, aux = load_tables(kind, k, n_internal_knots, n_mesh_points, cached_bases_path_root)
    dev = DeviceSpline(kind, k, n_internal_knots, n_mesh_points, zero_border, constraints_dict_left, constraints_dict_right, tables, aux)
    return params, knots, dev
