"""waveflow_amd.splines on the host: knots, initial parameters, the table cache, refused options (no GPU needed)."""
import os

import numpy as np
import pytest

from waveflow_amd import _lib
from waveflow_amd.splines import BSpline_fun, ISpline_fun, MSpline_fun
from waveflow_amd.utils import table_cache


def _ref_knots(kind, k, n):
    """The reference's lines (isplines_jax.py:90-92, msplines_jax.py:73-75, bsplines_jax.py:58-60)."""
    internal_knots = np.linspace(0, 1, n)
    if kind == "I":
        internal_knots = np.repeat(internal_knots, ((internal_knots == internal_knots[0]) * (k + 1)).clip(min=1))
        return np.repeat(internal_knots, ((internal_knots == internal_knots[-1]) * (k + 1)).clip(min=1))
    if kind == "M":
        internal_knots = np.repeat(internal_knots, ((internal_knots == internal_knots[0]) * k).clip(min=1))
        return np.repeat(internal_knots, ((internal_knots == internal_knots[-1]) * k).clip(min=1))
    internal_knots = np.repeat(internal_knots, ((internal_knots == internal_knots[0]) * k + 1).clip(min=1))
    return np.repeat(internal_knots, ((internal_knots == internal_knots[-1]) * k + 1).clip(min=1))


FUNS = {"I": ISpline_fun, "M": MSpline_fun, "B": BSpline_fun}


@pytest.mark.parametrize("kind", ["I", "M", "B"])
@pytest.mark.parametrize("k,n", [(2, 5), (5, 16), (6, 23), (3, 8)])   # (B: an even basis count, ortho_splines.py:58-63)
def test_knots_match_reference(tmp_path, kind, k, n):
    out = FUNS[kind]()(0, k, n, cached_bases_path_root=str(tmp_path), n_mesh_points=50)
    knots = out[4]
    assert np.array_equal(np.asarray(knots), _ref_knots(kind, k, n))
    assert len(out) == (6 if kind == "B" else 7)


@pytest.mark.parametrize("kind", ["I", "M", "B"])
@pytest.mark.parametrize("zero_border", [False, True])
def test_initial_params_shape_and_normalisation(tmp_path, kind, zero_border):
    k, n = 5, 16
    kw = {} if kind == "B" else {"zero_border": zero_border}
    p = FUNS[kind]()(np.random.default_rng(3), k, n, cached_bases_path_root=str(tmp_path), n_mesh_points=50, **kw)[0]
    knots = _ref_knots(kind, k, n)
    if kind == "B":
        assert p.shape == (len(knots) - k - 1,)
        assert abs(float(np.sum(p.astype(np.float64) ** 2)) - 1) < 1e-6
    else:
        nb = len(knots) - k
        assert p.shape == ((nb - 2) if zero_border else nb,)
        assert (p >= 0).all() and abs(float(p.sum()) - 1) < 1e-6


def test_rng_forms_accepted(tmp_path):
    f = ISpline_fun()
    a = f(7, 5, 16, cached_bases_path_root=str(tmp_path), n_mesh_points=50)[0]
    b = f(np.random.default_rng(7), 5, 16, cached_bases_path_root=str(tmp_path), n_mesh_points=50)[0]
    c = f(None, 5, 16, cached_bases_path_root=str(tmp_path), n_mesh_points=50)[0]
    assert np.array_equal(a, b) and a.shape == c.shape


@pytest.mark.parametrize("kind", ["I", "M", "B"])
def test_empty_cache_root_gets_reference_names(tmp_path, kind):
    root = str(tmp_path / kind)
    FUNS[kind]()(0, 5, 16, cached_bases_path_root=root, n_mesh_points=60)
    names = table_cache.cache_file_names(kind, 5, 16, 60)
    expect = set(names["nd"]) | (set(names["ob"]) | {names["b_to_ob"], names["ob_to_b"]} if kind == "B" else set())
    assert set(os.listdir(root)) == expect


@pytest.mark.parametrize("kind", ["I", "M", "B"])
def test_seeded_cache_is_loaded(tmp_path, kind):
    """Files under the reference's names are what the closures get, not a rebuild."""
    root = str(tmp_path)
    names = table_cache.cache_file_names(kind, 5, 16, 60)
    table_cache.write_cached_bases(root, kind, 5, 16, 60)
    marked = os.path.join(root, (names["ob"] if kind == "B" else names["nd"])[0])
    t = np.load(marked)
    t[3, 7] = 12345.0
    np.save(marked, t)
    dev = FUNS[kind]()(0, 5, 16, cached_bases_path_root=root, n_mesh_points=60)[1].spline
    assert dev.tables[0, 3, 7] == 12345.0
    if kind == "B":
        plain = dev.aux[:4 * dev.nb * 60].reshape(4, dev.nb, 60)
        assert np.array_equal(plain, table_cache.load_cached_bases(root, "B", 5, 16, 60)[0])


def test_refused_options(tmp_path):
    r = str(tmp_path)
    for fun in (ISpline_fun, MSpline_fun, BSpline_fun):
        with pytest.raises(NotImplementedError):
            fun()(0, 5, 16, cardinal_splines=False, cached_bases_path_root=r)
        with pytest.raises(NotImplementedError):
            fun()(0, 5, 16, use_cached_bases=False, cached_bases_path_root=r)
    with pytest.raises(ValueError):
        ISpline_fun()(0, 5, 16, constraints_dict_right={0: 0.5}, cached_bases_path_root=r)
    # more than 64 bases: refused (the library's limit, as elsewhere)
    for fun in (ISpline_fun, MSpline_fun, BSpline_fun):
        with pytest.raises(_lib.WfError) as e:
            fun()(0, 5, 70, cached_bases_path_root=r, n_mesh_points=50)
        assert e.value.status == _lib.ERR_UNSUPPORTED


def test_create_refuses_bad_descriptors():
    import ctypes
    L = _lib.lib()
    h = ctypes.c_void_p()
    d = _lib.SplineDesc(_lib.SPLINE_I, 5, 16, 100, 0, _lib.BC.from_dict({0: 0.0}), _lib.BC.from_dict({0: 0.5}))
    assert L.wf_spline_create(ctypes.byref(d), None, None, 0, ctypes.byref(h)) == -1
    d = _lib.SplineDesc(_lib.SPLINE_I, 5, 70, 100, 0, _lib.BC.from_dict({}), _lib.BC.from_dict({}))
    assert L.wf_spline_create(ctypes.byref(d), None, None, 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    d = _lib.SplineDesc(_lib.SPLINE_B, 5, 16, 100, 1, _lib.BC.from_dict({}), _lib.BC.from_dict({}))
    assert L.wf_spline_create(ctypes.byref(d), None, None, 0, ctypes.byref(h)) == -1
    assert L.wf_spline_n_bases(None) == -1


def test_no_device_first_call_is_loud(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = MSpline_fun()(0, 5, 16, cached_bases_path_root=str(tmp_path), n_mesh_points=50)
    with pytest.raises(_lib.WfError) as e:
        out[1](out[0][None], np.array([0.5], np.float32))
    assert e.value.status == _lib.ERR_NO_DEVICE
