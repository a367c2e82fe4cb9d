"""wf_tables_build (M, I, B and the orthogonalised B tables) against the fp64 first-principles splines of spline_fp64, at degrees 1..8,
32 / 33 (B: 34) / 64 bases and meshes from 2 to 2000 points.  test_tables.py holds these tables to the reference's own files at k = 5
with 16 knots only; everywhere else they were compared with oracle.table, a restatement of the same recursion."""
import numpy as np
import pytest

import spline_fp64 as S
from waveflow_amd import _lib, build_tables
from waveflow_amd.splines._device import make_knots

KIND = {"M": _lib.SPLINE_M, "I": _lib.SPLINE_I, "B": _lib.SPLINE_B}
DEGREES = (1, 2, 3, 5, 6, 8)
MESHES = (2, 3, 17, 1000, 2000)
TOL = 1e-13


def n_internal(kind, k, nb):
    """nb = n + k (I), n + k - 2 (M), n + k - 1 (B)."""
    return nb - k + {"I": 0, "M": 2, "B": 1}[kind]


def widths(kind):
    return (32, 34, 64) if kind == "B" else (32, 33, 64)   # (the B orthogonalisation needs an even count; plain B is kept alike)


SHAPES = [(kind, k, nb) for kind in "IMB" for k in DEGREES for nb in widths(kind) if not (kind == "M" and k == 1)]


def row_scale(kind, k, n, nd):
    """The row maximum of each basis function's derivative nd (its sup norm, from a fine grid: a mesh of two or three points can sit
    where a derivative vanishes).  For I derivatives, the reference sums sum_m (t_{m+k+1} - t_m) M_m^{k+1} / (k + 1) = sum_m B_m^(nd)
    over m >= i, which cancels: its rounding scales with sum_m |B_m^(nd)|, and so does the tolerance."""
    x = np.linspace(0, 1, 8001)
    scale = np.abs(S.basis(kind, k, n, x)[nd]).max(1)
    if kind == "I" and nd > 0:
        b = np.abs(S.bspline_basis(make_knots(_lib.SPLINE_I, k, n), k, x)[nd])
        terms = np.cumsum(b[::-1], axis=0)[::-1].max(1)
        scale = np.maximum(scale, np.concatenate([terms, [0.0]]))
    return np.where(scale > 0, scale, 1.0)


@pytest.mark.parametrize("kind,k,nb", SHAPES)
def test_tables_match_fp64_splines(kind, k, nb):
    n = n_internal(kind, k, nb)
    assert S.n_bases(kind, k, n) == nb
    t = make_knots(KIND[kind], k, n)
    interior_knots = t[(t > 0) & (t < 1)]
    scales = [row_scale(kind, k, n, nd) for nd in range(4)]
    worst = 0.0
    for nm in MESHES:
        T = build_tables(KIND[kind], k, n, nm)
        R = S.tables(kind, k, n, nm)
        assert T.shape == R.shape == (4, nb, nm)
        x = np.linspace(0, 1, nm)
        for nd in range(4):
            err = np.abs(T[nd] - R[nd]) / scales[nd][:, None]
            if kind == "I" and nd >= k:
                # A derivative of order >= k jumps at an interior knot.  There the reference's I table sums only the terms m <= j with
                # t_j < x <= t_{j+1} (splines_np.py:79-93), each evaluated from the right: neither one-sided limit.  Those mesh points
                # are left out; everywhere else the table is held to the right limit like M and B.
                err[:, np.isin(x, interior_knots)] = 0
            worst = max(worst, float(err.max()))
            assert err.max() <= TOL, (kind, k, nb, nm, nd, err.max())
        # the two facts the fp64 side builds in: the left limit at x = 1, and I_{nb-1} = 0
        if kind == "I":
            assert np.abs(T[0][:, -1] - np.r_[np.ones(nb - 1), 0.0]).max() <= TOL
            assert not T[:, nb - 1].any()
        if kind == "B":
            assert abs(T[0][nb - 1, -1] - 1.0) <= TOL
    print(f"{kind} k={k} nb={nb}: largest |table - fp64| / row scale = {worst:.2e}")


def test_m_splines_of_degree_one_are_refused():
    with pytest.raises(_lib.WfError):
        build_tables(_lib.SPLINE_M, 1, 32, 17)


@pytest.mark.parametrize("k", DEGREES)
@pytest.mark.parametrize("nm", [1000, 2000])
def test_ortho_b_tables_at_64_bases(k, nm):
    n = n_internal("B", k, 64)
    B = build_tables(_lib.SPLINE_B, k, n, nm)
    OB, b2o, o2b = build_tables(_lib.SPLINE_OB, k, n, nm)
    assert OB.shape == (4, 64, nm) and b2o.shape == o2b.shape == (64, 64)
    gram = OB[0] @ OB[0].T
    np.testing.assert_allclose(gram, nm * np.eye(64), rtol=0, atol=1e-10 * nm)
    np.testing.assert_allclose(b2o @ o2b, np.eye(64), rtol=0, atol=1e-10)
    for nd in range(4):
        scale = (np.abs(b2o) @ np.abs(B[nd])).max(1, keepdims=True)
        err = np.abs(OB[nd] - b2o @ B[nd]) / np.where(scale > 0, scale, 1)
        assert err.max() <= 1e-12, (nd, err.max())


def test_fp64_helper_matches_scipy_at_interior_points():
    interpolate = pytest.importorskip("scipy.interpolate")
    x = np.random.default_rng(0).uniform(0, 1, 500)
    for kind, k, nb in (("B", 3, 34), ("B", 8, 64), ("M", 5, 33), ("M", 2, 64), ("I", 1, 32), ("I", 6, 64)):
        n = n_internal(kind, k, nb)
        t = make_knots(KIND[kind], k, n).astype(np.float64)
        got = S.basis(kind, k, n, x)
        deg = k - 1 if kind == "M" else k
        nbs = len(t) - deg - 1
        eye = np.eye(nbs)
        Bm = np.stack([np.stack([interpolate.BSpline(t, eye[m], deg, extrapolate=False)(x, nu=nd) if nd <= deg else np.zeros_like(x)
                                 for m in range(nbs)]) for nd in range(4)])   # [4][nbs][X]
        if kind == "I":   # I_i = sum_{m >= i} B_m: sums that cancel in the derivatives, so the scale is sum_m |B_m^(nd)|
            tail = lambda a: np.concatenate([np.cumsum(a[:, ::-1], axis=1)[:, ::-1], np.zeros((4, 1, len(x)))], axis=1)
            ref, scale = tail(Bm), tail(np.abs(Bm)).max(2)
        else:
            w = np.ones(nbs) if kind == "B" else np.array([k / (t[i + k] - t[i]) if t[i + k] > t[i] else 0.0 for i in range(nbs)])
            ref = Bm * w[None, :, None]
            scale = np.abs(ref).max(2)
        err = np.abs(got - ref) / np.maximum(scale, 1.0)[..., None]
        assert err.max() <= 1e-12, (kind, k, err.max())
