"""fp64 spline reference from first principles, for the table and closure tests (a helper module, not a conftest).

Cox-de Boor on the knot vectors of waveflow_amd.splines._device.make_knots, vectorised over the abscissae, with the conventions the
reference's cached tables use:
  - half-open knot intervals [t_l, t_{l+1}): at an interior knot, a derivative that jumps there takes its value from the right;
  - x = 1 is the limit from the left (the last non-empty interval is closed);
  - B: the degree-k B-splines B_0 .. B_{nb-1}, nb = len(t) - k - 1;
  - M: order k (degree k - 1), M_i = k B_i^{k-1} / (t_{i+k} - t_i), 0 on an empty span; nb = len(t) - k;
  - I: I_i = sum_{m >= i} B_m^k, nb = len(t) - k, so that I_{nb-1} is zero everywhere; its derivatives are those of
    k B_i^{k-1} / (t_{i+k} - t_i).
Derivatives 0..3 by the textbook rule B_{i,d}^(r) = d (B_{i,d-1}^(r-1) / (t_{i+d} - t_i) - B_{i+1,d-1}^(r-1) / (t_{i+d+1} - t_{i+1})).

Plain NumPy only."""
import numpy as np

from waveflow_amd import _lib
from waveflow_amd.splines._device import make_knots

KINDS = {"M": _lib.SPLINE_M, "I": _lib.SPLINE_I, "B": _lib.SPLINE_B}
ND = 4


def _safe_div(a, d):
    return a / d if d != 0 else np.zeros_like(a)


def bspline_basis(t, deg, x, n_deriv=ND):
    """fp64 [n_deriv][len(t) - deg - 1][len(x)]: derivatives 0..n_deriv-1 of the degree-deg B-splines on knots t."""
    t = np.asarray(t, np.float64)
    x = np.asarray(x, np.float64)
    nt = len(t)
    # the interval of each x: t_l <= x < t_{l+1}, clamped to the last non-empty interval (x = t[-1] -> limit from the left)
    last = int(np.nonzero(t[1:] > t[:-1])[0][-1])
    first = int(np.nonzero(t[1:] > t[:-1])[0][0])
    ell = np.clip(np.searchsorted(t, x, side="right") - 1, first, last)
    # B[d][r]: [nt - d - 1][X]
    B = [[None] * n_deriv for _ in range(deg + 1)]
    b0 = np.zeros((nt - 1, len(x)))
    b0[ell, np.arange(len(x))] = 1.0
    B[0][0] = b0
    for r in range(1, n_deriv):
        B[0][r] = np.zeros_like(b0)
    for d in range(1, deg + 1):
        nbd = nt - d - 1
        prev = B[d]
        for r in range(n_deriv):
            prev[r] = np.zeros((nbd, len(x)))
        lo = B[d - 1]
        for i in range(nbd):
            s1, s2 = t[i + d] - t[i], t[i + d + 1] - t[i + 1]
            prev[0][i] = _safe_div((x - t[i]) * lo[0][i], s1) + _safe_div((t[i + d + 1] - x) * lo[0][i + 1], s2)
            for r in range(1, n_deriv):
                prev[r][i] = d * (_safe_div(lo[r - 1][i], s1) - _safe_div(lo[r - 1][i + 1], s2))
    return np.stack(B[deg])


def n_bases(kind, k, n_internal_knots):
    nt = len(make_knots(KINDS[kind], k, n_internal_knots))
    return nt - k - 1 if kind == "B" else nt - k


def basis(kind, k, n_internal_knots, x, n_deriv=ND):
    """fp64 [n_deriv][nb][len(x)] of the M, I or B basis of the closures (kind "M", "I", "B")."""
    t = make_knots(KINDS[kind], k, n_internal_knots).astype(np.float64)
    nb = n_bases(kind, k, n_internal_knots)
    if kind == "B":
        return bspline_basis(t, k, x, n_deriv)
    if kind == "M":
        b = bspline_basis(t, k - 1, x, n_deriv)   # [n_deriv][nt - k][X]
        scale = np.array([_safe_div(np.float64(k), t[i + k] - t[i]) for i in range(nb)])
        return b * scale[None, :, None]
    # value: the tail sum; derivatives: d/dx sum_{m >= i} B_m^k = k B_i^{k-1} / (t_{i+k} - t_i), which has no cancellation
    b = bspline_basis(t, k, x, 1)[0]               # [nt - k - 1][X]
    val = np.concatenate([np.cumsum(b[::-1], axis=0)[::-1], np.zeros((1, len(x)))])
    if n_deriv == 1:
        return val[None]
    d = bspline_basis(t, k - 1, x, n_deriv - 1)   # [n_deriv - 1][nt - k][X]
    scale = np.array([_safe_div(np.float64(k), t[i + k] - t[i]) for i in range(nb)])
    return np.concatenate([val[None], d * scale[None, :, None]])


def tables(kind, k, n_internal_knots, n_mesh, n_deriv=ND):
    """The basis on linspace(0, 1, n_mesh): the fp64 counterpart of wf_tables_build, [n_deriv][nb][n_mesh]."""
    return basis(kind, k, n_internal_knots, np.linspace(0, 1, n_mesh), n_deriv)


def lerp_indices(x32, n_mesh):
    """The mesh indices the kernels gather (make_lerp): fp32 x * (n_mesh - 1), floor and ceil; a negative index wraps once, then every
    index is clamped (jnp gathers).  -> (xl unwrapped, il, ir)."""
    x32 = np.asarray(x32, np.float32)
    xs = x32 * np.float32(n_mesh - 1)
    xl, xr = np.floor(xs).astype(np.int64), np.ceil(xs).astype(np.int64)
    wrap = lambda i: np.clip(np.where(i < 0, i + n_mesh, i), 0, n_mesh - 1)
    return xl, wrap(xl), wrap(xr)


def lerp64(T64, x32, n_mesh):
    """X_cached in fp64 on the kernel's gather indices: T64 [..., n_mesh], x32 [X] -> [..., X].  dx = x - xl / (n_mesh - 1) with the
    unwrapped xl, slope = (T[ir] - T[il]) * (n_mesh - 1), all in fp64."""
    xl, il, ir = lerp_indices(x32, n_mesh)
    n = np.float64(n_mesh - 1)
    dx = np.asarray(x32, np.float64) - xl / n
    yl, yr = T64[..., il], T64[..., ir]
    return yl + (yr - yl) * n * dx


def normalised_ob_weights(c, o2b64):
    """fp64 normalised(c @ ob_to_b) of the B closures, c [N][nb]."""
    p = np.asarray(c, np.float64) @ o2b64
    return p / np.sqrt((p * p).sum(1, keepdims=True))
