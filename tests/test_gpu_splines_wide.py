"""The spline closures on both halves of their kernels (NBP = 32 and the 64-wide path), up to the advertised 64 bases: bit for bit against
the fp32 restatement of test_gpu_splines, and within a derived fp32 error bound of the fp64 first-principles splines of spline_fp64."""
import numpy as np
import pytest
import torch

import spline_fp64 as S
from test_gpu_splines import apply_ref, bisect_ref, coefs, enforce_ref, make, np_, remove_bias_ref
from waveflow_amd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24   # fp32 unit roundoff


def gamma(n):
    return n * U / (1 - n * U)


# (kind, k, n_internal_knots, zero_border): nb = n + k (I), n + k - 2 (M), n + k - 1 (B)
WIDE = [("I", 6, 26, False), ("I", 6, 26, True),     # 32 bases: the top of NBP = 32
        ("I", 6, 27, False), ("I", 6, 27, True),     # 33: NBP = 64; with zero_border nc = 31
        ("I", 6, 58, False), ("I", 6, 58, True),     # 64
        ("M", 6, 29, False), ("M", 6, 29, True),     # 33
        ("M", 6, 60, False), ("M", 6, 60, True),     # 64
        ("B", 6, 29, False), ("B", 6, 59, False)]    # 34, 64
LOW_DEGREE = [("I", 1, 20, False), ("B", 1, 20, False), ("I", 2, 20, True), ("M", 2, 20, False), ("M", 3, 20, True), ("B", 3, 20, False),
              ("I", 8, 20, False), ("M", 8, 20, False), ("B", 8, 21, False)]   # NBP = 32 at degrees 1, 2, 3 and 8
NS = [1, 63, 64, 65, 255, 256, 257, 4097]   # (256 rows per block)
# every shape on meshes of 2, 17 and 2000 points; B only where n_mesh >= nb: the orthogonalisation needs as many samples as bases
APPLY_CASES = [s + (nm,) for s in WIDE + LOW_DEGREE for nm in (2, 17, 2000) if s[0] != "B" or nm >= s[1] + s[2] - 1]


def nbp_of(nb):
    return 32 if nb <= 32 else 64


def probes(N, nm, seed):
    """xs_probe of test_gpu_splines, with its mesh picks clamped so that a mesh of 2 points has them too."""
    g = np.random.default_rng(seed)
    x = g.uniform(0, 1, N).astype(f32)
    mesh = (np.arange(nm, dtype=f32) / f32(nm - 1)).astype(f32)
    pick = lambda *i: mesh[np.clip(i, 0, nm - 1)]
    special = np.concatenate([[0, 1, -1e-7, -1e-4, -0.3 / (nm - 1)], pick(1, 2, nm // 2, nm - 2),
                              np.nextafter(pick(1, nm // 3, nm - 1), f32(2)), np.nextafter(pick(0, nm // 3, nm - 2), f32(-1))]).astype(f32)
    m = min(N, len(special))
    x[:m] = special[:m]
    if N > 4 * len(special):
        p = g.integers(0, nm, N // 4)
        x[len(special):len(special) + N // 4] = np.nextafter(mesh[p], np.where(g.random(N // 4) < 0.5, f32(-1), f32(2)).astype(f32))
    return x


# ---------------------------------------------------------------------------------------------------- fp64 reference and error bound
class Fp64:
    """The closure's fp64 counterpart: tables from first principles, weights per basis [N][nb]."""

    def __init__(self, kind, k, n, nm, zb, dev):
        self.kind, self.nm, self.nb = kind, nm, dev.nb
        self.nbp = nbp_of(dev.nb)
        self.base = 1 if zb else 0
        self.T64 = S.tables(kind, k, n, nm)          # [4][nb][nm]
        if kind == "B":
            OB, b2o, o2b = _ortho(k, n, nm)
            self.T64, self.plain64, self.b2o64, self.o2b64 = OB, self.T64, b2o, o2b

    def weights(self, c):
        """-> (w64, dw): fp64 weights per basis and a bound on |w32 - w64| of the kernel's fp32 weights."""
        N = len(c)
        if self.kind != "B":
            w = np.zeros((N, self.nb))
            w[:, self.base:self.base + c.shape[1]] = c
            return w, np.zeros_like(w)
        w = S.normalised_ob_weights(c, self.o2b64)
        # ob_weights: p_j = sum_i c_i o2b32_ij over nb terms (o2b rounded to fp32 once), ss = sum_j p_j^2 over NBP terms, sqrt, divide
        c64 = c.astype(np.float64)
        p = c64 @ self.o2b64
        dp = gamma(self.nb + 2) * (np.abs(c64) @ np.abs(self.o2b64))
        ss = (p * p).sum(1, keepdims=True)
        nrm = np.sqrt(ss)
        rel = 0.5 * ((2 * np.abs(p) * dp + dp * dp).sum(1, keepdims=True) / ss + gamma(self.nbp + 1)) + U
        dw = (dp / nrm + np.abs(w) * (rel + U)) * (1 + 1e-6)
        return w, dw

    def terms(self, x, nd, T=None):
        """Per-basis lerped fp64 values y_j [nb][N] and the bound e_j on how far the kernel's fp32 lerp of the fp32 table lies from them:
        the table's rounding u (|yl| + |yr|)(1 + |n dx|); slope = (yr - yl) * n and slope * dx, 3 u |yr - yl| |n dx|; dx = x - xl / n,
        u (|xl| / n + |dx|) times |slope|; the final add, u |y|."""
        T = self.T64[nd] if T is None else T
        xl, il, ir = S.lerp_indices(x, self.nm)
        n = float(self.nm - 1)
        ndx = np.abs(n * (x.astype(np.float64) - xl / n))
        yl, yr = T[:, il], T[:, ir]
        y = S.lerp64(T, x, self.nm)
        d = np.abs(yr - yl)
        e = U * ((np.abs(yl) + np.abs(yr)) * (1 + ndx) + 3 * d * ndx + d * (np.abs(xl) + ndx) + np.abs(y))
        return y, e * (1 + 1e-6)

    def value_and_bound(self, c, x, nd):
        """y64 = sum_j w_j lerp64(T64_j, x) and the bound on |y32 - y64|: the per-basis terms, the weights' error for B, and the
        kernel's NBP-term ascending sum of fp32 products, gamma(NBP + 1) sum_j |w_j| |y32_j|."""
        w, dw = self.weights(c)
        y, e = self.terms(x, nd)
        yw = np.abs(y) + e
        aw = np.abs(w).T
        bound = (aw * e).sum(0) + (dw.T * yw).sum(0) + gamma(self.nbp + 1) * ((aw + dw.T) * yw).sum(0)
        return (w.T * y).sum(0), bound * (1 + 1e-6) + 1e-37


_ORTHO = {}


def _ortho(k, n, nm):
    """fp64 OB tables of the first-principles B-splines: the library's b_to_ob (the orthogonalisation itself is held to its definition in
    test_spline_tables_fp64) applied to them."""
    from waveflow_amd import build_tables
    key = (k, n, nm)
    if key not in _ORTHO:
        _, b2o, o2b = build_tables(_lib.SPLINE_OB, k, n, nm)
        B = S.tables("B", k, n, nm)
        _ORTHO[key] = (np.einsum("ij,njm->nim", b2o, B), b2o, o2b)
    return _ORTHO[key]


def negative_controls(ref, c, x, y32, bound):
    """fp64 variants of the spline, each one real mistake; -> {name: share of probes where |y32 - variant| exceeds the bound}."""
    w, _ = ref.weights(c)
    X = S.lerp64(ref.T64[0], x, ref.nm)                  # [nb][N]
    var = {}
    shifted = np.zeros_like(w)
    shifted[:, 1:] = w[:, :-1]                            # every weight one basis up
    var["index shifted by one"] = (shifted.T * X).sum(0)
    counted = [j for j in range(ref.nb) if ref.T64[0][j].any() and (w[:, j] != 0).any()]
    if counted:   # (none for M with zero_border on a mesh of 2 points: every weighted basis is 0 at x = 0 and 1, and so is the spline)
        last = counted[-1]                                # (I_{nb-1} is zero everywhere: the last basis that counts)
        dropped = w.copy()
        dropped[:, last] = 0
        var["last real basis dropped"] = (dropped.T * X).sum(0)
        # column nb read as a basis: the weight beyond the last coefficient not zeroed, and a gather that wraps to column 0
        var["padding column read as basis nb"] = (w.T * X).sum(0) + w[:, last] * X[0]
    xl = np.floor(x * f32(ref.nm)).astype(np.int64)       # n_mesh in place of n_mesh - 1
    il, ir = np.clip(xl, 0, ref.nm - 1), np.clip(np.ceil(x * f32(ref.nm)).astype(np.int64), 0, ref.nm - 1)
    Xn = ref.T64[0][:, il] + (ref.T64[0][:, ir] - ref.T64[0][:, il]) * ref.nm * (x.astype(np.float64) - xl / ref.nm)
    var["n_mesh in the lerp"] = (w.T * Xn).sum(0)
    if ref.kind == "B":
        wt = S.normalised_ob_weights(c, ref.o2b64.T)
        var["ob_to_b transposed"] = (wt.T * X).sum(0)
        var["plain B tables"] = (w.T * S.lerp64(ref.plain64[0], x, ref.nm)).sum(0)
    truth = (w.T * X).sum(0)
    # (a variant equal to the spline on this shape is no mistake here -- e.g. M with zero_border on a mesh of 2 points is 0 throughout)
    return {k: float((np.abs(y32 - v) > bound).mean()) for k, v in var.items() if not np.array_equal(v, truth)}


# share of the probes on which each control must exceed the bound.  The local ones change y only where one end basis is non-zero: the
# last or first k + 1 of n - 1 knot intervals, where a degree-6 basis rises like x^6 (1.6 % of the probes at 64 bases, 2000 points)
CONTROL_SHARE = {"index shifted by one": 0.5, "n_mesh in the lerp": 0.5, "ob_to_b transposed": 0.5, "plain B tables": 0.5,
                 "last real basis dropped": 0.01, "padding column read as basis nb": 0.01}


def build(kind, k, n, nm, zb, root, **kw):
    out, tab, plain, o2b, b2o = make(kind, (k, n, nm), root, zb, **kw)
    return out, out[1].spline, tab, plain, o2b, b2o


# ---------------------------------------------------------------------------------------------------- apply / grad
@pytest.mark.parametrize("kind,k,n,zb,nm", APPLY_CASES)
def test_apply_and_grad_bit_exact_and_fp64_accurate(tmp_path, kind, k, n, zb, nm):
    out, dev, tab, _, o2b, _ = build(kind, k, n, nm, zb, tmp_path)
    assert dev.nb == S.n_bases(kind, k, n)
    base = 1 if zb else 0
    ref = Fp64(kind, k, n, nm, zb, dev)
    worst = 0.0
    for N in NS:
        c = coefs(kind, N, dev.nc, N + nm)
        x = probes(N, nm, N + 1)
        for nd in (0, 1, 2):
            y, dy = dev.apply(c, x, nd=nd, grad=True)
            y, dy = np_(y), np_(dy)
            assert np.array_equal(y, apply_ref(kind, tab, c, x, nd, base, o2b)), (N, nd, "value")
            assert np.array_equal(dy, apply_ref(kind, tab, c, x, nd + 1, base, o2b)), (N, nd, "derivative")
            for got, order in ((y, nd), (dy, nd + 1)):
                y64, bound = ref.value_and_bound(c, x, order)
                ratio = np.abs(got - y64) / bound
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1).all(), (N, order, float(ratio.max()), int(ratio.argmax()))
                if N == 4097 and order == 0:
                    shares = negative_controls(ref, c, x, got, bound)
                    assert "index shifted by one" in shares
                    for name, share in shares.items():
                        assert share >= CONTROL_SHARE[name], (name, share)
        y3 = np_(dev.apply(c, x, nd=3))
        assert np.array_equal(y3, apply_ref(kind, tab, c, x, 3, base, o2b)), (N, 3)
        y64, bound = ref.value_and_bound(c, x, 3)
        assert (np.abs(y3 - y64) <= bound).all(), (N, 3)
        worst = max(worst, float((np.abs(y3 - y64) / bound).max()))
    print(f"{kind} k={k} n={n} zb={zb} n_mesh={nm}: largest |y32 - y64| / bound = {worst:.3f}")


def test_nc64_unaligned_view(tmp_path):
    """nc = 64 through a view that is 4-byte aligned only: the scalar staging fallback, with a partial last wave."""
    for kind, n in (("I", 58), ("M", 60)):
        out, dev, tab, _, _, _ = build(kind, 6, n, 1000, False, tmp_path / kind)
        assert dev.nc == 64
        N = 301
        c = coefs(kind, N, 64, 2)
        big = torch.from_numpy(np.concatenate([np.zeros(1, f32), c.ravel()])).cuda()
        view = big[1:].view(N, 64)
        assert view.data_ptr() % 16 != 0
        x = probes(N, 1000, 3)
        y, dy = dev.apply(view, x, nd=0, grad=True)
        assert np.array_equal(np_(y), apply_ref(kind, tab, c, x, 0))
        assert np.array_equal(np_(dy), apply_ref(kind, tab, c, x, 1))


@pytest.mark.parametrize("kind,n", [("I", 58), ("B", 59)])
def test_apply_large_batch_64_bases(tmp_path, kind, n):
    N, chunk = 1 << 20, 1 << 16
    out, dev, tab, _, o2b, _ = build(kind, 6, n, 1000, False, tmp_path)
    assert dev.nb == 64
    c, x = coefs(kind, N, dev.nc, 5), probes(N, 1000, 6)
    ct, xt = torch.from_numpy(c).cuda(), torch.from_numpy(x).cuda()
    y, dy = dev.apply(ct, xt, nd=0, grad=True)
    y, dy = np_(y), np_(dy)
    for s in range(0, N, chunk):   # (a 64 x 2^20 restatement at once is a lot of host memory)
        sl = slice(s, s + chunk)
        assert np.array_equal(y[sl], apply_ref(kind, tab, c[sl], x[sl], 0, 0, o2b)), s
        assert np.array_equal(dy[sl], apply_ref(kind, tab, c[sl], x[sl], 1, 0, o2b)), s


# ---------------------------------------------------------------------------------------------------- reverse
@pytest.mark.parametrize("tol", [1e-3, 1e-6])
@pytest.mark.parametrize("zb", [False, True])
def test_reverse_64_bases(tmp_path, tol, zb):
    out, dev, tab, _, _, _ = build("I", 6, 58, 1000, zb, tmp_path, reverse_fun_tol=tol)
    assert dev.nb == 64
    N = 5000
    c = coefs("I", N, dev.nc, 9)
    x_true = np.random.default_rng(10).uniform(0, 1, N).astype(f32)
    y = np_(out[1](c, x_true))
    xr = np_(out[3](c, y))
    assert np.array_equal(xr, bisect_ref("I", tab, c, y, tol, 1 if zb else 0))
    dy = np_(out[2](c, x_true))
    ok = dy > 1e-3
    assert ok.mean() > 0.5
    slack = 2e-6 / np.maximum(dy, 1e-3)
    assert (np.abs(xr - x_true.astype(np.float64))[ok] <= tol + slack[ok]).all()


# ---------------------------------------------------------------------------------------------------- boundary conditions, remove_bias
FOUR_ZERO = {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0}
FOUR_VALUES = {0: 0.1, 1: -0.2, 2: 0.3, 3: -0.4}
BC_CASES = [("I", 58, False), ("I", 58, True), ("M", 60, False), ("M", 60, True), ("B", 59, False)]


@pytest.mark.parametrize("left,right", [(FOUR_ZERO, FOUR_ZERO), (FOUR_VALUES, FOUR_VALUES), ({0: 0.0, 2: 0.0}, {1: 0.0, 3: 0.0})])
@pytest.mark.parametrize("kind,n,zb", BC_CASES)
def test_enforce_bc_and_remove_bias_64_bases(tmp_path, kind, n, zb, left, right):
    if kind == "I":   # the I-spline's right value constraint is 1 (any other value is refused)
        right = {**right, 0: 1.0}
    out, dev, _, plain, _, _ = build(kind, 6, n, 1000, zb, tmp_path, constraints_dict_left=left, constraints_dict_right=right)
    assert dev.nb == 64
    enforce = out[5]
    w = coefs(kind, 777, dev.nc, 4) + (0 if kind == "B" else f32(0.05))
    got = np_(enforce(w))
    assert np.array_equal(got, enforce_ref(kind, plain, w, left, right), equal_nan=True)
    homogeneous = all(v == 0 for v in left.values()) and all(v == 0 or (kind == "I" and nd == 0) for nd, v in right.items())
    if homogeneous and not zb:
        # The enforced weights satisfy the constraints in fp64: sum_j w_j E_j^(nd) at x = 0 / 1, E the plain tables from first
        # principles.  Solving for w_nd costs nd products and sums, a subtraction, a division and the normalisation's division:
        # |residual| <= (nd + 6) u sum_j |E_j w_j|; the I-spline's right value 1 also carries the normalising sum over nw terms.
        # (Under zero_border the reference indexes the constraint rows with nw = len(weights), not shifted by the border: the
        # enforced weights do not satisfy the constraints there, by design, so nothing is checked.)
        E = S.tables(kind, 6, n, 1000)   # (for B the plain tables, which enforce_boundary_conditions reads)
        nw = got.shape[1]
        g64 = got.astype(np.float64)
        for side, d in ((0, left), (-1, right)):
            for nd, v in d.items():
                e = E[nd][:nw, side]
                res = g64 @ e - v
                scale = np.abs(g64) @ np.abs(e)
                ops = nw + 6 if (kind == "I" and side == -1 and nd == 0) else nd + 6
                assert (np.abs(res) <= ops * U * scale).all(), (side, nd, float(np.abs(res).max()))
    if kind != "B":
        rb = out[6]
        for nw in (dev.nc, 6 + 2 if kind == "I" else 6):   # full width and the narrowest row the reference's indices fit in
            p = w[:, :nw].copy()
            assert np.array_equal(np_(rb(torch.from_numpy(p).cuda())), remove_bias_ref(kind, 6, p)), nw


# ---------------------------------------------------------------------------------------------------- samplers
def density_cdf64(kind, ref, c, n_knots, cells=1 << 20):
    """CDF on a fine grid of the density the sampler draws from, min(f^2, ymax) (B) / min(f, ymax) (M), with f the fp64 spline on the
    fp64 tables (lerp is linear in the table, so f = lerp64(sum_j w_j T_j)) and ymax as the reference bounds it; integrated in fp64."""
    w, _ = ref.weights(c[None])
    F = w[0] @ ref.T64[0]
    grid = (np.arange(cells + 1) / cells).astype(f32)
    f = S.lerp64(F, grid, ref.nm)
    if kind == "B":
        ymax = float(((w[0] @ ref.b2o64) ** 2).max())
        dens = np.minimum(f ** 2, ymax)
    else:
        dens = np.minimum(np.maximum(f, 0), float(c.max()) * n_knots)
    g64 = grid.astype(np.float64)
    cdf = np.concatenate([[0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(g64))])
    return g64, cdf / cdf[-1]


@pytest.mark.parametrize("kind,n", [("M", 60), ("B", 59)])
def test_sampler_64_bases(tmp_path, kind, n):
    out, dev, *_ = build(kind, 6, n, 1000, False, tmp_path)
    assert dev.nb == 64
    ref = Fp64(kind, 6, n, 1000, False, dev)
    sample = out[3]
    c = np_(out[5](coefs(kind, 2, dev.nc, 12)))
    ns = 1 << 16
    x = sample(5, c, ns)
    xa = np_(x)
    assert (xa >= 0).all() and (xa < 1).all()
    # draws keyed by (seed, row, slot): a shorter call is a prefix of a longer one
    assert np.array_equal(np_(sample(5, c, 1000)), xa[:, :1000])
    # one-sample KS at 0.1 % (sqrt(n) D < 1.949): the draws are fixed by the seed, each row's pass is a fixed outcome
    crit = 1.949 / np.sqrt(ns)
    for r in range(len(c)):
        grid, cdf = density_cdf64(kind, ref, c[r], len(out[4]))
        s = np.sort(xa[r].astype(np.float64))
        F = np.interp(s, grid, cdf)
        i = np.arange(1, ns + 1)
        ks = max((i / ns - F).max(), (F - (i - 1) / ns).max())
        assert ks < crit, (r, ks * np.sqrt(ns))


# ---------------------------------------------------------------------------------------------------- error paths
def raises_status(status, fn, *a, **kw):
    with pytest.raises(_lib.WfError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def test_error_paths(tmp_path):
    INVALID, UNSUPPORTED = -1, _lib.ERR_UNSUPPORTED
    outs = {kind: build(kind, 6, n, 1000, False, tmp_path / kind, constraints_dict_left={0: 0.0, 3: 0.0})
            for kind, n in (("I", 58), ("M", 60), ("B", 59))}
    for kind, (out, dev, *_rest) in outs.items():
        c, x = coefs(kind, 8, dev.nc, 1), probes(8, 1000, 2)
        raises_status(INVALID, dev.apply, c, x, nd=3, grad=True)
        raises_status(INVALID, dev.apply, c, x, nd=4)
        w = coefs(kind, 8, 64, 1)
        raises_status(INVALID, dev.rowwise, "wf_spline_enforce_bc", np.zeros((8, 65), f32))   # nw > nb
        raises_status(INVALID, dev.rowwise, "wf_spline_enforce_bc", w[:, :3])                 # left order 3 >= nw
        assert np_(dev.rowwise("wf_spline_enforce_bc", w[:, :4])).shape == (8, 4)
        if kind in "MB":
            raises_status(UNSUPPORTED, dev.reverse, c, x, 1e-3)
        else:
            raises_status(UNSUPPORTED, dev.sample, 0, c, 4, 10)
    raises_status(UNSUPPORTED, outs["B"][1].rowwise, "wf_spline_remove_bias", coefs("B", 8, 64, 1))
    raises_status(INVALID, outs["I"][1].rowwise, "wf_spline_remove_bias", coefs("I", 8, 7, 1))   # narrower than k + 2
    raises_status(INVALID, outs["M"][1].rowwise, "wf_spline_remove_bias", coefs("M", 8, 5, 1))   # narrower than k
