"""waveflow_amd.splines on the GPU against a NumPy fp32 restatement of the reference's closures in the operation order of
include/waveflow_hip.h (wf_spline_*): lerp, ascending sums, no fused multiply-add."""
import os

import numpy as np
import pytest
import torch

from waveflow_amd.splines import BSpline_fun, ISpline_fun, MSpline_fun
from waveflow_amd.utils import table_cache
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---------------------------------------------------------------------------------------------------- fp32 restatement
def lerp(T, x):
    """X_cached (isplines_jax.py:45-56) of every basis: T [nb][n_mesh] fp32, x [N] fp32 -> [nb][N]."""
    nm = T.shape[1]
    n = f32(nm - 1)
    xs = x * n
    xl, xr = np.floor(xs).astype(np.int64), np.ceil(xs).astype(np.int64)
    wrap = lambda i: np.clip(np.where(i < 0, i + nm, i), 0, nm - 1)
    yl, yr = T[:, wrap(xl)], T[:, wrap(xr)]
    dx = x - xl.astype(f32) / n
    slope = (yr - yl) * n
    return yl + slope * dx


def dot(c, X, base=0):
    acc = np.zeros(c.shape[0], f32)
    for i in range(c.shape[1]):
        acc = acc + c[:, i] * X[base + i]
    return acc


def ob_weights(c, o2b):
    p = np.zeros(c.shape, f32)
    for i in range(c.shape[1]):
        p = p + c[:, i:i + 1] * o2b[i][None, :]
    ss = np.zeros(c.shape[0], f32)
    for j in range(c.shape[1]):
        ss = ss + p[:, j] * p[:, j]
    return p / np.sqrt(ss)[:, None]


def apply_ref(kind, tab, c, x, nd, base=0, o2b=None):
    if kind == "B":
        c, base = ob_weights(c, o2b), 0
    return dot(c, lerp(tab[nd], x), base)


def bisect_ref(kind, tab, c, y, tol, base):
    low, high = np.zeros(len(y), f32), np.ones(len(y), f32)
    h = f32(tol) / f32(2)
    for _ in range(200):
        mid = f32(0.5) * (low + high)
        go = (low + h < mid) & (mid < high - h)
        if not go.any():
            break
        f = dot(c, lerp(tab[0], mid), base) - y
        up = f > 0
        high = np.where(go & up, mid, high)
        low = np.where(go & ~up, mid, low)
    return low


def enforce_ref(kind, plain, w, left, right):
    w = w.copy()
    nw = w.shape[1]
    E = lambda nd, m, j: plain[nd][j][m]
    for nd, v in left.items():
        s = np.zeros(len(w), f32)
        for j in range(nd):
            s = s + E(nd, 0, j) * w[:, j]
        w[:, nd] = (f32(v) - s) / E(nd, 0, nd)
    for nd, v in right.items():
        if kind == "I" and nd == 0:
            w[:, nw - 1] = 0
            continue
        s = np.zeros(len(w), f32)
        for j in range(nd):
            s = s + E(nd, -1, nw - 1 - j) * w[:, nw - 1 - j]
        w[:, nw - 1 - nd] = (f32(v) - s) / E(nd, -1, nw - 1 - nd)
    ss = np.zeros(len(w), f32)
    for j in range(nw):
        ss = ss + (w[:, j] * w[:, j] if kind == "B" else w[:, j])
    return w / (np.sqrt(ss) if kind == "B" else ss)[:, None]


def remove_bias_ref(kind, k, p):
    p = p.copy()
    nw = p.shape[1]
    for i in range(k):
        a, b = (i + 1, nw - i - 2) if kind == "I" else (i, nw - i - 1)
        p[:, a] = p[:, a] * f32(i + 1) / f32(k)
        p[:, b] = p[:, b] * f32(i + 1) / f32(k)
    ss = np.zeros(len(p), f32)
    for j in range(nw):
        ss = ss + p[:, j]
    return p / ss[:, None]


def np_(t):
    assert t.is_cuda and t.dtype == torch.float32
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- fixtures
FUNS = {"I": ISpline_fun, "M": MSpline_fun, "B": BSpline_fun}


@pytest.fixture(scope="module")
def fixture_root(tmp_path_factory):
    """The reference's own tables (k = 5, 16 knots, n_mesh 2000) under the reference's cache names."""
    g = np.load(os.path.join(GOLDEN, "ref_tables_k5_n16.npz"))
    root = tmp_path_factory.mktemp("refcache")
    B = np.stack([g[f"B_nd{nd}"] for nd in range(4)])
    OB = np.einsum("ij,njm->nim", g["b_to_ob"], B)
    cols = g["OB_cols"]
    for nd in range(4):
        sub = OB[nd][:, cols]
        assert np.allclose(sub, g[f"OB_nd{nd}_sub"], rtol=1e-6, atol=1e-6 * np.abs(g[f"OB_nd{nd}_sub"]).max())
    for kind in ("I", "B"):
        names = table_cache.cache_file_names(kind, 5, 16, 2000)
        d = root / kind
        d.mkdir()
        for nd in range(4):
            np.save(d / names["nd"][nd], g[f"{kind}_nd{nd}"])
            if kind == "B":
                np.save(d / names["ob"][nd], OB[nd])
        if kind == "B":
            np.save(d / names["b_to_ob"], g["b_to_ob"])
            np.save(d / names["ob_to_b"], g["ob_to_b"])
    return root


def make(kind, case, root, zero_border=False, **kw):
    """-> closures, fp32 tables (evaluated, plain), fp32 ob_to_b / b_to_ob"""
    if case == "fixture":
        k, n, nm, r = 5, 16, 2000, str(root / kind)
    else:
        k, n, nm, r = case + (str(root / f"{kind}_{case}"),)
    zb = {} if kind == "B" else {"zero_border": zero_border}
    out = FUNS[kind]()(0, k, n, cached_bases_path_root=r, n_mesh_points=nm, **zb, **kw)
    dev = out[1].spline
    tab = dev.tables.astype(f32)
    if kind == "B":
        nb = dev.nb
        plain = dev.aux[:4 * nb * nm].reshape(4, nb, nm).astype(f32)
        b2o = dev.aux[4 * nb * nm:4 * nb * nm + nb * nb].reshape(nb, nb).astype(f32)
        o2b = dev.aux[4 * nb * nm + nb * nb:].reshape(nb, nb).astype(f32)
        return out, tab, plain, o2b, b2o
    return out, tab, tab, None, None


def xs_probe(N, nm, seed):
    g = np.random.default_rng(seed)
    x = g.uniform(0, 1, N).astype(f32)
    mesh = (np.arange(nm, dtype=f32) / f32(nm - 1)).astype(f32)
    special = np.concatenate([[0, 1, -1e-7, -1e-4, -0.3 / (nm - 1)], mesh[[1, 2, nm // 2, nm - 2]],
                              np.nextafter(mesh[[1, nm // 3, nm - 1]], f32(2)), np.nextafter(mesh[[0, nm // 3, nm - 2]], f32(-1))]).astype(f32)
    m = min(N, len(special))
    x[:m] = special[:m]
    if N > 4 * len(special):   # exact mesh points and their neighbours throughout the batch
        pick = g.integers(0, nm, N // 4)
        x[len(special):len(special) + N // 4] = np.nextafter(mesh[pick], np.where(g.random(N // 4) < 0.5, f32(-1), f32(2)).astype(f32))
    return x


def coefs(kind, N, nc, seed):
    g = np.random.default_rng(seed)
    c = g.uniform(-1, 1, (N, nc)) if kind == "B" else g.uniform(0, 1, (N, nc))
    return (c / np.abs(c).sum(1, keepdims=True)).astype(f32)


# ---------------------------------------------------------------------------------------------------- apply / grad
CASES = [("I", "fixture", False), ("I", "fixture", True), ("B", "fixture", False), ("M", (5, 16, 1000), False), ("M", (5, 16, 1000), True),
         ("I", (6, 23, 1000), False), ("I", (6, 23, 1000), True), ("B", (6, 23, 1000), False), ("M", (6, 23, 1000), True)]


@pytest.mark.parametrize("kind,case,zb", CASES)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_apply_and_grad_bit_exact(fixture_root, tmp_path, kind, case, zb, N):
    out, tab, plain, o2b, _ = make(kind, case, fixture_root if case == "fixture" else tmp_path, zb)
    dev = out[1].spline
    c = coefs(kind, N, dev.nc, N)
    x = xs_probe(N, tab.shape[2], N + 1)
    base = 1 if zb else 0
    for nd in (0, 1, 2):
        y, dy = dev.apply(c, x, nd=nd, grad=True)
        assert np.array_equal(np_(y), apply_ref(kind, tab, c, x, nd, base, o2b)), (nd, "value")
        assert np.array_equal(np_(dy), apply_ref(kind, tab, c, x, nd + 1, base, o2b)), (nd, "derivative")
    assert np.array_equal(np_(out[1](c, x)), apply_ref(kind, tab, c, x, 0, base, o2b))
    assert np.array_equal(np_(out[2](torch.from_numpy(c).cuda(), torch.from_numpy(x).cuda())), apply_ref(kind, tab, c, x, 1, base, o2b))


@pytest.mark.parametrize("kind", ["I", "B"])
def test_apply_large_batch_bit_exact(tmp_path, kind):
    N = 1 << 22
    out, tab, _, o2b, _ = make(kind, (6, 23, 1000), tmp_path)
    dev = out[1].spline
    c, x = coefs(kind, N, dev.nc, 5), xs_probe(N, 1000, 6)
    ct, xt = torch.from_numpy(c).cuda(), torch.from_numpy(x).cuda()
    assert np.array_equal(np_(out[1](ct, xt)), apply_ref(kind, tab, c, x, 0, 0, o2b))
    assert np.array_equal(np_(out[2](ct, xt)), apply_ref(kind, tab, c, x, 1, 0, o2b))


def test_unaligned_rows_and_empty_batch(tmp_path):
    out, tab, _, _, _ = make("I", (6, 23, 1000), tmp_path)
    c = coefs("I", 301, 29, 2)
    big = torch.from_numpy(np.concatenate([np.zeros(1, f32), c.ravel()])).cuda()
    view = big[1:].view(301, 29)   # 4-byte aligned only: the staging falls back to 4-byte loads
    x = xs_probe(301, 1000, 3)
    assert np.array_equal(np_(out[1].spline.apply(view, x)), apply_ref("I", tab, c, x, 0))
    assert out[1](np.zeros((0, 29), f32), np.zeros(0, f32)).shape == (0,)


# ---------------------------------------------------------------------------------------------------- reverse
@pytest.mark.parametrize("tol", [1 / 1000, 1e-6])
@pytest.mark.parametrize("zb", [False, True])
def test_reverse_bit_exact_and_accurate(tmp_path, tol, zb):
    out, tab, _, _, _ = make("I", (6, 23, 1000), tmp_path, zb, reverse_fun_tol=tol)
    dev = out[1].spline
    N = 5000
    c = coefs("I", N, dev.nc, 9)            # non-negative weights: a monotone I-spline
    x_true = np.random.default_rng(10).uniform(0, 1, N).astype(f32)
    y = np_(out[1](c, x_true))
    xr = np_(out[3](c, y))
    assert np.array_equal(xr, bisect_ref("I", tab, c, y, tol, 1 if zb else 0))
    # where the spline rises by at least 1e-3 per unit (flat pieces have no unique inverse)
    dy = np_(out[2](c, x_true))
    ok = dy > 1e-3
    assert ok.mean() > 0.5
    slack = 2e-6 / np.maximum(dy, 1e-3)   # y itself carries fp32 rounding
    assert (np.abs(xr - x_true)[ok] <= tol + slack[ok]).all(), np.abs(xr - x_true)[ok].max()


# ---------------------------------------------------------------------------------------------------- boundary conditions, remove_bias
DICTS = [({0: 0}, {}), ({0: 0, 1: 0}, {0: 0}), ({0: 0, 2: 0, 3: 0}, {0: 0, 2: 0, 3: 0}), ({1: 0.3}, {1: 0.3}), ({0: 0.0}, {0: 1.0})]


@pytest.mark.parametrize("kind,zb", [("I", False), ("I", True), ("M", False), ("M", True), ("B", False)])   # (B-splines have no zero_border)
@pytest.mark.parametrize("left,right", DICTS)
def test_enforce_bc_and_remove_bias_bit_exact(fixture_root, tmp_path, kind, left, right, zb):
    if kind == "I" and right.get(0, 1) != 1:
        right = {**right, 0: 1.0}
    if kind != "I" and right.get(0) == 1.0:
        right = {0: 0.5}
    case = "fixture" if kind != "M" else (5, 16, 1000)
    root = fixture_root if kind != "M" else tmp_path
    out, _, plain, _, _ = make(kind, case, root, zb, constraints_dict_left=left, constraints_dict_right=right)
    dev = out[1].spline
    enforce = out[5]
    w = coefs(kind, 777, dev.nc, 4) + (0 if kind == "B" else f32(0.05))
    got = np_(enforce(w))
    # (equal_nan: some dictionaries divide by a basis that vanishes at the end -- zero_border rows are indexed with nw -- as the reference does)
    assert np.array_equal(got, enforce_ref(kind, plain, w, left, right), equal_nan=True)
    if kind != "B":
        rb = out[6]
        assert np.array_equal(np_(rb(torch.from_numpy(w).cuda())), remove_bias_ref(kind, 5, w))


# ---------------------------------------------------------------------------------------------------- the IMADE composition
def test_imade_composition_matches_oracle(tmp_path, he_flat):
    """made.py:66-81 through the new closures on layer 0 of the He checkpoint vs the oracle's IMADE layer."""
    import oracle
    from oracle import energy_torch as et
    from test_gpu_parity import as_accurate_as_fp32_reference, close
    om = oracle.he_model(10.0)
    tm = et.he_model(torch.float32)
    init = ISpline_fun()
    _, apply_v, apply_g, _, _, enforce, remove_bias = init(0, 6, 23, zero_border=False, n_mesh_points=2000, cached_bases_path_root=str(tmp_path),
                                                           constraints_dict_left={0: 0.0}, constraints_dict_right={0: 1.0})
    g = np.random.default_rng(7)
    u = g.uniform(0, 1, size=(4096, 2)).astype(f32)
    u[:6] = [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [1.0 / 1999, 1998.0 / 1999], [1e-7, 1 - 1e-7], [0.25, 0.75]]
    lp_ = he_flat[:om.layer_param_count()]
    net, _ = tm._net(torch.from_numpy(np.asarray(lp_, f32)), 0, 29)
    bij = tm._conditioner(net, torch.from_numpy(u), 29, True).detach().numpy().astype(f32) + f32(0.05)
    bij = bij.reshape(-1, 29)
    bij = enforce(remove_bias(bij))
    y = np_(apply_v(bij, u.reshape(-1))).reshape(-1, 2)
    ld = np_(torch.log(apply_g(bij, u.reshape(-1)) + 1e-7)).reshape(-1, 2).sum(-1)
    yo, ldo, _ = om.imade_direct(lp_, u)
    _, ldt, _ = om.imade_direct(lp_, u, f64=True)
    close(y, yo, rtol=0, atol=2e-6)
    as_accurate_as_fp32_reference(ld, ldo, ldt)


# ---------------------------------------------------------------------------------------------------- samplers
def density_cdf(kind, tab, c, o2b, b2o, n_knots):
    """CDF on a fine grid (2^20 intervals) of the density the sampler draws from: min(f^2, ymax) (B) / min(f, ymax) (M), with f the lerped
    spline evaluated by the fp32 restatement (the bits the kernel evaluates) and ymax in the kernel's order; integrated in fp64."""
    grid = (np.arange((1 << 20) + 1) / (1 << 20)).astype(f32)
    cr = np.repeat(c[None], len(grid), 0)
    f = apply_ref(kind, tab, cr, grid, 0, 0, o2b).astype(np.float64)
    if kind == "B":
        p = ob_weights(c[None], o2b)[0]
        q = np.zeros(len(p), f32)
        for i in range(len(p)):
            q = q + p[i] * b2o[i]
        ymax = float((q * q).max())
    else:
        ymax = float(c.max() * f32(n_knots))
    dens = np.minimum(f ** 2 if kind == "B" else np.maximum(f, 0), ymax)
    g64 = grid.astype(np.float64)
    cdf = np.concatenate([[0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(g64))])
    return g64, cdf / cdf[-1]


@pytest.mark.parametrize("kind", ["M", "B"])
def test_sampler_distribution_and_reproducibility(tmp_path, kind):
    out, tab, plain, o2b, b2o = make(kind, (5, 16, 1000), tmp_path)
    dev = out[1].spline
    sample = out[3]
    c = np_(out[5](coefs(kind, 4, dev.nc, 12)))   # {0: 0} at both ends (the defaults)
    ns = 1 << 16
    x = sample(5, c, ns)
    assert tuple(x.shape) == (4, ns)
    xa = np_(x)
    assert (xa >= 0).all() and (xa < 1).all()
    assert torch.equal(sample(5, c, ns), x)
    assert not np.array_equal(np_(sample(4, c, ns)), xa)
    # one-sample KS, 1 %.  The draws are fixed by the seed, so each row's pass is a fixed outcome with a 1 % chance of failing a correct
    # sampler (seed 3 puts row 1 of the B case at sqrt(n) D = 1.70; 2^20 draws of the same row with seed 6 give 1.06: no systematic drift)
    crit = 1.628 / np.sqrt(ns)
    for r in range(4):
        grid, cdf = density_cdf(kind, tab, c[r], o2b, b2o, len(out[4]))
        s = np.sort(xa[r].astype(np.float64))
        F = np.interp(s, grid, cdf)
        i = np.arange(1, ns + 1)
        ks = max((i / ns - F).max(), (F - (i - 1) / ns).max())
        assert ks < crit, (r, ks, crit)


def test_sampler_exhaustion_raises(tmp_path):
    out, tab, _, _, _ = make("M", (5, 16, 1000), tmp_path)
    dev = out[1].spline
    c = np.full((2, dev.nc), 0.1 / (dev.nc - 1), f32)
    c[:, 0] = 0.9            # one large coefficient sets the bound max(c) * len(knots) far above the spline: acceptance small, not zero
    c[0] = 1.0 / dev.nc      # row 0: a flat spline, most proposals accepted
    x = out[3](0, c, 64)     # the default budget suffices
    assert torch.isfinite(x).all()
    with pytest.raises(RuntimeError, match="row 0"):
        out[3](0, c[[1]], 4096, max_proposals=2)   # (the flat row could run out of two proposals too: the peaked row alone)
