"""tests/rqs_fp64.py, the fp64 reference of the RQS family, pinned without a GPU: against the C oracle's fp32 restatement (oracle.rqs_batch),
and by its own consistency at fp64 accuracy.  Also the CPU side of what tests/test_gpu_rqs_fp64.py presumes about the fp32 reference."""
import numpy as np
import pytest

import oracle
import rqs_fp64 as R

KS = [4, 6, 16, 40, 64]
MODES = pytest.mark.parametrize("unconstrained", [False, True], ids=["RQS", "unconstrained"])
DIRS = pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])


def _figures(K, unconstrained, inverse, width, N=20000):
    nd = K - 1 if unconstrained else K + 1
    lo, hi = (-3.0, 3.0) if unconstrained else (0.0, 1.0)
    seed = 1000 * K + 10 * int(unconstrained) + int(inverse)
    uw, uh, ud = R.normal_params(N, K, nd, seed, width)
    x = R.uniform_inputs(N, lo, hi, seed + 1, unconstrained)
    y64, l64, b64, _, _ = R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi)
    yo, ldo, bo = oracle.rqs_batch(x, uw, uh, ud, inverse=inverse, left=lo, right=hi, bottom=lo, top=hi)
    special = ~np.isfinite(x) | (b64 < 0)
    # identity outside the tails and for NaN / inf: both agree bit for bit
    assert np.array_equal(bo[special], b64[special]) and np.array_equal(yo[special].view(np.uint32), x[special].view(np.uint32))
    assert np.array_equal(y64[special].astype(np.float32).view(np.uint32), x[special].view(np.uint32)) and np.all(l64[special] == 0) and np.all(ldo[special] == 0)
    assert not np.isnan(yo[~special]).any() and not np.isnan(ldo[~special]).any() and np.isfinite(y64[~special]).all() and np.isfinite(l64[~special]).all()
    same = (bo == b64) & ~special
    with np.errstate(invalid="ignore"):                         # (NaN - NaN at the NaN input: not among `same`)
        dy, dl = np.abs(yo - y64), np.abs(ldo - l64)
    ey, el = dy[same] / (hi - lo), dl[same]
    flipped = ~(bo == b64)
    assert np.all(dy[flipped] <= 2e-5 * (hi - lo))     # a flipped bin at a knot still gives a continuous map
    f = dict(mismatch=flipped.mean(), y_max=ey.max(), y_med=np.median(ey), y_999=np.quantile(ey, 0.999), ld_max=el.max(), ld_med=np.median(el),
             ld_999=np.quantile(el, 0.999))
    print(f"[rqs_fp64 vs oracle: K {K} {'unc' if unconstrained else 'RQS'} {'inv' if inverse else 'fwd'} width {width}] " + " ".join(f"{k} {v:.2e}" for k, v in f.items()))
    return f


@MODES
@DIRS
@pytest.mark.parametrize("K", KS)
def test_reference_agrees_with_the_fp32_oracle(K, unconstrained, inverse):
    """Standard-normal parameters, N = 20 000, x uniform over [0, 1] (RQS) or 10 % beyond the +-3 tails (unconstrained), errors of y as a
    fraction of the range.  Measured over the 20 cases (worst case each): no element differs in its bin (bound 1e-4: two elements); |y|
    differs by 1.6e-4 of the range at most (bound 2.5e-4; median 4.7e-8, bound 7e-8) and logabsdet by 5.9e-3 (bound 1e-2; median 5.1e-6,
    bound 8e-6); no NaN.  (The large single differences are fp32's own, in the inverse at K = 64: -b - sqrt(b^2 - 4ac) cancels where b < 0.)"""
    f = _figures(K, unconstrained, inverse, 1.0)
    assert f["mismatch"] <= 1e-4
    assert f["y_max"] <= 2.5e-4 and f["y_med"] <= 7e-8
    assert f["ld_max"] <= 1e-2 and f["ld_med"] <= 8e-6


@MODES
@DIRS
@pytest.mark.parametrize("K", KS)
def test_reference_agrees_with_the_fp32_oracle_on_wide_parameters(K, unconstrained, inverse):
    """Parameters three times wider: many bins sit at their 1e-3 minimum, where the fp32 formula itself loses accuracy (single elements are off by
    up to 4.1e-1 in logabsdet and 7.6e-4 of the range in y, inverse direction), so medians and 99.9th percentiles only are pinned here.  Measured
    (worst of the 20 cases): y median 3.8e-8 of the range (bound 6e-8), 99.9th percentile 1.05e-5 (bound 1.6e-5); logabsdet median 1.7e-5 (bound
    2.6e-5), 99.9th percentile 4.1e-3 (bound 6e-3); no element differs in its bin (bound 1e-4)."""
    f = _figures(K, unconstrained, inverse, 3.0)
    assert f["mismatch"] <= 1e-4
    assert f["y_med"] <= 6e-8 and f["y_999"] <= 1.6e-5
    assert f["ld_med"] <= 2.6e-5 and f["ld_999"] <= 6e-3


@MODES
@pytest.mark.parametrize("K", [4, 6, 16, 40, 64, 159])
def test_reference_is_consistent_with_itself(K, unconstrained):
    """In fp64, to 1e-10 (x as a fraction of the range): inverse(forward(x)) == x and the two logabsdets cancel, 5000 standard-normal rows;
    along a 4001-point scan of one element's spline y never decreases, forward and inverse, and logabsdet is the log of a fourth-order central
    finite difference of the map at every fourth scan point (step 1e-7 of the range; where the stencil stays inside one bin: the second derivative jumps at a knot), to the
    stencil's own rounding error, which 1 / slope amplifies (fd_check): 1e-8 + 4 * 2^-52 / (1e-7 slope), i.e. 2e-8 at best -- a difference
    quotient in float64 cannot reach 1e-10 (measured best 3e-9 .. 2e-7 over K = 4 .. 159 at any step).  An element that the round trip puts into
    the neighbouring bin at a knot is held to 1e-9 of the range in x instead (the map is continuous there, its log-det formula is the other bin's)."""
    N = 5000
    x, uw, uh, ud, lo, hi = R.case(K, N, unconstrained, 60 + K)
    x64 = np.where(np.isfinite(x), x, 0.0).astype(np.float64)
    T = np.float64
    c = lambda a: np.asarray(a, T)
    y, ld, b, _, _ = R._rqs(x64, c(uw), c(uh), c(ud), False, lo, hi, lo, hi, T)
    xb, ldb, bb, _, _ = R._rqs(y, c(uw), c(uh), c(ud), True, lo, hi, lo, hi, T)
    inside = b >= 0
    assert np.array_equal(bb[inside], b[inside]) or (bb != b).mean() < 1e-3
    ok = bb == b
    assert np.abs(xb - x64)[ok].max() <= 1e-10 * (hi - lo) and np.abs(ld + ldb)[ok].max() <= 1e-10
    assert np.abs(xb - x64).max() <= 1e-9 * (hi - lo)
    # scan
    n = 4001
    rep = lambda a, m=n: np.repeat(c(a[:1]), m, axis=0)
    t = np.linspace(1.1 * lo, 1.1 * hi, n) if unconstrained else np.linspace(lo, hi, n)
    ys, lds, bs, _, _ = R._rqs(t, rep(uw), rep(uh), rep(ud), False, lo, hi, lo, hi, T)
    assert np.all(np.diff(ys) >= 0) and len(np.unique(bs[bs >= 0])) == K
    assert abs(ys[bs >= 0][0] - max(lo, t[bs >= 0][0])) <= 1e-3 * (hi - lo) and np.all(ys[bs < 0] == t[bs < 0])
    eps = 1e-7 * (hi - lo)

    def fd_check(pts, inverse):
        """log of the fourth-order central difference (f(-2e) - 8 f(-e) + 8 f(e) - f(2e)) / 12e against logabsdet, where the whole stencil lies in
        one bin (or one tail).  Its rounding error is about 1.5 * 2^-52 * range / (eps * slope) relative, the truncation (eps / bin width)^4."""
        f = {s: R._rqs(pts + s * eps, rep(uw, pts.size), rep(uh, pts.size), rep(ud, pts.size), inverse, lo, hi, lo, hi, T) for s in (-2, -1, 0, 1, 2)}
        one_bin = np.all([f[s][2] == f[0][2] for s in (-2, -1, 1, 2)], axis=0)
        assert one_bin.mean() > 0.8
        fd = (f[-2][0] - 8 * f[-1][0] + 8 * f[1][0] - f[2][0]) / (12 * eps)
        slope = np.exp(f[0][1])
        err = np.abs(np.log(fd) - f[0][1])
        assert np.all(err[one_bin] <= 1e-8 + 4 * 2.0 ** -52 * (hi - lo) / (eps * slope[one_bin])), (err[one_bin] * slope[one_bin]).max()

    ti = np.linspace(lo, hi, n)
    fd_check(t[::4], False)                                      # (every fourth scan point: five evaluations each)
    fd_check(ti[::4], True)
    assert np.all(np.diff(R._rqs(ti, rep(uw), rep(uh), rep(ud), True, lo, hi, lo, hi, T)[0]) >= 0)


@pytest.mark.parametrize("reverse", [True, False], ids=["reverse", "plain"])
@pytest.mark.parametrize("dim,K,hidden", [(2, 5, 8), (8, 5, 8), (4, 12, 32), (6, 20, 8)])
def test_coupling_reference_inverts_itself(dim, K, hidden, reverse):
    """fp64: the layer's inverse undoes its direct map and the log-dets cancel; so does a three-layer stack with and without Reverse.  To 1e-10
    wherever conditioning allows it: the doubly normalised parameters of a coupling layer produce slopes down to 1e-5 (a flat bin between knot
    derivatives >= 0.69), every half-step of the inverse amplifies the rounding it receives by up to 1 / slope, and the next one is conditioned
    on its result -- so the bound per walker is 1e-10 + 1e-14 A (x, as a fraction of the range) and 1e-10 + 1e-12 A for the log-dets (whose
    derivative along a bin is up to ~1e2 times steeper), A = the product over the half-steps of max(1, 1 / flattest slope).  The weights are the
    GPU test's (initial networks times 2).  And the fp32 leg: the same lines in float32 stay in float32 and land next to the fp64 result."""
    from waveflow_amd.flows.neural_splines import NeuralSplineCoupling
    g = np.random.default_rng(dim + K)
    scaled = lambda net: [tuple(a * np.float32(2.0) for a in l) if l else () for l in net]      # the GPU test's weights: initial networks times 2
    layers = [tuple(scaled(net) for net in NeuralSplineCoupling(K=K, B=3.0, hidden_dim=hidden).init_params(g, dim)) for _ in range(3)]
    x = g.uniform(-3.45, 3.45, size=(2000, dim)).astype(np.float32)
    def round_trip(x, xb, ld, ldb, details, tag):
        # per walker: every half-step the inverse goes back through amplifies what it receives by at most 1 / (its flattest coordinate's slope)
        amp = np.prod([np.maximum(1.0, np.exp(-d[3].min(1))) for d in details], axis=0)
        ex, el = np.abs(xb - x).max(1) / 6.0, np.abs(ld + ldb)
        print(f"[coupling reference {tag} dim {dim} K {K}] round trip: x {ex.max():.1e} of the range, log-det {el.max():.1e}, largest amplification {amp.max():.1e}")
        assert np.all(ex <= 1e-10 + 1e-14 * amp) and np.all(el <= 1e-10 + 1e-12 * amp)

    det = []
    y, ld = R.nsc_layer(layers[0], x, K, 3.0, details=det)
    xb, ldb = R.nsc_layer(layers[0], y, K, 3.0, inverse=True)
    assert np.abs(y - x).max() > 0.1
    round_trip(x, xb, ld, ldb, det, "layer")
    outside = np.abs(x) > 3.0
    assert np.array_equal(y[outside], x[outside].astype(np.float64))
    det = []
    z, l = R.nsc_stack(layers, x, K, 3.0, reverse, details=det)
    xs, ls = R.nsc_stack(layers, z, K, 3.0, reverse, inverse=True)
    round_trip(x, xs, l, ls, det, "stack")
    if reverse:                                                   # Reverse matters: without it the stack is a different map
        assert np.abs(R.nsc_stack(layers, x, K, 3.0, False)[0] - z).max() > 1e-3
    z32, l32 = R.nsc_stack(layers, x, K, 3.0, reverse, dtype=np.float32)
    assert z32.dtype == np.float32 and l32.dtype == np.float32
    assert np.median(np.abs(z32 - z)) <= 1e-5 and np.median(np.abs(l32 - l)) <= 1e-4
    lp, u = R.flow_log_pdf(layers, x, K, 3.0, reverse, "normal", -0.25)
    assert np.allclose(lp, l - 0.5 * (np.log(2 * np.pi) + (z - 0.25) ** 2).sum(1), rtol=0, atol=1e-12) and np.array_equal(u, z)
    lpu, uu = R.flow_log_pdf(layers, x, K, 3.0, reverse, "uniform")
    assert np.array_equal(lpu, l) and uu.min() >= 0.0 and uu.max() <= 1.0 and np.array_equal(uu, np.clip(z, 0, 1))


@MODES
@DIRS
@pytest.mark.parametrize("K", R.HARD_K)
def test_fp32_reference_is_finite_and_in_range_on_the_hard_set(K, unconstrained, inverse):
    """What test_rqs_hard_set of the GPU suite presumes: on exactly its inputs (rqs_fp64.hard_case) the fp32 oracle, and the float32 run of
    rqs_fp64, are finite wherever the spline is evaluated and stay inside the range to 1e-6 of it."""
    x, uw, uh, ud, lo, hi = R.hard_case(K, unconstrained, inverse)
    b64 = R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi)[2]
    inside = b64 >= 0
    assert inside.sum() > 0.8 * x.size
    tol = 1e-6 * (hi - lo)
    for y, ld, b in (oracle.rqs_batch(x, uw, uh, ud, inverse=inverse, left=lo, right=hi, bottom=lo, top=hi),
                     R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi, dtype=np.float32)[:3]):
        assert np.isfinite(y[inside]).all() and np.isfinite(ld[inside]).all()
        assert y[inside].min() >= lo - tol and y[inside].max() <= hi + tol


@DIRS
@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
def test_fp32_oracle_maps_knots_onto_knots(K, inverse):
    """What test_rqs_on_the_knots presumes (rqs_fp64.knot_inputs: equal widths and heights, tail 1): the oracle sends every knot onto itself
    exactly, gives no NaN on the knots and their +-1..4 ulp neighbours, and puts a knot into the bin on its right (the last one: the last bin)."""
    x, uw, uh, ud, on_knot = R.knot_inputs(K, 1.0, 31 + K)
    y, ld, b = oracle.rqs_batch(x, uw, uh, ud, inverse=inverse, left=-1.0, right=1.0, bottom=-1.0, top=1.0)
    assert not np.isnan(y).any() and not np.isnan(ld).any()
    assert np.array_equal(y[on_knot], x[on_knot])
    assert np.array_equal(b[on_knot], np.minimum(np.arange(K + 1), K - 1))
    y64 = R.rqs(x, uw, uh, ud, inverse, -1.0, 1.0, -1.0, 1.0)[0]
    assert np.abs(y - y64).max() <= 2e-5 * 2.0
