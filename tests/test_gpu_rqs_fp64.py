"""The RQS and spline-coupling kernels (wf_kernels_rqs.hip) against the fp64 reference of tests/rqs_fp64.py, on every kernel family,
instantiation and staging / loop path.

Which kernel a case runs, read from the dispatch (no counters in the kernels):
  launch_rqs:       K in {4, 8, 16, 32} and uw, uh both 16-byte aligned -> k_rqs_reg<K> (grid capped at 4096 blocks of 256); everything else ->
                    k_rqs, the LDS-staged kernel (grid capped at 2048 blocks; 256 (K + 1) 4 bytes of LDS: beyond 64 KiB from K = 64 on --
                    ensure_dynamic_lds -- and all 160 KiB at K = 159 = WF_RQS_MAX_BINS); stage_tile copies with 16-byte loads when the
                    tile's first float is 16-byte aligned and dword by dword otherwise.
  wf_nsc_fwd:       nsc_model_built (dim 2..8 even, K 2..16, hidden 8 or 32) and WF_NSC_STAGED unset -> launch_nsc_model (one layer, modes
                    2 / 3); otherwise launch_nsc: k_nsc_cond -> launch_rqs -> k_nsc_cond -> launch_rqs -> k_nsc_finish.
  launch_nsc_model: hidden 8, K 5, dim 2 -> <8, 8, 1, 5>; hidden 8, K 5, dim 4 -> <8, 8, 2, 5>; hidden 8: K <= 8 -> <8, 8>, else <8, 16>;
                    hidden 32: K <= 8 -> <32, 8>, else <32, 16>; grid capped at 4096 blocks of 256.

The yardstick is the project's (tests/test_gpu_coord_derivs.py): e_g = |gpu - fp64|, e_o = |fp32 reference - fp64|, scale = the range for y and 1
for logabsdet; median(e_g) <= 3 median(e_o) + 1e-6 scale and max(e_g) <= 4 max(e_o) + 2e-5 scale, over the elements whose bin equals the
fp64 bin.  The fp32 reference is the C oracle up to K = 64 and rqs_fp64 in float32 beyond and for the coupling layers.  At most 2e-3 of
the elements may differ in their bin (x within rounding of a knot), and those still have to meet |y - y64| <= 2e-5 scale."""
import numpy as np
import pytest

import oracle
import rqs_fp64 as R

pytestmark = pytest.mark.gpu

# The project's factors; none had to be raised.  Measured on an MI355X, worst e_g / e_o of any populated case (median, max; before the additive
# terms, which carry the few cases above 4):
#   k_rqs_reg<4|8|16|32>  y 1.11, 3.48   logabsdet 1.28, 3.09          k_rqs (K 5 .. 159)   y 2.00, 2.99   logabsdet 1.37, 2.55
#   hard sets (median, 99.9th percentile)  registers 1.23, 1.77        staged 1.19, 1.47
#   grid-stride second trips 1.05, 1.70    4-byte-offset views 1.11, 1.01
#   k_nsc_model<8, 8> (incl. <8, 8, 1, 5>, <8, 8, 2, 5>)  y 1.32, 2.49   logdet 1.28, 1.90      <8, 16>   y 1.18, 1.24   logdet 1.29, 1.30
#   k_nsc_model<32, 8>  y 1.14, 1.76   logdet 1.13, 1.84               <32, 16>  y 1.26, 8.21 (2.0e-5 against 2.4e-6: inside 2e-5 scale)   logdet 1.21, 1.55
#   staged coupling path  y 1.44, 5.78 (1.5e-5 against 2.6e-6: inside 2e-5 scale)   logdet 1.22, 2.13
#   the stack as a model (L = 3)  y 1.14, 1.81   log_pdf / logdet 1.08, 2.48
#   the Uniform prior's clipped sample where 0 < z < 1  y 1.19, 1.14      B = 4096 256 + 1  y 1.26, 2.14   log_pdf 1.21, 1.35
MED, MAX = 3.0, 4.0
SENTINEL = -12345.678
REG_K, GEN_K = (4, 8, 16, 32), (5, 6, 40, 64, 159)


# ---------------------------------------------------------------- plumbing
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offset_copy(t):
    """The same numbers in a contiguous view that starts 4 bytes behind a 16-byte boundary."""
    import torch
    big = torch.empty(t.numel() + 8, device="cuda", dtype=t.dtype)
    v = big[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def gpu_rqs(x, uw, uh, ud, inverse, lo, hi, offset=(), status=False):
    """wf_rqs_fwd on device copies of the inputs; `offset` names the arrays (x, uw, uh, ud, out) taken from a 4-byte-offset view.  The outputs
    are over-allocated by one element and pre-filled: no fill value may survive inside, the extra element must stay."""
    import torch
    from waveflow_amd import _lib
    P = _lib.ptr
    dev = {k: _t(v) for k, v in (("x", x), ("uw", uw), ("uh", uh), ("ud", ud))}
    for k in offset:
        if k in dev:
            dev[k] = _offset_copy(dev[k])
    N, K = uw.shape
    pad = 9 if "out" in offset else 1
    bufs = [torch.full((N + pad,), SENTINEL, device="cuda"), torch.full((N + pad,), SENTINEL, device="cuda"),
            torch.full((N + pad,), -77, device="cuda", dtype=torch.int32)]
    outs = [b[1:1 + N] if "out" in offset else b[:N] for b in bufs]
    if "out" in offset:
        assert all(o.data_ptr() % 16 == 4 for o in outs)
    rc = _lib.lib().wf_rqs_fwd(P(dev["x"]), P(dev["uw"]), P(dev["uh"]), P(dev["ud"]), N, K, ud.shape[1], int(inverse), lo, hi, lo, hi,
                               P(outs[0]), P(outs[1]), P(outs[2]), _lib.stream_ptr())
    torch.cuda.synchronize()
    full = [b.cpu().numpy() for b in bufs]
    if status:
        return rc, full
    assert rc == 0, rc
    s = np.float32(SENTINEL)
    first = 1 if "out" in offset else 0
    for f, fill in zip(full, (s, s, -77)):
        inner = f[first:first + N]
        assert not np.any(inner == fill), "an output element was not written"
        assert np.all(f[:first] == fill) and np.all(f[first + N:] == fill), "an element outside the output was written"
    return tuple(f[first:first + N] for f in full)


def ref32(x, uw, uh, ud, inverse, lo, hi):
    if uw.shape[1] <= 64:
        return oracle.rqs_batch(x, uw, uh, ud, inverse=inverse, left=lo, right=hi, bottom=lo, top=hi)
    return R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi, dtype=np.float32)[:3]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def yardstick(tag, x, got, r64, r32, scale, med=MED, mx=MAX, quantile=None):
    """The comparison described at the top.  quantile = 0.999 replaces the maximum (the hard sets).  -> the measured ratios."""
    y, ld, b = got
    y64, l64, b64 = r64[:3]
    y32, l32, b32 = r32
    special = ~np.isfinite(x) | (b64 < 0)
    # outside the tails or not finite: y == x bit for bit (NaN stays NaN), logabsdet == 0, bin == -1
    assert np.array_equal(_bits(y[special]), _bits(x[special])) and np.all(ld[special] == 0) and np.all(b[special] == -1), tag
    assert np.all(b[~special] >= 0), tag
    fin = np.isfinite(y64) & np.isfinite(l64)
    assert fin[~special].all(), tag                       # (the fp64 reference itself is finite wherever the spline is evaluated)
    same_g, same_o = (b == b64) & ~special, (b32 == b64) & ~special
    aside = ~(b == b64)
    assert aside.sum() <= 2e-3 * x.size, (tag, int(aside.sum()), x.size)
    assert np.all(np.abs(y[aside] - y64[aside]) <= 2e-5 * scale), (tag, np.abs(y[aside] - y64[aside]).max())
    top = (lambda e: np.quantile(e, quantile)) if quantile else np.max
    ratios = {}
    for what, g, o, r, sc in (("y", y, y32, y64, scale), ("logabsdet", ld, l32, l64, 1.0)):
        assert np.isfinite(g[same_g]).all(), (tag, what)
        if not same_g.any():
            continue
        e_g, e_o = np.abs(g[same_g] - r[same_g]), np.abs(o[same_o] - r[same_o])
        e_o = e_o if e_o.size else np.zeros(1)
        ratios[what] = (np.median(e_g) / max(np.median(e_o), 1e-30), top(e_g) / max(top(e_o), 1e-30))
        print(f"[{tag}] {what}: median e_g {np.median(e_g):.2e} e_o {np.median(e_o):.2e}, {'q' + str(quantile) if quantile else 'max'} e_g {top(e_g):.2e} "
              f"e_o {top(e_o):.2e}, bins set aside {int(aside.sum())} of {x.size}")
        assert np.median(e_g) <= med * np.median(e_o) + 1e-6 * sc, (tag, what, np.median(e_g), np.median(e_o))
        assert top(e_g) <= mx * top(e_o) + 2e-5 * sc, (tag, what, top(e_g), top(e_o))
    return ratios


def _case(K, N, unconstrained, inverse, seed, hard=False):
    return R.case(K, N, unconstrained, seed + 500 * int(inverse), hard)


# ---------------------------------------------------------------- wf_rqs_fwd
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("unconstrained", [False, True], ids=["RQS", "unconstrained"])
@pytest.mark.parametrize("K,N", [(K, N) for K in REG_K + GEN_K for N in ((1, 257) if K >= 64 else (1, 255, 257, 4099))])
def test_rqs_against_fp64(K, N, unconstrained, inverse):
    """Standard-normal parameters, x (y for the inverse) uniform over the range -- [0, 1] for RQS, 10 % beyond the +-3 tails with +-tail,
    their outer neighbours, 0, NaN and +-inf in front for the unconstrained form.  K in {4, 8, 16, 32}: k_rqs_reg<K>; {5, 6, 40, 64, 159}: k_rqs
    (K = 64: 65 KiB of LDS, the ensure_dynamic_lds branch; K = 159: all 160 KiB).  The project's factors 3 / 4 hold on every case: measured
    ratios e_g / e_o are printed per case and summarised in DESIGN.md 4.4.
    N = 1: a median and a maximum over one element compare one rounding error with another (measured: e_g / e_o from 0.01 to 11 on single
    elements of populations that pass with ratios below 1.4 / 3.5).  The one-element launch is therefore run on a row of the 257-row case, must
    give that row's bits (an element's arithmetic does not depend on N), and the yardstick is applied to the 257 rows it belongs to."""
    tag = f"rqs K {K} N {N} {'unc' if unconstrained else 'RQS'} {'inv' if inverse else 'fwd'}"
    M = 257 if N == 1 else N                              # (N = 255 is a single partial block: it runs 255 rows)
    x, uw, uh, ud, lo, hi = _case(K, M, unconstrained, inverse, 100 * K + M)
    got = gpu_rqs(x, uw, uh, ud, inverse, lo, hi)
    if N == 1:
        for i in (0, 5, 11):                              # -tail itself, NaN (unconstrained form), an ordinary row
            one = gpu_rqs(x[i:i + 1], uw[i:i + 1], uh[i:i + 1], ud[i:i + 1], inverse, lo, hi)
            assert all(np.array_equal(a.view(np.uint32), c[i:i + 1].view(np.uint32)) for a, c in zip(one, got)), (tag, i)
    yardstick(tag, x, got, R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi), ref32(x, uw, uh, ud, inverse, lo, hi), hi - lo)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("unconstrained", [False, True], ids=["RQS", "unconstrained"])
@pytest.mark.parametrize("K", R.HARD_K)
def test_rqs_hard_set(K, unconstrained, inverse):
    """rqs_fp64.hard_params: parameters three times wider and saturated rows (one entry of +60, all entries equal, derivatives of +-30).  The fp32
    formula itself loses accuracy where a bin sits at its 1e-3 minimum (tests/test_rqs_fp64_host.py), so medians and 99.9th percentiles only --
    and every output finite where fp64 is, and inside the range to 1e-6 of it."""
    x, uw, uh, ud, lo, hi = R.hard_case(K, unconstrained, inverse)
    got = gpu_rqs(x, uw, uh, ud, inverse, lo, hi)
    r64 = R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi)
    inside = r64[2] >= 0
    assert np.isfinite(got[0][inside]).all() and np.isfinite(got[1][inside]).all()
    tol = 1e-6 * (hi - lo)
    assert got[0][inside].min() >= lo - tol and got[0][inside].max() <= hi + tol
    yardstick(f"rqs hard K {K} {'unc' if unconstrained else 'RQS'} {'inv' if inverse else 'fwd'}", x, got, r64, ref32(x, uw, uh, ud, inverse, lo, hi),
              hi - lo, quantile=0.999)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
def test_rqs_on_the_knots(K, inverse):
    """Equal unnormalised widths and heights, tail 1: the knots -1 + 2 i / K are exact, kernel and oracle hold the same ones, the map sends knots to
    knots.  x on every knot and its +-1..4 ulp neighbours, random derivatives three times wider: the bins are the oracle's, nothing is NaN, and
    on the knots y == x to 1e-6 of the range.  (K = 64: the staged kernel.)"""
    x, uw, uh, ud, on_knot = R.knot_inputs(K, 1.0, 31 + K)
    y, ld, b = gpu_rqs(x, uw, uh, ud, inverse, -1.0, 1.0)
    yo, ldo, bo = oracle.rqs_batch(x, uw, uh, ud, inverse=inverse, left=-1.0, right=1.0, bottom=-1.0, top=1.0)
    assert np.array_equal(b, bo), (x[b != bo][:8], b[b != bo][:8], bo[b != bo][:8])
    assert not np.isnan(y).any() and not np.isnan(ld).any()
    assert np.abs(y[on_knot] - x[on_knot]).max() <= 1e-6 * 2.0
    inside = np.abs(x) <= 1.0
    assert np.array_equal(np.unique(b[inside]), np.arange(K)) and np.all(b[~inside] == -1)
    y64 = R.rqs(x, uw, uh, ud, inverse, -1.0, 1.0, -1.0, 1.0)[0]
    assert np.abs(y - y64).max() <= 2e-5 * 2.0       # (whatever bin fp64 picks next to a knot: the map is continuous)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("K,unconstrained", [(8, True), (8, False), (6, True), (6, False), (64, True)])
def test_rqs_scan_is_monotone(K, unconstrained, inverse):
    """One element's parameters repeated over a sorted 4001-point scan (through the +-tail bounds for the unconstrained form, where the map
    continues as the identity): y never decreases by more than 1e-6 of the range, across knots and tail bounds included."""
    n = 4001
    nd = K - 1 if unconstrained else K + 1
    lo, hi = (-3.0, 3.0) if unconstrained else (0.0, 1.0)
    uw, uh, ud = (np.repeat(a, n, axis=0) for a in R.normal_params(1, K, nd, 900 + K))
    t = np.linspace(1.1 * lo, 1.1 * hi, n, dtype=np.float32) if unconstrained else np.linspace(lo, hi, n, dtype=np.float32)
    y, ld, b = gpu_rqs(t, uw, uh, ud, inverse, lo, hi)
    assert np.diff(y.astype(np.float64)).min() >= -1e-6 * (hi - lo), np.diff(y.astype(np.float64)).min()
    assert len(np.unique(b[b >= 0])) == K                                            # the scan crosses every knot
    if unconstrained:
        assert np.array_equal(y[b < 0], t[b < 0]) and (b < 0).sum() > 300                # ... and both tail bounds


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("K,N", [(4, 4096 * 256 + 257), (6, 2048 * 256 + 255)], ids=["registers", "staged"])
def test_rqs_grid_stride_second_trip(K, N, inverse):
    """More elements than the capped grid covers in one trip (k_rqs_reg: 4096 blocks, k_rqs: 2048 blocks, of 256), with a ragged last block:
    compared with fp64 everywhere; gpu_rqs pre-fills the outputs and checks that every element inside was written and the one behind was not."""
    x, uw, uh, ud, lo, hi = _case(K, N, True, inverse, 5 + K)
    got = gpu_rqs(x, uw, uh, ud, inverse, lo, hi)
    yardstick(f"rqs grid-stride K {K} N {N} {'inv' if inverse else 'fwd'}", x, got, R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi),
              ref32(x, uw, uh, ud, inverse, lo, hi), hi - lo)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("K", [8, 6])
def test_rqs_alignment(K, inverse):
    """uw alone, uh alone and both from a view 4 bytes behind a 16-byte boundary (the scalar staging of stage_tile); then x, ud and the outputs
    too.  K = 6: both runs use k_rqs and must give the same bits.  K = 8: the offset run leaves k_rqs_reg<8> for k_rqs (launch_rqs), a different
    sum order, so both are held to the fp64 yardstick instead."""
    N = 1031
    x, uw, uh, ud, lo, hi = _case(K, N, True, inverse, 40 + K)
    r64, r32 = R.rqs(x, uw, uh, ud, inverse, lo, hi, lo, hi), ref32(x, uw, uh, ud, inverse, lo, hi)
    base = gpu_rqs(x, uw, uh, ud, inverse, lo, hi)
    yardstick(f"rqs aligned K {K}", x, base, r64, r32, hi - lo)
    for offset in (("uw",), ("uh",), ("uw", "uh"), ("x", "ud", "out"), ("x", "uw", "uh", "ud", "out")):
        got = gpu_rqs(x, uw, uh, ud, inverse, lo, hi, offset=offset)
        yardstick(f"rqs K {K} offset {'+'.join(offset)}", x, got, r64, r32, hi - lo)
        if K == 6 or not ({"uw", "uh"} & set(offset)):     # the same kernel ran: the same bits
            assert all(np.array_equal(a.view(np.uint32), c.view(np.uint32)) for a, c in zip(got, base)), offset


def test_rqs_bin_count_contract():
    """wf_rqs_fwd stages 256 (K + 1) floats in LDS: K <= WF_RQS_MAX_BINS = 159 fits the 160 KiB of a CU (and is compared with fp64 in
    test_rqs_against_fp64); K in 160 .. 256 returns WF_ERR_UNSUPPORTED before any device call and leaves the outputs alone; K > 256 is invalid."""
    from waveflow_amd import _lib
    for K in (160, 256):
        for unconstrained in (True, False):
            for inverse in (False, True):
                x, uw, uh, ud, lo, hi = _case(K, 257, unconstrained, inverse, K)
                rc, full = gpu_rqs(x, uw, uh, ud, inverse, lo, hi, status=True)
                assert rc == -2, (K, rc)
                assert np.all(full[0] == np.float32(SENTINEL)) and np.all(full[1] == np.float32(SENTINEL)) and np.all(full[2] == -77)
    L = _lib.lib()
    assert L.wf_rqs_fwd(None, None, None, None, 0, 160, 159, 0, 0.0, 1.0, 0.0, 1.0, None, None, None, None) == -2    # (N = 0 as well)
    assert L.wf_rqs_fwd(None, None, None, None, 0, 159, 158, 0, 0.0, 1.0, 0.0, 1.0, None, None, None, None) == 0
    assert L.wf_rqs_fwd(None, None, None, None, 0, 257, 256, 0, 0.0, 1.0, 0.0, 1.0, None, None, None, None) == -1


# ---------------------------------------------------------------- the coupling kernels
TAIL = 3.0
WEIGHT_SCALE = 2.0


def _scaled(net):
    return [tuple(np.asarray(a * np.float32(WEIGHT_SCALE), np.float32) for a in l) if l else () for l in net]


def _walkers(B, dim, seed):
    return np.random.default_rng(seed).uniform(-1.15 * TAIL, 1.15 * TAIL, size=(B, dim)).astype(np.float32)


def couple_yardstick(tag, got, r64, r32, med=MED, mx=MAX):
    """The coupling entry points return no bins, and need none: an RQS and its derivative are continuous across knots, so every walker is
    compared (nothing set aside).  Per walker: max over the coordinates of |y - y64| against the range 2 tail; |logdet - logdet64| against 1.
    got[1] is None where the entry point returns no log-det (inverse): y alone is judged then."""
    ratios = {}
    for what, g, o, r, sc in (("y", got[0], r32[0], r64[0], 2 * TAIL), ("logdet", got[1], r32[1], r64[1], 1.0)):
        if g is None:
            continue
        assert np.isfinite(g).all(), (tag, what)
        e_g, e_o = np.abs(g - r).reshape(len(g), -1).max(1), np.abs(o - r).reshape(len(g), -1).max(1)
        ratios[what] = (np.median(e_g) / max(np.median(e_o), 1e-30), e_g.max() / max(e_o.max(), 1e-30))
        print(f"[{tag}] {what}: median e_g {np.median(e_g):.2e} e_o {np.median(e_o):.2e}, max e_g {e_g.max():.2e} e_o {e_o.max():.2e}")
        assert np.median(e_g) <= med * np.median(e_o) + 1e-6 * sc, (tag, what, np.median(e_g), np.median(e_o))
        assert e_g.max() <= mx * e_o.max() + 2e-5 * sc, (tag, what, e_g.max(), e_o.max())
    return ratios


ONE_KERNEL = [(2, 5, 8), (4, 5, 8), (8, 5, 8), (6, 8, 8), (4, 12, 8), (8, 16, 32), (2, 9, 32), (6, 5, 32)]
STAGED = [(4, 5, 16), (4, 32, 8), (6, 20, 8)]


@pytest.mark.parametrize("B", [1, 255, 4099])
@pytest.mark.parametrize("dim,K,hidden,force_staged", [c + (False,) for c in ONE_KERNEL + STAGED] + [(4, 8, 8, True)])
def test_coupling_layer_against_fp64(dim, K, hidden, force_staged, B, monkeypatch):
    """wf_nsc_fwd, direct and inverse, against the fp64 layer of rqs_fp64 (the inverse against the fp64 inverse of the same fp32 input, not by
    a round trip); the fp32 leg of the yardstick is rqs_fp64 in float32.
    One kernel: (2, 5, 8) <8, 8, 1, 5>; (4, 5, 8) <8, 8, 2, 5>; (8, 5, 8) and (6, 8, 8) <8, 8> (dh = 4: every `a < 4` guard live); (4, 12, 8) <8, 16>;
    (8, 16, 32) and (2, 9, 32) <32, 16>; (6, 5, 32) <32, 8>.  Staged: hidden 16 and K > 16 are not built as one kernel -- (4, 5, 16) k_rqs,
    (4, 32, 8) k_rqs_reg<32>, (6, 20, 8) k_rqs; (4, 8, 8) under WF_NSC_STAGED=1 k_rqs_reg<8> (the workspace's uh rows start B dh K floats behind
    the uw rows: a multiple of 16 bytes at K = 8 and 32 for every B, so launch_rqs keeps the register kernels).
    Weights AND biases of the initial networks (glorot-normal weights, biases of 1e-6) times 2: every shape moves some walker by more than 0.1
    (0.17 at K = 32 up to 5.6 at K = 5; asserted), the conditioner's tanh units are not saturated, local slopes stay between 5e-5 and 2e2.  At
    this scale the fp32 reference's own error e_o is (CPU, 4099 walkers): y median 4e-8 .. 1.2e-7 of the range, max 4e-7 .. 2e-5; logdet median
    1e-6 .. 3e-6, max 1e-5 .. 4e-4.  Walkers uniform in +-1.15 tail."""
    from waveflow_amd import flows
    if force_staged:
        monkeypatch.setenv("WF_NSC_STAGED", "1")
    params, direct_fun, inverse_fun = flows.NeuralSplineCoupling(K=K, B=TAIL, hidden_dim=hidden)(17 + dim + K, dim)
    params = tuple(_scaled(net) for net in params)
    x = _walkers(max(B, 255), dim, 3 * max(B, 255) + dim)
    for inverse, fun in ((False, direct_fun), (True, inverse_fun)):
        got = fun(params, x)
        if B == 1:       # one walker is no population (test_rqs_against_fp64): its launch must give the bits it has among the 255 judged below
            for i in (0, 7):
                one = fun(params, x[i:i + 1])
                assert np.array_equal(_bits(one[0]), _bits(got[0][i:i + 1])) and np.array_equal(_bits(one[1]), _bits(got[1][i:i + 1])), (i, inverse)
        r64 = R.nsc_layer(params, x, K, TAIL, inverse)
        r32 = R.nsc_layer(params, x, K, TAIL, inverse, dtype=np.float32)
        outside = np.abs(x) > TAIL
        assert np.array_equal(_bits(got[0][outside]), _bits(x[outside]))               # identity beyond the tails, bit for bit
        assert np.abs(r64[0] - x).max() > 0.1                                          # the layer does transform
        couple_yardstick(f"nsc layer dim {dim} K {K} hidden {hidden}{' staged' if force_staged else ''} B {B} {'inv' if inverse else 'dir'}",
                         got, r64, r32)


def _stack(dim, K, hidden, reverse, prior, L=3):
    from waveflow_amd import flows
    items = []
    for _ in range(L):
        items += [flows.NeuralSplineCoupling(K=K, B=TAIL, hidden_dim=hidden)] + ([flows.Reverse()] if reverse else [])
    pr = flows.Normal(-0.25) if prior == "normal" else flows.Uniform()
    params, log_pdf, sample = flows.Flow(flows.Serial(*items), pr, prior_support=None if prior == "normal" else (0.0, 1.0))(7, dim)
    assert log_pdf.model.desc.layer_kind == 2
    params = [tuple(_scaled(net) for net in p) if p else () for p in params]
    return params, [p for p in params if p], log_pdf, sample


@pytest.mark.parametrize("prior", ["normal", "uniform"])
@pytest.mark.parametrize("reverse", [True, False], ids=["reverse", "plain"])
@pytest.mark.parametrize("dim,K,hidden", [(8, 5, 8), (4, 12, 32)])
def test_coupling_stack_as_a_model_against_fp64(dim, K, hidden, reverse, prior):
    """layer_kind 2, L = 3: log_pdf with its sample (k_nsc_model mode 0), flow (mode 2) and inverse (mode 3) against the fp64 chain; the Uniform
    prior's clipped sample against clip(z64, 0, 1).  (8, 5, 8): <8, 8>; (4, 12, 32): <32, 16>.
    Under the Uniform prior most coordinates of z (walkers in +-3.45) lie outside (0, 1), where both sides clip to the same 0 or 1 and a median
    says nothing: the yardstick is applied to the coordinates with 0 < z64 < 1 (about one in seven; at least 500 asserted), the others must sit
    within 2e-5 of the range of clip(z64, 0, 1); the unclipped z is judged in full by the `flow` comparison below."""
    B = 4099
    params, layers, log_pdf, _ = _stack(dim, K, hidden, reverse, prior)
    x = _walkers(B, dim, 50 + dim)
    tag = f"nsc stack dim {dim} K {K} hidden {hidden} {'reverse' if reverse else 'plain'} {prior}"
    lp, u = log_pdf(params, x, return_sample=True)
    lp64, u64 = R.flow_log_pdf(layers, x, K, TAIL, reverse, prior, -0.25)
    lp32, u32 = R.flow_log_pdf(layers, x, K, TAIL, reverse, prior, -0.25, dtype=np.float32)
    u, lp = np.asarray(u), np.asarray(lp)
    if prior == "uniform":
        assert u.min() >= 0.0 and u.max() <= 1.0
        z64 = R.nsc_stack(layers, x, K, TAIL, reverse)[0]
        inner = (z64 > 0.0) & (z64 < 1.0)
        assert inner.sum() >= 500
        assert np.abs(u - u64)[~inner].max() <= 2e-5 * 2 * TAIL
        couple_yardstick(tag + " clipped sample, 0 < z < 1", (u[inner], None), (u64[inner], None), (u32[inner], None))
        couple_yardstick(tag + " log_pdf", (u, lp), (u64, lp64), (u32, lp32))
    else:
        couple_yardstick(tag + " log_pdf", (u, lp), (u64, lp64), (u32, lp32))
    m = log_pdf.model
    z, ld = m.flow(x)
    couple_yardstick(tag + " flow", (np.asarray(z), np.asarray(ld)), R.nsc_stack(layers, x, K, TAIL, reverse), R.nsc_stack(layers, x, K, TAIL, reverse, dtype=np.float32))
    xb = np.asarray(m.inverse(x))
    x64, li64 = R.nsc_stack(layers, x, K, TAIL, reverse, inverse=True)
    x32, li32 = R.nsc_stack(layers, x, K, TAIL, reverse, inverse=True, dtype=np.float32)
    couple_yardstick(tag + " inverse", (xb, None), (x64, li64), (x32, li32))


@pytest.mark.parametrize("mode", ["log_pdf", "inverse"])
def test_coupling_grid_stride_second_trip(mode):
    """B = 4096 256 + 1 walkers at (2, 5, 8): one more than the capped grid of k_nsc_model covers in one trip (modes 0 and 3).  The first and last
    2048 walkers and every 997th in between against fp64; the whole output was written (no fill value survives)."""
    import torch
    B = 4096 * 256 + 1
    params, layers, log_pdf, _ = _stack(2, 5, 8, True, "normal", L=1)
    x = _walkers(B, 2, 77)
    pick = np.unique(np.concatenate([np.arange(2048), np.arange(2048, B - 2048, 997), np.arange(B - 2048, B)]))
    m = log_pdf.model
    m.ensure_params(params)
    xd = torch.from_numpy(x).cuda()
    if mode == "log_pdf":
        out, u = torch.full((B,), SENTINEL, device="cuda"), torch.full((B, 2), SENTINEL, device="cuda")
        m._run("wf_logpdf_fwd", m._p(xd), B, m._p(out), m._p(u), None)
        out, u = out.cpu().numpy(), u.cpu().numpy()
        assert not np.any(out == np.float32(SENTINEL)) and not np.any(u == np.float32(SENTINEL))
        r64 = R.flow_log_pdf(layers, x[pick], 5, TAIL, True, "normal", -0.25)
        r32 = R.flow_log_pdf(layers, x[pick], 5, TAIL, True, "normal", -0.25, dtype=np.float32)
        couple_yardstick("nsc grid-stride log_pdf", (u[pick], out[pick]), (r64[1], r64[0]), (r32[1], r32[0]))
    else:
        xb = torch.full((B, 2), SENTINEL, device="cuda")
        m._run("wf_inverse_fwd", m._p(xd), B, m._p(xb), 0)
        xb = xb.cpu().numpy()
        assert not np.any(xb == np.float32(SENTINEL))
        x64, l64 = R.nsc_stack(layers, x[pick], 5, TAIL, True, inverse=True)
        x32, l32 = R.nsc_stack(layers, x[pick], 5, TAIL, True, inverse=True, dtype=np.float32)
        couple_yardstick("nsc grid-stride inverse", (xb[pick], None), (x64, l64), (x32, l32))


@pytest.mark.parametrize("prior", ["normal", "uniform"])
def test_coupling_latent_draws(prior):
    """k_nsc_latent through sample(..., return_original_samples=True): 2^16 x dim numbers, the bounds of test_chi_is_standard_normal
    (tests/test_gpu_dmc.py) -- five standard errors on mean and variance (Uniform(0, 1): mean 1/2, variance 1/12, fourth central moment 1/80),
    Kolmogorov-Smirnov p > 1e-4 --, the same bits on a second call, and a batch's first 64 rows equal to a 64-row call (streams are keyed by
    (seed, walker))."""
    from scipy import stats
    dim, B = 2, 1 << 16
    params, _, _, sample = _stack(dim, 5, 8, True, prior)
    s, lat = sample(3, params, B, return_original_samples=True)
    c = lat.double().cpu().numpy()
    n = c.size
    assert c.shape == (B, dim) and np.isfinite(c).all() and bool(s.isfinite().all())
    if prior == "normal":
        mean, var, se_mean, se_var, p = 0.0, 1.0, 1 / np.sqrt(n), np.sqrt(2.0 / n), stats.kstest(c.reshape(-1), "norm").pvalue
    else:
        assert c.min() >= 0.0 and c.max() <= 1.0
        mean, var, se_mean, se_var, p = 0.5, 1 / 12, np.sqrt(1 / 12 / n), np.sqrt((1 / 80 - 1 / 144) / n), stats.kstest(c.reshape(-1), "uniform").pvalue
    print(f"[nsc latent {prior}] n {n}: mean - {mean} {c.mean() - mean:+.2e} (bound {5 * se_mean:.2e}), var - {var:.4f} {c.var() - var:+.2e} (bound {5 * se_var:.2e}), KS p {p:.3f}")
    assert abs(c.mean() - mean) <= 5 * se_mean and abs(c.var() - var) <= 5 * se_var and p > 1e-4
    assert abs(np.corrcoef(c[:, 0], c[:, 1])[0, 1]) <= 5 / np.sqrt(B)
    s2, lat2 = sample(3, params, B, return_original_samples=True)
    assert np.array_equal(_bits(lat2.cpu().numpy()), _bits(lat.cpu().numpy())) and np.array_equal(_bits(s2.cpu().numpy()), _bits(s.cpu().numpy()))
    s3, lat3 = sample(3, params, 64, return_original_samples=True)
    assert np.array_equal(_bits(lat3.cpu().numpy()), _bits(lat.cpu().numpy())[:64]) and np.array_equal(_bits(s3.cpu().numpy()), _bits(s.cpu().numpy())[:64])
