"""High-precision reference of the rational-quadratic-spline family (a helper module, not a conftest).

Plain NumPy, vectorised over the elements, no limit on the number of bins.  Every function takes a `dtype`: float64 (the default) is the
reference; float32 runs the very same lines with every operation rounded to fp32 by NumPy -- the "fp32 reference" leg of the tests
where the C oracle does not reach (K > 64, the coupling layer).  The inputs are the fp32 numbers the kernels get, converted exactly.

Formulas as in the reference's flows/bijections/neural_splines.py:11-184 and :244-296:
  - widths / heights: min + (1 - min K) softmax, min = 1e-3; knots = lo + (hi - lo) cumsum, both end knots forced, sizes = differences;
  - bin = sum(x >= knots) - 1 with 1e-6 added to the last knot, clamped to [0, K - 1];
  - derivatives: 1e-3 + softplus; K + 1 columns is `RQS`, K - 1 columns is `unconstrained_RQS`, which pads both ends with
    log(exp(1 - 1e-3) - 1) (derivative exactly 1) and is the identity outside [left, right] (NaN included: not inside);
  - the inverse solves the quadratic with the root 2c / (-b - sqrt(b^2 - 4ac)) (in float64, where b < 0 makes that line cancel, the same
    root from its equivalent (-b + sqrt(b^2 - 4ac)) / (2a): see _rqs);
  - NeuralSplineCoupling: FCNN = Dense Tanh Dense Tanh Dense on the conditioning half; per transformed coordinate K, K, K - 1 columns,
    soft-max times 2B, soft-max times 2B, soft-plus -- handed to unconstrained_RQS as *unnormalised* parameters, which normalises them
    again (the reference's double application is kept);
  - the stack: Serial((layer [, Reverse]) x L) under Normal(offset) (log_pdf = sum norm.logpdf(z + offset)) or Uniform(0, 1) with
    prior_support (0, 1) (density 1, the returned sample clipped)."""
import numpy as np

MIN_SIZE = 1e-3
MIN_DERIVATIVE = 1e-3
LAST_KNOT_EPS = 1e-6


def _softmax(a, T):
    e = np.exp(a - a.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(T, copy=False)


def _softplus(a, T):
    return np.logaddexp(T(0), a).astype(T, copy=False)


def _knots(u, lo, hi, T):
    """[N][K + 1] knots and [N][K] bin sizes of one unnormalised array."""
    K = u.shape[-1]
    s = T(MIN_SIZE) + (T(1) - T(MIN_SIZE) * T(K)) * _softmax(u, T)
    cum = np.concatenate([np.zeros(u.shape[:-1] + (1,), T), np.cumsum(s, axis=-1, dtype=T)], -1)
    knots = (hi - lo) * cum + lo
    knots[..., 0] = lo
    knots[..., -1] = hi
    return knots, knots[..., 1:] - knots[..., :-1]


def edge_constant(T=np.float64):
    """unnormalised derivative of the padded ends: 1e-3 + softplus(c) == 1 (neural_splines.py:36)"""
    return np.log(np.exp(T(1) - T(MIN_DERIVATIVE)) - T(1))


def _rqs(x, uw, uh, ud, inverse, left, right, bottom, top, T):
    """The operation on arrays that already are of type T."""
    N, K = uw.shape
    assert x.dtype == uw.dtype == uh.dtype == ud.dtype == np.dtype(T)
    assert uh.shape == (N, K) and x.shape == (N,) and ud.shape[0] == N and ud.shape[1] in (K - 1, K + 1)
    left, right, bottom, top = T(left), T(right), T(bottom), T(top)
    if ud.shape[1] == K - 1:
        pad = np.full((N, 1), edge_constant(T), T)
        ud = np.concatenate([pad, ud, pad], 1)
        inside = (x >= left) & (x <= right)
    else:
        inside = np.ones(N, bool)
    xin = np.where(inside, x, left)                     # (the elements outside are overwritten below)
    cw, w = _knots(uw, left, right, T)
    ch, h = _knots(uh, bottom, top, T)
    d = T(MIN_DERIVATIVE) + _softplus(ud, T)
    loc = (ch if inverse else cw).copy()
    loc[:, -1] += T(LAST_KNOT_EPS)
    b = np.clip((xin[:, None] >= loc).sum(-1) - 1, 0, K - 1)
    pick = lambda a, i=b: np.take_along_axis(a, i[:, None], -1)[:, 0]
    in_cw, in_w, in_ch, in_h = pick(cw), pick(w), pick(ch), pick(h)
    delta = in_h / in_w
    d0, d1 = pick(d), pick(d, b + 1)
    with np.errstate(all="ignore"):
        if inverse:
            a = (xin - in_ch) * (d0 + d1 - 2 * delta) + in_h * (delta - d0)
            bq = in_h * d0 - (xin - in_ch) * (d0 + d1 - 2 * delta)
            cq = -delta * (xin - in_ch)
            disc = bq * bq - 4 * a * cq
            root = (2 * cq) / (-bq - np.sqrt(disc))
            if T is np.float64:
                # bq < 0 (x far into a bin whose right derivative exceeds 2 delta): -bq - sqrt(disc) cancels and the line above keeps 1e-9 at
                # best.  The reference takes the same root from its other expression, 2c / (-b - s) == (-b + s) / (2a) (the roots' product is
                # c / a), which does not cancel there.  The float32 run keeps the formula as the kernels and the C oracle have it.
                stable = (bq < 0) & (a != 0)
                root = np.where(stable, (-bq + np.sqrt(disc)) / np.where(stable, 2 * a, 1.0), root)
            y = root * in_w + in_cw
            t1 = root * (1 - root)
            den = delta + (d0 + d1 - 2 * delta) * t1
            num = delta * delta * (d1 * root * root + 2 * delta * t1 + d0 * (1 - root) * (1 - root))
            ld = -(np.log(num) - 2 * np.log(den))
        else:
            th = (xin - in_cw) / in_w
            t1 = th * (1 - th)
            num = in_h * (delta * th * th + d0 * t1)
            den = delta + (d0 + d1 - 2 * delta) * t1
            y = in_ch + num / den
            dnum = delta * delta * (d1 * th * th + 2 * delta * t1 + d0 * (1 - th) * (1 - th))
            ld = np.log(dnum) - 2 * np.log(den)
    for a in (y, ld):
        assert a.dtype == np.dtype(T)
    return np.where(inside, y, x), np.where(inside, ld, T(0)), np.where(inside, b, -1).astype(np.int32), in_w, in_h


def rqs(x, uw, uh, ud, inverse=False, left=0.0, right=1.0, bottom=0.0, top=1.0, dtype=np.float64):
    """RQS (ud [N][K + 1]) / unconstrained_RQS (ud [N][K - 1]) of fp32 inputs -> y [N], logabsdet [N], bin [N] (int32, -1 outside the
    tails of the unconstrained form), and the selected bin's width and height (what conditions the element: the forward map divides
    by the width, the inverse amplifies by 1 / slope)."""
    T = np.dtype(dtype).type
    c = lambda a: np.asarray(a, np.float32).astype(T)
    return _rqs(c(x).reshape(-1), c(uw), c(uh), c(ud), bool(inverse), left, right, bottom, top, T)


# ---------------------------------------------------------------- NeuralSplineCoupling, the stack, the priors

def _fcnn(net, v, T):
    (W1, b1), _, (W2, b2), _, (W3, b3) = net
    c = lambda a: np.asarray(a, np.float32).astype(T)
    h = np.tanh(v @ c(W1) + c(b1))
    h = np.tanh(h @ c(W2) + c(b2))
    return (h @ c(W3) + c(b3)).astype(T, copy=False)


def nsc_half(net, cond, trans, K, tail, inverse, T, details=None):
    """One half-step: the columns `trans` [B][dh] through unconstrained_RQS conditioned on `cond` [B][dh] -> new columns, log-dets [B][dh].
    The conditioner's outputs stay of type T (in the fp64 chain they are not rounded to fp32 on the way into the spline)."""
    dh = cond.shape[1]
    out = _fcnn(net, cond, T).reshape(-1, dh, 3 * K - 1)
    W = T(2) * T(tail) * _softmax(out[..., :K], T)
    H = T(2) * T(tail) * _softmax(out[..., K:2 * K], T)
    D = _softplus(out[..., 2 * K:], T)
    y, ld, b, w, h = _rqs(np.ascontiguousarray(trans).reshape(-1), W.reshape(-1, K), H.reshape(-1, K), D.reshape(-1, K - 1), inverse, -tail, tail,
                          -tail, tail, T)
    if details is not None:
        details.append(tuple(a.reshape(trans.shape) for a in (b, w, h, ld)))
    return y.reshape(trans.shape), ld.reshape(trans.shape)


def nsc_layer(params, x, K, tail, inverse=False, dtype=np.float64, details=None):
    """NeuralSplineCoupling.direct_fun / inverse_fun: params = (f1, f2), x [B][dim] -> y [B][dim], logdet [B].  `details`, a list,
    receives (bin, width, height, logabsdet) [B][dh] of the two half-steps in the order they run."""
    T = np.dtype(dtype).type
    x = np.asarray(x).astype(T)
    dh = x.shape[1] // 2
    lower, upper = x[:, :dh], x[:, dh:]
    f1, f2 = params
    if not inverse:
        upper, l1 = nsc_half(f1, lower, upper, K, tail, False, T, details)
        lower, l2 = nsc_half(f2, upper, lower, K, tail, False, T, details)
    else:
        lower, l1 = nsc_half(f2, upper, lower, K, tail, True, T, details)
        upper, l2 = nsc_half(f1, lower, upper, K, tail, True, T, details)
    return np.concatenate([lower, upper], 1), (l1.sum(1) + l2.sum(1)).astype(T, copy=False)


def nsc_stack(layers, x, K, tail, reverse, inverse=False, dtype=np.float64, details=None):
    """Serial((NeuralSplineCoupling [, Reverse]) x L): layers = [(f1, f2), ...] -> z [B][dim], logdet [B] (of the map applied)."""
    T = np.dtype(dtype).type
    z = np.asarray(x).astype(T)
    ld = np.zeros(len(z), T)
    for p in (layers[::-1] if inverse else layers):
        if inverse and reverse:
            z = z[:, ::-1]
        z, l = nsc_layer(p, z, K, tail, inverse, T, details)
        ld = ld + l
        if reverse and not inverse:
            z = z[:, ::-1]
    return np.ascontiguousarray(z), ld


def flow_log_pdf(layers, x, K, tail, reverse, prior, offset=0.0, dtype=np.float64, details=None):
    """Flow(stack, Normal(offset) | Uniform()).log_pdf -> log_pdf [B], the returned sample [B][dim] (clipped to (0, 1) under Uniform)."""
    T = np.dtype(dtype).type
    z, ld = nsc_stack(layers, x, K, tail, reverse, False, T, details)
    if prior == "normal":
        zo = z + T(offset)
        return ld + (T(-0.5) * (T(np.log(2 * np.pi)) + zo * zo)).sum(1), z
    assert prior == "uniform"
    return ld, np.clip(z, T(0), T(1))


# ---------------------------------------------------------------- inputs shared by the host test and the GPU test

def normal_params(N, K, n_deriv, seed, width=1.0):
    g = np.random.default_rng(seed)
    return tuple((width * g.normal(size=(N, c))).astype(np.float32) for c in (K, K, n_deriv))


def hard_params(N, K, n_deriv, seed):
    """Parameters three times wider than standard normal, and from the front three groups of 16 saturated rows each (so that each kind meets
    several bins and positions): a single entry of +60 among zeros in uw and in uh (every other bin at its 1e-3 minimum), all entries equal,
    derivatives of +-30 (both soft-plus branches: the x > 20 shortcut and exp(-30)).  No more than 16: the inverse through a flat bin
    (delta ~ 2e-3) next to a knot derivative of 30 is where the fp32 formula itself breaks -- its root comes out a few 1e-5 below 0 and the
    log-det's denominator turns negative, NaN in the C oracle and in NumPy fp32 alike at about one such element in 2500 -- so the host test
    checks that the fp32 reference is finite on exactly the sets the GPU test uses (hard_case over HARD_K)."""
    uw, uh, ud = normal_params(N, K, n_deriv, seed, 3.0)
    R = min(16, N // 8)
    i = np.arange(R)
    uw[:R] = 0.0
    uh[:R] = 0.0
    uw[i, i % K] = 60.0
    uh[i, (7 * i + 3) % K] = 60.0
    uw[R:2 * R] = 0.7
    uh[R:2 * R] = -1.3
    sign = np.where((np.arange(n_deriv)[None, :] + i[:, None]) % 2 == 0, 30.0, -30.0).astype(np.float32)
    ud[2 * R:3 * R] = sign
    return uw, uh, ud


def uniform_inputs(N, lo, hi, seed, unconstrained):
    """x (y for the inverse) uniform over the range; for the unconstrained form 10 % beyond the tails, and in the first elements: exactly
    +-tail, their fp32 neighbours outside, 0, NaN, +-inf (as many as fit)."""
    g = np.random.default_rng(seed)
    lo, hi = np.float32(lo), np.float32(hi)
    if not unconstrained:
        return g.uniform(lo, hi, size=N).astype(np.float32).clip(lo, hi)
    x = g.uniform(1.1 * lo, 1.1 * hi, size=N).astype(np.float32)
    special = np.array([lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)), 0.0, np.nan, np.inf, -np.inf],
                       np.float32)
    x[:min(N, special.size)] = special[:N]
    return x


HARD_K, HARD_N = (4, 8, 16, 32, 6, 40), 4099


def case(K, N, unconstrained, seed, hard=False):
    """-> x, uw, uh, ud, lo, hi: RQS on [0, 1], unconstrained_RQS with tails +-3."""
    nd = K - 1 if unconstrained else K + 1
    lo, hi = (-3.0, 3.0) if unconstrained else (0.0, 1.0)
    uw, uh, ud = hard_params(N, K, nd, seed) if hard else normal_params(N, K, nd, seed)
    return uniform_inputs(N, lo, hi, seed + 1, unconstrained), uw, uh, ud, lo, hi


def hard_case(K, unconstrained, inverse):
    """The hard set of the GPU test (and of the host test's check of the fp32 reference on it)."""
    return case(K, HARD_N, unconstrained, 7000 + K + 500 * int(inverse), hard=True)


def knot_inputs(K, tail, seed):
    """Equal unnormalised widths AND heights (K a power of two: the soft-max is exactly 1 / K, every knot -tail + 2 tail i / K is an exact fp32
    number when tail is one too), x on every knot and on its +-1..4 ulp neighbours, derivatives random and three times wider."""
    knots = (-tail + 2.0 * tail * np.arange(K + 1) / K).astype(np.float32)
    pts, up, dn = [knots], knots, knots
    for _ in range(4):
        up = np.nextafter(up, np.float32(np.inf))
        dn = np.nextafter(dn, np.float32(-np.inf))
        pts += [up, dn]
    x = np.concatenate(pts)
    N = x.size
    ud = (3.0 * np.random.default_rng(seed).normal(size=(N, K - 1))).astype(np.float32)
    return x, np.zeros((N, K), np.float32), np.zeros((N, K), np.float32), ud, np.arange(K + 1)
