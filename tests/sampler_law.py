"""The law of the samplers' draws (helpers, no tests): case table, fp64 Rosenblatt transform, statistics, a host restatement of the reference's
rejection sampler with planted defects.

wf_sample draws the latent point column by column, column d from the conditional density p_d(. | lat[<d]) that the oracle restates
(oracle.Model.prior_column_density).  With F_d the normalised cumulative of that density (oracle.Model.prior_rosenblatt: closed form on the mesh
intervals, fp64), v[b, d] = F_d(lat[b, d] | lat[b, <d]) is i.i.d. uniform on the unit cube, across columns and walkers, exactly when the law is right.
The statistics below test that: Kolmogorov-Smirnov per column, a chi-square of the 8 x 8 histogram of every pair of columns, and one of neighbouring
walkers.  tests/test_sampler_law_host.py shows on a CPU that they accept a correct sampler and reject four planted defects at the sizes the GPU
tests use; tests/test_gpu_sampler_law.py applies them to the kernels' draws."""
import functools
import os

import numpy as np

import oracle

P_MIN = 1e-6          # every statistic's p-value must exceed it: fewer than 1000 statistics on fixed seeds => a correct sampler fails with p < 1e-3, reproducibly
N0 = 1 << 19          # walkers of the column-0 test (column 0 does not depend on the walker: one cumulative table)
H = 64


def threads():
    return max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16"))))


# name -> oracle description, seed of the parameters, factors on the prior net's output layer (weights, bias), walkers of the conditional-column tests.  The factors are fixed here and checked for power in tests/test_sampler_law_host.py (freshly initialised nets
# give nearly flat conditionals, which test nothing): column 1's conditional CDFs at lat0 = 0.2 and 0.8 differ by >= 0.1 in sup-distance, the acceptance
# rate 1 / ymax lies in [0.05, 0.6]; every scaled weight stays far below the fp16 range guard of the matrix-core images (|W| < 1e4).
_WF = dict(prior="waveflow", i_left={0: 0}, i_right={0: 1})
CASES = {
    # (He: the checkpoint's two columns -- relative and centre-of-mass coordinate -- have densities so unlike each other that column 1 rarely accepts the
    # proposal column 0 accepted: planted defect "d" shows at p = 0.1 with 16 384 walkers, 4e-5 with 2^18 and 2e-17 with 2^19, hence 2^19)
    "he": dict(om=None, N=1 << 19),
    "two_row_blocks": dict(om=dict(D=2, n_layers=2, box="mean", box_L=10.0, i_k=6, i_knots=33, i_reg=0.05, p_k=6, p_knots=33, constr_left=(0,), **_WF),
                           seed=1, scale=(2.0, 1.0), N=16384),
    "envelope_k8": dict(om=dict(D=2, n_layers=1, box="mean", box_L=3.0, i_k=5, i_knots=16, i_reg=0.05, p_k=8, p_knots=15, constr_left=(0,), **_WF),
                        seed=6, scale=(3.0, 1.0), N=16384),
    "envelope_k1": dict(om=dict(D=2, n_layers=1, box="mean", box_L=3.0, i_k=5, i_knots=16, i_reg=0.05, p_k=1, p_knots=16, constr_left=(0,), **_WF),
                        seed=5, scale=(5.0, 1.0), N=16384),
    "d3_mean_box": dict(om=dict(D=3, n_layers=2, box="mean", box_L=7.0, i_k=5, i_knots=16, i_reg=0.05, p_k=5, p_knots=16, constr_left=(0, 1), **_WF),
                        seed=2, scale=(5.0, 1.0), N=16384),
    "d5": dict(om=dict(D=5, n_layers=2, box="mean", box_L=7.0, i_k=5, i_knots=16, i_reg=0.05, p_k=5, p_knots=16, constr_left=(0, 1, 2, 3), **_WF),
               seed=8, scale=(3.0, 1.0), N=8192),
    "d8": dict(om=dict(D=8, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=23, i_reg=0.05, p_k=6, p_knots=23, constr_left=tuple(range(7)), **_WF),
               seed=32, scale=(5.0, 1.0), N=8192),
    "first_box": dict(om=dict(D=3, n_layers=1, box="first", box_L=2.0, i_k=5, i_knots=16, i_reg=0.0, p_k=5, p_knots=16, constr_left=(1, 2), **_WF),
                      seed=9, scale=(5.0, 1.0), N=16384),
    "gated": dict(om=dict(D=3, n_layers=2, box="mean", box_L=3.0, i_k=6, i_knots=23, i_reg=0.05, p_k=6, p_knots=23, constr_left=(0, 1), i_gate=True,
                          p_gate=True, **_WF), seed=4, scale=(10.0, 10.0), N=16384),
    "boundary_d2": dict(om=dict(D=2, n_layers=2, box="mean", box_L=3.0, i_k=6, i_knots=23, i_reg=0.05, p_k=6, p_knots=23, constr_left=(0,), prior="waveflow",
                                i_left={0: 0.0}, i_right={0: 1.0}, p_left={0: 0.2, 1: 8.0}, p_right={0: -0.1, 1: -5.0}), seed=3, scale=(2.0, 1.0), N=16384),
    "boundary_d3": dict(om=dict(D=3, n_layers=2, box="mean", box_L=3.0, i_k=6, i_knots=23, i_reg=0.05, p_k=6, p_knots=23, constr_left=(0, 1), prior="waveflow",
                                i_left={0: 0.0}, i_right={0: 1.0}, p_left={0: 0.2, 1: 8.0}, p_right={0: -0.1, 1: -5.0}), seed=5, scale=(2.0, 1.0), N=16384),
    "mflow": dict(om=dict(D=2, n_layers=2, i_k=5, i_knots=9, i_reg=0.05, prior="mflow", p_k=3, p_knots=15), seed=2, scale=(20.0, 20.0), N=16384),
    "flow_normal": dict(om=dict(D=2, n_layers=2, layer_kind="made", prior="normal", normal_offset=-0.5), seed=3, scale=None, N=16384),
}
WITH_PRIOR_NET = [n for n in CASES if n != "flow_normal"]


@functools.lru_cache(None)
def oracle_model(name):
    return oracle.he_model(10.0) if name == "he" else oracle.Model(**CASES[name]["om"])


def he_flat():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "he_checkpoint.npz"))["flat"]


@functools.lru_cache(None)
def flat_params(name):
    """The parameter vector of a case, shared by the host and the GPU tests: the He checkpoint, or the oracle's seeded initialisation with the prior
    net's output layer scaled by the case's fixed factors."""
    if name == "he":
        flat = he_flat().copy()
    else:
        om, c = oracle_model(name), CASES[name]
        flat = om.init_params(c["seed"])
        if c["scale"] is not None:
            D, nb = om.D, om.p_nb
            w2 = om.n_layers * om.layer_param_count() + D * H + H + H * H + H
            b2 = w2 + H * nb * D
            flat[w2:b2] *= c["scale"][0]
            flat[b2:b2 + nb * D] *= c["scale"][1]
    flat.setflags(write=False)
    return flat


def device_model(name):
    """The device model of a case with the case's parameters uploaded (GPU tests only)."""
    from waveflow_amd import flows, model_factory, wavefunctions
    mt = model_factory.get_masked_transform
    o = CASES[name]["om"]
    if name == "he":
        init = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23, i_spline_reg=0.05,
                                                i_spline_reverse_fun_tol=1e-6, n_flow_layers=3, box_size=10, xu_coord_type="mean")
        model = init(0, 2)[2].model
    elif name == "mflow":
        init = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=o["i_k"], n_internal_knots=o["i_knots"], spline_regularization=o["i_reg"],
                                                      reverse_fun_tol=1e-6), flows.Reverse()) * o["n_layers"]), mt(), spline_degree=o["p_k"], n_internal_knots=o["p_knots"])
        model = init(0, o["D"])[1].model
    elif name == "flow_normal":
        init = flows.Flow(flows.Serial(*(flows.MADE(mt(return_simple_masked_transform=True)), flows.Reverse()) * o["n_layers"]), flows.Normal(o["normal_offset"]))
        model = init(0, o["D"])[1].model
    else:
        gate = bool(o.get("i_gate"))
        init = wavefunctions.Waveflow(
            flows.Serial(flows.BoxTransformLayer(o["box_L"], o["box"]),
                         *(flows.IMADE(mt(), o["i_k"], o["i_knots"], o["i_reg"], 1e-6, o["i_left"], o["i_right"], set_nn_output_grad_to_zero=gate), flows.Reverse()) * o["n_layers"]),
            mt(allow_negative_params=True), o["p_k"], o["p_knots"], constraints_dict_left=o.get("p_left", {0: 0}), constraints_dict_right=o.get("p_right", {0: 0}),
            constrained_dimension_indices_left=list(o["constr_left"]), set_nn_output_grad_to_zero=bool(o.get("p_gate")))
        model = init(0, o["D"])[1].model
    flat = flat_params(name)
    om = oracle_model(name)
    assert flat.size == om.n_params() == model.n_params, (name, flat.size, model.n_params)
    assert name == "flow_normal" or (model.i_nb, model.p_nb) == (om.i_nb, om.p_nb), (name, model.i_nb, model.p_nb, om.i_nb, om.p_nb)
    model.set_params(np.array(flat))
    return model


# ---------------------------------------------------------------- the reference transform
def rosenblatt(name, lat, ncol=None):
    """v [B, ncol] in fp64 (and Z): the oracle's transform; Normal prior: v = Phi(lat), Z = 1."""
    lat = np.asarray(lat, np.float32)
    if name == "flow_normal":
        from scipy import special
        v = special.ndtr(lat.astype(np.float64))
        v = v if ncol is None else v[:, :ncol]
        return v, np.ones_like(v)
    return oracle_model(name).prior_rosenblatt(flat_params(name), lat, threads=threads(), ncol=ncol)


# ---------------------------------------------------------------- statistics
def _chi2_8x8(a, b):
    from scipy import stats
    ia, ib = np.minimum((np.asarray(a) * 8).astype(np.int64), 7), np.minimum((np.asarray(b) * 8).astype(np.int64), 7)
    counts = np.bincount(ia * 8 + ib, minlength=64)
    return float(stats.chisquare(counts).pvalue)        # expected: uniform on the 64 cells (uniform margins and independence at once), 63 degrees of freedom


def uniform_statistics(v):
    """p-values of the statistics of v [B, n] ~ i.i.d. uniform on the unit cube: {label: p}.
      ks[d]        Kolmogorov-Smirnov of column d against the uniform law;
      pair[d,e]    chi-square of the 8 x 8 histogram of (v[:, d], v[:, e]), d < e: independence of the columns;
      next[d]/[d]' chi-square of the 8 x 8 histogram of (v[b, d], v[b + 1, d]) over the disjoint pairs starting at even / odd b: independence of
                   neighbouring walkers' streams (disjoint pairs, so that the cells' counts are multinomial and the statistic is chi-square)."""
    from scipy import stats
    v = np.asarray(v, np.float64)
    if v.ndim == 1:
        v = v[:, None]
    assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0
    B, n = v.shape
    out = {}
    for d in range(n):
        out[f"ks[{d}]"] = float(stats.kstest(v[:, d], "uniform").pvalue)
        for e in range(d + 1, n):
            out[f"pair[{d},{e}]"] = _chi2_8x8(v[:, d], v[:, e])
        for off, tag in ((0, ""), (1, "'")):
            m = (B - off) // 2
            out[f"next[{d}]{tag}"] = _chi2_8x8(v[off:off + 2 * m:2, d], v[off + 1:off + 2 * m:2, d])
    return out


def smallest(stats_dict):
    k = min(stats_dict, key=stats_dict.get)
    return k, stats_dict[k]


def assert_uniform(v, what):
    """Every statistic of uniform_statistics(v) has p > P_MIN; prints and returns the smallest."""
    st = uniform_statistics(v)
    k, p = smallest(st)
    print(f"[sampler law] {what}: n={len(v)}, {len(st)} statistics, smallest p = {p:.3g} ({k})")
    bad = {a: b for a, b in st.items() if not b > P_MIN}
    assert not bad, (what, bad)
    return p


# ---------------------------------------------------------------- host restatement of the rejection sampler, with planted defects
def _spline_values(om, coef, x):
    """sum_j coef[b, j] X_cached(x[b], j): linear interpolation of the prior table between mesh points (fp64 accumulation)."""
    tab = om.p_tab[0]
    n = tab.shape[1]
    xs = x.astype(np.float64) * (n - 1)
    q = np.clip(np.floor(xs).astype(np.int64), 0, n - 2)
    t = xs - q
    fl = np.einsum("bj,jb->b", coef, tab[:, q].astype(np.float64))
    fr = np.einsum("bj,jb->b", coef, tab[:, q + 1].astype(np.float64))
    return fl + (fr - fl) * t


def host_sampler(name, n, seed, defect=None):
    """NumPy restatement of the reference's rejection sampler (wavefunctions.py:74-107 / bsplines_jax.py:144-171): column by column, proposals uniform on
    [0, 1) x [0, ymax) under the oracle's bound, accepted where y < density -- lat [n, D] fp32.  Walker b's proposal `it` of column `col` comes from a
    stream of its own, (seed, col, it)[b].  defect plants one of
      "a"  column d drawn with the conditioning columns set to zero,
      "b"  acceptance against min(density, 0.7 bound): a bound below the density.  The oracle's global ymax (the largest squared B coefficient) lies so far
           above most of these densities that 0.7 ymax is still a valid bound and changes no draw; the planted bound is therefore 0.7 x the sharpest
           bound a sampler may use, the density's own maximum (what a piecewise envelope approaches), which never exceeds 0.7 ymax,
      "c"  a piecewise-constant envelope (the density's maximum on each knot interval) with proposals uniform on [0, 1) instead of weighted by the
           intervals' bounds: the law becomes density / bound,
      "d"  column 1's proposals reuse column 0's random numbers."""
    om, flat = oracle_model(name), flat_params(name)
    D, wavefn = om.D, om.c.prior_kind == 0
    lat = np.zeros((n, D), np.float32)
    nint = om.c.psp.nb - om.c.psp.k + (2 if wavefn else 3)     # knot intervals: internal knots + 1
    for col in range(D):
        cond = np.zeros_like(lat) if defect == "a" else lat
        coef, ymax = om.prior_column_coeffs(flat, cond, col, threads=threads())
        if defect in ("b", "c"):
            grid = np.linspace(0.0, 1.0, 16 * nint + 1)
            basis = np.stack([_spline_values(om, np.eye(om.p_nb), np.full(om.p_nb, g)) for g in grid], 1)      # [nb, grid]
            peak, cell = np.zeros(n), np.zeros((n, nint))
            for lo in range(0, n, 32768):
                dens_grid = coef[lo:lo + 32768] @ basis
                dens_grid = dens_grid ** 2 if wavefn else dens_grid
                peak[lo:lo + 32768] = np.minimum(dens_grid.max(1), ymax[lo:lo + 32768])
                cell[lo:lo + 32768] = np.maximum(dens_grid[:, :-1], dens_grid[:, 1:]).reshape(-1, nint, 16).max(-1) * 1.02      # (bound per knot interval)
        pending = np.arange(n)
        src = 0 if (defect == "d" and col == 1) else col
        for it in range(100000):
            if not pending.size:
                break
            g = np.random.default_rng([seed, src, it])
            xc, yc = g.random(n, dtype=np.float32)[pending], g.random(n, dtype=np.float32)[pending].astype(np.float64)
            f = _spline_values(om, coef[pending], xc)
            dens = f * f if wavefn else f
            if defect == "c":
                bound = cell[pending, np.minimum((xc.astype(np.float64) * nint).astype(np.int64), nint - 1)]
            else:
                bound = ymax[pending]
            if defect == "b":
                dens = np.minimum(dens, 0.7 * peak[pending])
            ok = yc * bound < dens
            lat[pending[ok], col] = xc[ok]
            pending = pending[~ok]
        assert not pending.size
    return lat
