"""33 .. 64 spline bases per dimension beyond four particles (D = 5 .. 8, e.g. `num_knots = 33` of examples/run_vqmc.py on the
8-electron chain): construction, log_pdf / psi against the oracle, the local energy and the parameter gradients against
oracle/energy_torch.py (fp64), the inverse and the samplers, and training steps eager and captured.  These models take the scalar
kernel for large batches (the MFMA kernel is not built for them), the wave kernels for small ones and R3 for the second-order
sweeps; WF_WIDE_RF selects the RF forms there for A/B comparisons."""
import numpy as np
import pytest

import oracle
from conftest import sorted_walkers

pytestmark = pytest.mark.gpu


def wide(D, box="mean", kn=33, k=6, layers=2, L=10.0, seed=7, pkn=None):
    from waveflow_amd import model_factory
    pkn = kn if pkn is None else pkn
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=pkn, n_i_internal_knots=kn,
                                                i_spline_reg=0.05, i_spline_reverse_fun_tol=1e-6, n_flow_layers=layers, box_size=L,
                                                xu_coord_type=box)
    params, psi, log_pdf, sample = init_fun(seed, D)
    psi.model.ensure_params(params)
    return params, psi, log_pdf, sample


def oracle_of(D, box="mean", kn=33, k=6, layers=2, L=10.0, pkn=None):
    constr = tuple(range(0, D - 1)) if box == "mean" else tuple(range(1, D))
    return oracle.Model(D=D, n_layers=layers, box=box, box_L=L, i_k=k, i_knots=kn, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                        prior="waveflow", p_k=k, p_knots=kn if pkn is None else pkn, p_left={0: 0}, p_right={0: 0}, constr_left=constr)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("D", [5, 6, 7, 8])
def test_wide_models_build(D):
    """33 knots at k = 6 (39 I-bases, 38 B-bases) for D = 5 .. 8; the MFMA kernel refuses these shapes loudly, auto evaluates anyway."""
    from waveflow_amd._lib import WfError
    params, psi, log_pdf, _ = wide(D)
    m = psi.model
    assert (m.i_nb, m.p_nb) == (39, 38)
    with pytest.raises(WfError) as e:
        m.set_kernel("mfma")
    assert e.value.status == -2
    m.set_kernel("auto")
    x = sorted_walkers(300, D, 10.0, 5)
    assert np.isfinite(log_pdf(params, x)).all()


@pytest.mark.parametrize("D", [5, 8])
def test_exactly_64_bases_and_one_more(D):
    """n_internal_knots = 64 - k gives 64 I-spline bases (the widest padded row; the B prior takes 34 knots: an even basis count, ortho_splines.py); one more basis stays
    WF_ERR_UNSUPPORTED."""
    from waveflow_amd._lib import WfError
    k = 5
    params, psi, log_pdf, _ = wide(D, kn=64 - k, k=k, layers=1, pkn=34)
    assert psi.model.i_nb == 64
    x = sorted_walkers(4099, D, 10.0, 6)
    om = oracle_of(D, kn=64 - k, k=k, layers=1, pkn=34)
    from waveflow_amd import flatten_params
    flat = flatten_params(params)
    from test_gpu_parity import as_accurate_as_fp32_reference
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True))
    with pytest.raises(WfError) as e:
        wide(D, kn=65 - k, k=k, layers=1, pkn=34)
    assert e.value.status == -2


@pytest.mark.parametrize("D,box", [(5, "mean"), (5, "first"), (8, "mean"), (8, "first")])
def test_log_pdf_and_psi_vs_oracle(D, box):
    """Ragged batches (wave kernel up to 6144 walkers), one batch of 2^17 (scalar kernel; the oracle on every 64th walker), the scalar
    kernel on a small batch too; psi_antisym on unsorted walkers; launch-to-launch reproducibility."""
    import torch
    from test_gpu_parity import as_accurate_as_fp32_reference
    from waveflow_amd import flatten_params
    params, psi, log_pdf, _ = wide(D, box=box)
    m = psi.model
    flat = flatten_params(params)
    om = oracle_of(D, box=box)
    for B in (1, 63, 257, 4099):
        x = sorted_walkers(B, D, 10.0, 100 + B)
        lp, ps = log_pdf(params, x), psi(params, x)
        pst = om.psi(flat, x, threads=8, f64=True)
        as_accurate_as_fp32_reference(lp, om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True), what=f"D={D} B={B}")
        as_accurate_as_fp32_reference(ps, om.psi(flat, x, threads=8), pst, atol=1e-6 * np.abs(pst).max(), what=f"psi D={D} B={B}")
    m.set_kernel("scalar")
    x = sorted_walkers(4099, D, 10.0, 77)
    as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True), what="scalar")
    m.set_kernel("auto")
    B = 1 << 17
    xn = sorted_walkers(B, D, 10.0, 4321)
    x = torch.from_numpy(xn).cuda()
    lp = log_pdf(params, x)
    assert torch.equal(log_pdf(params, x), lp)
    sel = np.arange(0, B, 64)
    as_accurate_as_fp32_reference(lp[torch.from_numpy(sel).cuda()].cpu().numpy(), om.log_pdf(flat, xn[sel], threads=8),
                                  om.log_pdf(flat, xn[sel], threads=8, f64=True), what=f"D={D} 2^17 sample")
    # psi_antisym: psi(sort(x)) (-1)^inversions on walkers in any particle order
    g = np.random.default_rng(3)
    xu = g.uniform(-10.0, 10.0, size=(3000, D)).astype(np.float32)
    pa, inv = m.psi_antisym(xu, return_inversions=True)
    want = psi(params, np.sort(xu, axis=1)) * (-1.0) ** np.asarray(inv)
    assert np.array_equal(np.asarray(pa), want.astype(np.float32))


def test_mflow_prior_with_64_row_bases():
    """The MFlow M-spline prior with 33 .. 64 bases at D = 6 against the oracle."""
    from test_gpu_parity import as_accurate_as_fp32_reference
    from waveflow_amd import flatten_params, flows, model_factory
    D = 6
    mt = model_factory.get_masked_transform
    init = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=40, spline_regularization=0.05,
                                                  reverse_fun_tol=1e-6), flows.Reverse()) * 2), mt(), spline_degree=3, n_internal_knots=40)
    params, log_pdf, _ = init(0, D)
    om = oracle.Model(D=D, n_layers=2, i_k=5, i_knots=40, i_reg=0.05, prior="mflow", p_k=3, p_knots=40)
    flat = flatten_params(params)
    g = np.random.default_rng(1)
    for B in (257, 20000):
        x = g.uniform(0.0, 1.0, size=(B, D)).astype(np.float32)
        as_accurate_as_fp32_reference(log_pdf(params, x), om.log_pdf(flat, x, threads=8), om.log_pdf(flat, x, threads=8, f64=True), what=f"mflow B={B}")


@pytest.mark.parametrize("D,B", [(5, 37), (8, 9)])
def test_local_energy_vs_autograd_oracle(D, B, monkeypatch):
    """H psi, psi and the Laplacian against energy_torch (fp64); the default sweep (R3 for these shapes), WF_ENERGY_R3 and the RF form
    (WF_WIDE_RF) agree."""
    import torch
    from oracle import energy_torch as et
    from waveflow_amd import flatten_params
    params, psi, log_pdf, _ = wide(D, L=5.0)
    m = psi.model
    flat = flatten_params(params)
    mo = et.TorchWaveflow(D, 2, "mean", 5.0, 6, 33, 0.05, tuple(range(0, D - 1)), dtype=torch.float64)
    x = sorted_walkers(B, D, 4.5, 21)
    protons = np.linspace(-3.0, 3.0, 4)
    ho, po, lo = et.hamiltonian(mo, flat, x.astype(np.float64), protons)
    res = {}
    for tag in ("default", "R3", "RF"):
        monkeypatch.delenv("WF_ENERGY_R3", raising=False)
        monkeypatch.delenv("WF_WIDE_RF", raising=False)
        if tag == "R3":
            monkeypatch.setenv("WF_ENERGY_R3", "1")
        if tag == "RF":
            monkeypatch.setenv("WF_WIDE_RF", "1")
        hp, ps, lap = res[tag] = m.hamiltonian(x, protons, return_psi=True, return_laplacian=True)
        np.testing.assert_allclose(ps, po, rtol=2e-4, atol=1e-6 * np.abs(po).max())
        np.testing.assert_allclose(lap, lo, rtol=0, atol=2e-3 * np.abs(lo).max())
        np.testing.assert_allclose(hp, ho, rtol=0, atol=2e-3 * np.abs(ho).max())
    for tag in ("R3", "RF"):
        for a, b in zip(res[tag], res["default"]):
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-3 * np.abs(b).max())
    # a larger batch: the two sweeps agree to rounding
    xl = sorted_walkers(3000, D, 5.0, 22)
    monkeypatch.delenv("WF_WIDE_RF")
    hd, pd, ld = m.hamiltonian(xl, protons, return_psi=True, return_laplacian=True)
    monkeypatch.setenv("WF_WIDE_RF", "1")
    hf, pf, lf = m.hamiltonian(xl, protons, return_psi=True, return_laplacian=True)
    assert np.isfinite(hd).all() and np.array_equal(pd, pf)
    assert np.linalg.norm(lf - ld) <= 1e-4 * np.linalg.norm(ld) and np.linalg.norm(hf - hd) <= 1e-4 * np.linalg.norm(hd)


@pytest.mark.parametrize("D,box,B", [(5, "first", 6), (6, "mean", 17), (8, "mean", 9)])
def test_gradients_vs_autograd_oracle(D, box, B, monkeypatch):
    """psi_vjp (first and second order), logpdf_vjp and vqmc_loss_grad against energy_torch; the default ring (R3 for these shapes),
    WF_GRAD_R3 and the RF form (WF_WIDE_RF, read at model creation) agree."""
    import torch
    from oracle import energy_torch as et
    from waveflow_amd import flatten_params
    constr = tuple(range(0, D - 1)) if box == "mean" else tuple(range(1, D))
    mo = et.TorchWaveflow(D, 2, box, 5.0, 6, 33, 0.05, constr, dtype=torch.float64)
    x = sorted_walkers(B, D, 4.5, 21)
    g = np.random.default_rng(8)
    wp, wl, w = (g.normal(size=B).astype(np.float32) for _ in range(3))
    protons = np.linspace(-3.0, 3.0, 4)
    out = {}
    for tag in ("default", "R3", "RF"):
        monkeypatch.delenv("WF_GRAD_R3", raising=False)
        monkeypatch.delenv("WF_WIDE_RF", raising=False)
        if tag == "R3":
            monkeypatch.setenv("WF_GRAD_R3", "1")
        if tag == "RF":
            monkeypatch.setenv("WF_WIDE_RF", "1")
        params, psi, log_pdf, _ = wide(D, box=box, L=5.0)
        m = psi.model
        flat = flatten_params(params)
        o = out[tag] = {}
        o["psi"] = m.psi_vjp(x, wp, wl).cpu().numpy().astype(np.float64)
        o["psi1"] = m.psi_vjp(x, wp, np.zeros_like(wl)).cpu().numpy().astype(np.float64)
        o["lp"] = m.logpdf_vjp(x, w).cpu().numpy().astype(np.float64)
        o["loss"] = m.vqmc_loss_grad(x, protons, running_average=-1.0)[1].cpu().numpy().astype(np.float64)
        del m, psi, log_pdf
    monkeypatch.delenv("WF_WIDE_RF", raising=False)
    want = {"psi": et.psi_vjp(mo, flat, x.astype(np.float64), wp, wl), "psi1": et.psi_vjp(mo, flat, x.astype(np.float64), wp, np.zeros_like(wl)),
            "lp": et.logpdf_vjp(mo, flat, x.astype(np.float64), w), "loss": et.vqmc_loss_grad(mo, flat, x.astype(np.float64), protons, -1.0)[1]}
    for tag in out:
        for k in want:
            assert rel_l2(out[tag][k], want[k]) < 3e-3, (tag, k, rel_l2(out[tag][k], want[k]))
    for k in want:
        assert np.array_equal(out["R3"][k], out["default"][k]), k                  # the default IS R3 for these shapes
        assert rel_l2(out["RF"][k], out["default"][k]) < 1e-4, (k, rel_l2(out["RF"][k], out["default"][k]))


@pytest.mark.parametrize("D", [5, 8])
def test_inverse_round_trip(D, monkeypatch):
    """exact inverse: inverse(direct(x)) = x and direct(inverse(u)) = u in both kernels (wave / one lane per walker), sorted walkers inside
    the box; both kernels agree, exact or not (made.py:88).  The mean-type box reverse of D >= 7 is ill-conditioned for a few walkers in
    1000 at any basis count (the same rows at 23 knots): the round trip is checked on the 99th percentile, the kernels against each other."""
    params, psi, log_pdf, _ = wide(D, L=7.0)
    m = psi.model
    x = sorted_walkers(5000, D, 6.5, 31)
    u, _ = m.flow(x)
    u = np.asarray(u)
    u_in = np.random.default_rng(0).uniform(0.02, 0.98, size=(5000, D)).astype(np.float32)
    res = {}
    for limit in ("100000000", "0"):                                          # wave kernel, one-lane kernel
        monkeypatch.setenv("WF_WAVE_SAMPLE_MAX", limit)
        xe = m.inverse(u, exact=True)
        assert np.quantile(np.abs(xe - x).max(1), 0.99) < 2e-3, (limit, np.abs(xe - x).max())
        xi = m.inverse(u_in, exact=True)
        assert np.all(np.diff(xi, axis=1) >= 0) and np.abs(xi).max() <= 7.0
        u2, _ = m.flow(xi)
        e = np.abs(np.asarray(u2) - u_in).max(1)
        assert np.median(e) < 3e-5 and np.quantile(e, 0.99) < 1e-2, (limit, np.quantile(e, 0.99), e.max())
        res[limit] = (xi, m.inverse(u, exact=False))
    for a, b in zip(res["0"], res["100000000"]):
        d = np.abs(a - b)
        assert np.median(d) < 1e-6 and np.quantile(d, 0.999) < 2e-4 and d.max() < 2e-3, (np.median(d), d.max())


@pytest.mark.parametrize("D", [5, 8])
def test_sampler_on_both_sides_of_the_switch(D, monkeypatch):
    """2^17 draws from the wave sampler (<= WF_WAVE_SAMPLE_MAX) and from the one-lane sampler: sorted, finite, inside the box; the two
    kernels' marginals agree (two-sample Kolmogorov-Smirnov).  (Importance-weighted uniform walkers are no reference here: 2^20 of them
    carry ~200 effective samples at D = 5 and ~2 at D = 8.)"""
    from scipy import stats
    params, psi, log_pdf, _ = wide(D, L=5.0)
    m = psi.model
    N = 1 << 17
    for exact in (True, False):
        draws = {}
        for limit in ("131072", "0"):
            monkeypatch.setenv("WF_WAVE_SAMPLE_MAX", limit)
            xs = draws[limit] = m.sample(11 + D + (limit == "0"), N, exact=exact).cpu().numpy()
            assert np.isfinite(xs).all() and np.all(np.diff(xs, axis=1) >= 0) and np.abs(xs).max() <= 5.0
        for c in range(D):
            p = stats.ks_2samp(draws["131072"][:, c], draws["0"][:, c]).pvalue
            assert p > 1e-4, (exact, c, p)


def _chain(kn):
    from waveflow_amd import vqmc
    psi, log_pdf, sample, st, opt_update, get_params = vqmc.create_train_state(10.0, 1e-3, n_particle=8, num_knots=kn)
    return psi, get_params(st)


def test_training_steps_on_the_8_electron_chain():
    """num_knots = 33 on the 8-electron chain: fused training steps keep the loss finite; loss + gradient + Adam + refill captured in a
    hipGraph reproduce the eager steps bit for bit; the fused step replayed from a graph equals the same step issued eagerly."""
    import torch
    from waveflow_amd import flatten_params
    psi, params = _chain(33)
    m = psi.model
    assert (m.i_nb, m.p_nb) == (39, 38)
    flat = flatten_params(params)
    protons = np.linspace(-3.5, 3.5, 8)
    x = torch.as_tensor(sorted_walkers(256, 8, 6.0, 13)).cuda()

    def fresh():
        xs = torch.as_tensor(flat).cuda()
        return xs, torch.zeros_like(xs), torch.zeros_like(xs)

    def step(xs, mm, vv, i):
        m.set_params_device(xs)
        sums, grad = m.vqmc_loss_grad(x, protons, -2.0)
        m.adam_step(xs, grad, mm, vv, i, 1e-3)
        return sums

    xe, me, ve = fresh()
    se = [step(xe, me, ve, i).clone() for i in range(3)]
    torch.cuda.synchronize()
    xg, mg, vg = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(xg, mg, vg, 0)
        xg.copy_(torch.as_tensor(flat)); mg.zero_(); vg.zero_()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            sg = [step(xg, mg, vg, i).clone() for i in range(3)]
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(xg.cpu().numpy(), xe.cpu().numpy())
    for a_, b_ in zip(sg, se):
        assert np.array_equal(a_.cpu().numpy(), b_.cpu().numpy())
    assert np.abs(xg.cpu().numpy() - flat).max() > 1e-4
    # the fused step (sampler -> loss + gradient -> Adam -> refill): a few eager steps, then the same two steps from a graph
    seed, Bt, lr = 5, 256, 1e-3
    xa, ma, va = fresh()
    st = m.make_train_state(xa, ma, va, 0, ring_len=8)
    m.set_params_device(xa)
    for _ in range(4):
        m.train_step(st, seed, Bt, protons, lr, exact_sampler=True)
    torch.cuda.synchronize()
    ring = st["ring"].cpu().numpy()[:4]
    assert int(st["counter"].item()) == 4 and np.isfinite(ring).all() and (ring[:, 2] == Bt).all()
    assert np.isfinite(xa.cpu().numpy()).all()
    x1, m1, v1 = fresh()
    s1 = m.make_train_state(x1, m1, v1, 0, ring_len=8)
    m.set_params_device(x1)
    m.train_step(s1, seed, Bt, protons, lr, exact_sampler=True)
    m.train_step(s1, seed, Bt, protons, lr, exact_sampler=True)
    torch.cuda.synchronize()
    x2, m2, v2 = fresh()
    s2 = m.make_train_state(x2, m2, v2, 0, ring_len=8)
    with torch.cuda.stream(side):
        m.train_step(s2, seed, Bt, protons, lr, exact_sampler=True)       # warm-up: workspace allocation
        x2.copy_(torch.as_tensor(flat)); m2.zero_(); v2.zero_(); s2["counter"].zero_(); s2["ring"].zero_()
        m.set_params_device(x2)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            m.train_step(s2, seed, Bt, protons, lr, exact_sampler=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(x2.cpu().numpy(), x1.cpu().numpy())
    assert np.array_equal(s2["ring"].cpu().numpy(), s1["ring"].cpu().numpy())
