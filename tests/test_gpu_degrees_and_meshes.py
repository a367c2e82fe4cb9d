"""The model kernels at spline degrees 1 .. 8 and at mesh sizes from 33 to 4001 points (the rest of the GPU suite evaluates models at degrees 3 .. 6 on
2000 mesh points): log_pdf / psi on the three forward kernels, the local energy on the wave and the matrix-core paths, the parameter gradients, the
inverse and the samplers on every kernel, and what wf_model_create refuses.  Every reference is the CPU oracle (oracle.Model in fp32 and fp64,
oracle/energy_torch.py) of the same model; the yardsticks are those of the tests named in each docstring.

What depends on these two numbers: the two-round mesh search of the wave-cooperative inverse (64 lanes x 32 points reach 2048 mesh points; beyond them
the first round takes a wider stride and a walk over the 32-point blocks of the interval found precedes the second), its masks on a coarse mesh, the 64-bin envelope
and the 12-row band windows of the staged sampler (I-spline band form: degrees <= 7), the support bounds of the table pieces, the vanishing third
derivative table of degrees 1 and 2, and the division by n_mesh - 1 of the matrix-core kernel."""
import numpy as np
import pytest

import oracle
from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

L = 10.0
LAYERS = 2
SEED = 17
# name -> (D, degree, internal knots, mesh points).  knots + degree is odd (the orthogonalised prior needs an even basis count: knots + degree - 1),
# and no mesh has fewer points than the prior has bases.
CASES = {
    "k1": (2, 1, 16, 2000),      # lowest degree: the derivative tables of order >= 2 vanish
    "k2": (2, 2, 13, 2000),      # third derivative table piecewise constant
    "k7": (2, 7, 12, 2000),      # last degree on the staged sampler's band-limited I-rows
    "k8": (2, 8, 9, 257),        # first degree off them; coarse mesh
    "k7w": (2, 7, 40, 257),      # 47 / 46 bases: two 32-row blocks at a high degree
    "m33": (2, 3, 10, 33),       # fewer mesh points than sampler bins and than coarse-search lanes
    "m2049": (2, 6, 23, 2049),   # first size beyond 64 x 32
    "m4001": (2, 6, 23, 4001),   # well beyond it
    "d3m": (3, 2, 13, 4001),     # D > 2 kernels on a large mesh
    "d3k8": (3, 8, 9, 257),      # D > 2 kernels at the top degree
}
ALL = list(CASES)
TWO = [n for n in ALL if CASES[n][0] == 2]
# (wf_dispatch.cpp: every case is a mean-type box over ungated IMADE layers with homogeneous constraints, three nets that stay resident in LDS and
# at most 64 (D = 2) / 32 (D >= 3) bases: all of them belong to the family of the matrix-core local energy (energy_tile2_capable_at /
# energy_dir_capable_at), the two-particle ones to that of the matrix-core gradient (grad_tile_capable_at) and of the staged sampler
# (tile_sample_capable_at: prior degree <= 8) -- a forced run is another kernel's bits in every test below)
_cache = {}


def build_device(name):
    """A fresh device model of case `name` (environment switches read at creation, e.g. WF_MFMA_NO_BAND, apply): (params, psi, log_pdf, sample)"""
    from waveflow_amd import flows, model_factory, wavefunctions
    D, k, kn, n_mesh = CASES[name]
    mt = model_factory.get_masked_transform
    init = wavefunctions.Waveflow(
        flows.Serial(flows.BoxTransformLayer(L, "mean"),
                     *(flows.IMADE(mt(), k, kn, 0.05, 1e-6, {0: 0}, {0: 1}, n_spline_base_mesh_points=n_mesh), flows.Reverse()) * LAYERS),
        mt(allow_negative_params=True), k, kn, constraints_dict_left={0: 0}, constraints_dict_right={0: 0},
        constrained_dimension_indices_left=list(range(D - 1)), set_nn_output_grad_to_zero=False, n_spline_base_mesh_points=n_mesh)
    params, psi, log_pdf, sample = init(SEED, D)
    psi.model.ensure_params(params)
    return params, psi, log_pdf, sample


def case(name):
    """One device model, one CPU oracle and the references computed so far per case, shared by the tests of the module."""
    if name not in _cache:
        from waveflow_amd import flatten_params
        D, k, kn, n_mesh = CASES[name]
        params, psi, log_pdf, sample = build_device(name)
        om = oracle.Model(D=D, n_layers=LAYERS, box="mean", box_L=L, i_k=k, i_knots=kn, i_reg=0.05, i_left={0: 0}, i_right={0: 1}, prior="waveflow",
                          p_k=k, p_knots=kn, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(D - 1)), n_mesh=n_mesh, reverse_tol=1e-6)
        assert (psi.model.i_nb, psi.model.p_nb) == (kn + k, kn + k - 1) == (om.i_nb, om.p_nb)
        _cache[name] = dict(params=params, psi=psi, log_pdf=log_pdf, m=psi.model, flat=flatten_params(params), om=om, ref={})
    c = _cache[name]
    c["m"].set_kernel("auto")
    c["m"].ensure_params(c["params"])
    return c


def ref(name, key, make):
    """A reference of case `name`, computed once and left unchanged"""
    r = case(name)["ref"]
    if key not in r:
        r[key] = make()
    return r[key]


def torch_model(name, dtype):
    from oracle import energy_torch as et
    D, k, kn, n_mesh = CASES[name]
    return ref(name, ("torch", str(dtype)), lambda: et.TorchWaveflow(D, LAYERS, "mean", L, k, kn, 0.05, tuple(range(D - 1)), dtype=dtype, n_mesh=n_mesh))


def set_kernel_or_skip(m, kernel):
    """Select a forward kernel; skip where the library says that this kind is not built for the shape (WF_ERR_UNSUPPORTED), fail on anything else"""
    from waveflow_amd import _lib
    try:
        m.set_kernel(kernel)
    except _lib.WfError as e:
        if e.status != -2:
            raise
        pytest.skip(str(e))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


# ------------------------------------------------------------------------------------------------ 1. forward

def _forward_refs(name):
    c = case(name)
    D = CASES[name][0]
    x = sorted_walkers(3000, D, L, 1234)

    def make():
        om, flat = c["om"], c["flat"]
        out = dict(x=x, lp32=om.log_pdf(flat, x, threads=8), lp64=om.log_pdf(flat, x, threads=8, f64=True), ps32=om.psi(flat, x, threads=8),
                   ps64=om.psi(flat, x, threads=8, f64=True))
        if D == 2:
            out["idx"] = om.log_pdf(flat, x[:512], return_u=True, return_idx=True)[2]
        return out
    return ref(name, "forward", make)


@pytest.mark.parametrize("kernel", ["scalar", "mfma", "wave"])
@pytest.mark.parametrize("name", ALL)
def test_log_pdf_and_psi_on_the_three_kernels_vs_oracle(name, kernel):
    """log_pdf and psi of 3000 uniform sorted walkers: as close to fp64 arithmetic as the fp32 oracle is (test_waveflow_other_shapes_vs_oracle).  Two
    particles: the mesh indices of 512 walkers against the oracle's return_idx -- bit for bit at every layer on the scalar kernel; on the matrix-core
    kernel bit for bit at layer 0, and behind it as test_end_to_end_bin_index_mismatch_rate bounds them (see the comment at the assertion)."""
    from test_gpu_parity import as_accurate_as_fp32_reference
    c, r = case(name), _forward_refs(name)
    D, k, kn, n_mesh = CASES[name]
    m, params = c["m"], c["params"]
    set_kernel_or_skip(m, kernel)
    try:
        x = r["x"]
        as_accurate_as_fp32_reference(c["log_pdf"](params, x), r["lp32"], r["lp64"], what=f"{name} {kernel} log_pdf")
        as_accurate_as_fp32_reference(c["psi"](params, x), r["ps32"], r["ps64"], atol=1e-6 * np.abs(r["ps64"]).max(), what=f"{name} {kernel} psi")
        if D == 2 and kernel != "wave":
            lp, u, idx = m.log_pdf(x[:512], return_sample=True, return_bin_idx=True)
            idx, idxo = np.asarray(idx), r["idx"]
            assert idx.shape == idxo.shape and idx.max() <= n_mesh - 1
            flips = (idx != idxo).any(axis=(2, 3)).sum(axis=0)
            print(f"[bin indices {name} {kernel}] walkers of 512 whose (floor, ceil) indices differ from the oracle's, per layer input: {flips.tolist()}")
            if kernel == "scalar":   # the oracle's operation order: every layer sees the oracle's inputs bit for bit
                assert np.array_equal(idx, idxo), flips
            else:
                # the matrix-core kernel rounds its layers in another order: layer 0 (bit-identical inputs) must give the oracle's indices; behind it
                # an input that differs in the last ulp flips an index where u (n_mesh - 1) sits on an integer -- by one mesh point, and within the
                # 5e-3 of test_end_to_end_bin_index_mismatch_rate (measured: one walker of 512 on k2 and on m2049, none elsewhere)
                assert np.array_equal(idx[:, 0], idxo[:, 0])
                assert np.abs(idx.astype(np.int64) - idxo).max() <= 1
                assert flips.max() / 512.0 < 5e-3, flips
    finally:
        m.set_kernel("auto")


@pytest.mark.parametrize("name", TWO)
def test_layer_bin_indices_bit_exact(name):
    """test_bin_indices_bit_exact_per_layer at another degree and mesh: identical fp32 inputs to one layer give the oracle's (floor, ceil) table
    indices bit for bit -- the mesh ends, the first and the last interval and points next to them included."""
    from test_gpu_parity import as_accurate_as_fp32_reference, close
    c = case(name)
    n_mesh = CASES[name][3]
    m, om, flat = c["m"], c["om"], c["flat"]
    n = float(n_mesh - 1)
    u = np.random.default_rng(7).uniform(0, 1, size=(512, 2)).astype(np.float32)
    u[:7] = [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [1.0 / n, (n - 1.0) / n], [1e-7, 1 - 1e-7], [0.25, 0.75], [(n - 1.0) / n, 1.0 / n]]
    per_layer = om.layer_param_count()
    for l in range(LAYERS):
        y, ld, idx = m.layer(l, u, return_bin_idx=True)
        lp_ = flat[l * per_layer:(l + 1) * per_layer]
        yo, ldo, idxo = om.imade_direct(lp_, u)
        yt, ldt, _ = om.imade_direct(lp_, u, f64=True)
        assert np.array_equal(idx, idxo), (name, l)
        close(y, yo, rtol=0, atol=2e-6)
        as_accurate_as_fp32_reference(ld, ldo, ldt, what=f"{name} layer {l} log-det")


@pytest.mark.parametrize("kernel", ["scalar", "mfma", "wave"])
@pytest.mark.parametrize("name", ["m33", "m4001"])
def test_walkers_outside_the_box_wrap_like_the_oracle(name, kernel):
    """test_walkers_outside_the_box_wrap_like_the_reference on another mesh: 256 walkers and a copy of them shifted by 2 L.  The shifted copy sits above
    the box: its last box coordinate (x_0 + L) / den exceeds 1, so the first layer's mesh indices lie beyond the table (up to 1e5 at 4001 points) and
    the gathers clamp to the last row as jnp's do (oracle: wrap_clamp; the negative-index wrap is the existing test's).  The oracle keeps every
    shifted walker finite: all of them are compared."""
    from test_gpu_parity import as_accurate_as_fp32_reference, close
    c = case(name)
    m, om, flat = c["m"], c["om"], c["flat"]
    x0 = sorted_walkers(256, 2, L, 31)
    x = np.concatenate([x0, x0 + np.float32(2 * L)])

    def make():
        lpo, uo, idxo = om.log_pdf(flat, x, return_u=True, return_idx=True)
        return lpo, uo, idxo, om.log_pdf(flat, x, f64=True)
    lpo, uo, idxo, lpt = ref(name, "outside", make)
    n_mesh = CASES[name][3]
    fin = np.isfinite(lpo)
    assert (idxo[256:, 0] > n_mesh - 1).any(axis=(1, 2)).all(), "a shifted walker has no index beyond the table"
    assert fin[256:].sum() >= 200, "too few shifted walkers stay finite in the oracle"
    set_kernel_or_skip(m, kernel)
    try:
        if kernel == "wave":
            lp, u = m.log_pdf(x, return_sample=True)
        else:
            lp, u, idx = m.log_pdf(x, return_sample=True, return_bin_idx=True)
            assert np.array_equal(np.asarray(idx)[:, 0], idxo[:, 0])            # layer 0: bit-identical inputs
        assert np.array_equal(np.isfinite(lp), fin)
        close(np.asarray(u)[fin], uo[fin], rtol=0, atol=5e-6)
        as_accurate_as_fp32_reference(np.asarray(lp)[fin], lpo[fin], lpt[fin], what=f"{name} {kernel} outside the box")
    finally:
        m.set_kernel("auto")


# ------------------------------------------------------------------------------------------------ 2. local energy

def _tile_and_wave(model, x, protons, monkeypatch):
    """(H psi, psi, laplacian) of x through the matrix-core tile path (forced) and through the wave kernel (tile path disabled), as tests/test_gpu_energy.py"""
    out = []
    for tile_min in ("1", "0"):
        monkeypatch.setenv("WF_ENERGY_TILE_MIN", tile_min)
        out.append([np.asarray(t, dtype=np.float64) for t in model.hamiltonian(x, protons, return_psi=True, return_laplacian=True)])
    monkeypatch.delenv("WF_ENERGY_TILE_MIN")
    return out


def _energy_refs(name):
    import torch
    from oracle import energy_torch as et
    c = case(name)
    D = CASES[name][0]
    x = sorted_walkers(300, D, 9.5, 3)
    protons = np.linspace(-3, 3, D)
    return x, protons, ref(name, "energy", lambda: (et.hamiltonian(torch_model(name, torch.float64), c["flat"], x.astype(np.float64), protons),
                                                     et.hamiltonian(torch_model(name, torch.float32), c["flat"], x, protons)))


@pytest.mark.parametrize("name", ALL)
def test_local_energy_on_the_wave_and_the_matrix_core_path(name, monkeypatch):
    """wf_hamiltonian_fwd of 300 walkers against energy_torch.hamiltonian in fp64, once on the wave kernel and once with WF_ENERGY_TILE_MIN lowered to
    the batch (k_efused for two particles, k_edir beyond): the assertions of test_local_energy_on_the_matrix_cores_beyond_two_particles -- 3 x the fp32
    torch model's own median and maximum deviation from fp64, + 1e-6 / 2e-5 of the scale.  Every case belongs to the tile family (a model outside
    it would take the wave kernel both times and give the same bits): the forced run must be another kernel's bits.  Two particles: a model
    created with WF_MFMA_NO_BAND (no support clamp of the table chunks) gives the bits of the clamped reads
    (test_local_energy_tile_path_other_models).

    Measured on the MI355X (deviation from fp64 as a multiple of the fp32 torch model's own: maximum / median, wave | tile): see DESIGN.md 4.19."""
    c = case(name)
    D = CASES[name][0]
    m = c["m"]
    x, protons, ((ho64, po64, lo64), (ho32, po32, lo32)) = _energy_refs(name)
    (hp, ps, lap), (hw, pw, lw) = _tile_and_wave(m, x, protons, monkeypatch)
    assert not np.array_equal(lap, lw), "the forced run took the wave kernel"
    paths = (("wave", hw, pw, lw), ("tile", hp, ps, lap))
    scale = np.abs(lo64).max()
    e_o = np.abs(lo32 - lo64)
    for tag, h, p, l in paths:
        e_g = np.abs(l - lo64)
        print(f"[hpsi {name} {tag}] laplacian vs fp64 torch oracle: max {e_g.max():.2e} = {e_g.max() / e_o.max():.2f} x the fp32 torch oracle's {e_o.max():.2e}, "
              f"median {np.median(e_g):.2e} = {np.median(e_g) / np.median(e_o):.2f} x its {np.median(e_o):.2e}; scale {scale:.2e}; "
              f"H psi max {np.abs(h - ho64).max():.2e} (oracle {np.abs(ho32 - ho64).max():.2e}, max|H psi| {np.abs(ho64).max():.2e}); "
              f"psi max {np.abs(p - po64).max():.2e} (oracle {np.abs(po32 - po64).max():.2e}, max|psi| {np.abs(po64).max():.2e})")
    for tag, h, p, l in paths:
        e_g = np.abs(l - lo64)
        assert np.isfinite(h).all(), tag
        np.testing.assert_allclose(p, po64, rtol=0, atol=3e-5 * np.abs(po64).max() + 3 * np.abs(po32 - po64).max())
        assert np.median(e_g) <= 3 * np.median(e_o) + 1e-6 * scale, (tag, np.median(e_g), np.median(e_o))
        assert e_g.max() <= 3 * e_o.max() + 2e-5 * scale, (tag, e_g.max(), e_o.max(), scale)
        np.testing.assert_allclose(h, ho64, rtol=0, atol=3 * np.abs(ho32 - ho64).max() + 2e-5 * np.abs(ho64).max())
    if D == 2:
        monkeypatch.setenv("WF_MFMA_NO_BAND", "1")
        params2, psi2, _, _ = build_device(name)
        monkeypatch.delenv("WF_MFMA_NO_BAND")
        (hp2, ps2, lap2), _ = _tile_and_wave(psi2.model, x, protons, monkeypatch)
        assert np.array_equal(hp2, hp) and np.array_equal(ps2, ps) and np.array_equal(lap2, lap)


@pytest.mark.parametrize("name", ["k1", "k8", "m4001", "d3m"])
def test_hessian_diagonal_sums_to_the_laplacian(name, monkeypatch):
    """wf_psi_coord_derivs: sum_d hdiag against the Laplacian of wf_hamiltonian_fwd on the same forced path, to the bounds of
    test_consistent_with_the_local_energy_entry_point -- 1e-4 in relative L2 on the wave sweep and on k_edir (psi bit for bit); two particles on the
    matrix cores (the five-component jet is another instantiation): psi and the sum within 1e-4 of max|.|."""
    c = case(name)
    D = CASES[name][0]
    m = c["m"]
    x, protons, _ = _energy_refs(name)
    for tag, tile_min in (("wave", "0"), ("tile", "1")):
        monkeypatch.setenv("WF_ENERGY_TILE_MIN", tile_min)
        grad, hdiag, psi = (np.asarray(t, dtype=np.float64) for t in m.psi_derivatives(x, hessian_diag=True, return_psi=True))
        hp, ps, lap = (np.asarray(t, dtype=np.float64) for t in m.hamiltonian(x, protons, return_psi=True, return_laplacian=True))
        monkeypatch.delenv("WF_ENERGY_TILE_MIN")
        assert np.isfinite(grad).all() and np.isfinite(hdiag).all()
        rel = np.linalg.norm(hdiag.sum(1) - lap) / np.linalg.norm(lap)
        print(f"[coord derivs {name} {tag}] sum hdiag vs laplacian: rel L2 {rel:.2e}, psi equal: {np.array_equal(psi, ps)}")
        if D == 2 and tag == "tile":
            for a, b in ((psi, ps), (hdiag.sum(1), lap)):
                assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (tag, np.abs(a - b).max() / np.abs(b).max())
        else:
            assert np.array_equal(psi, ps)
            assert rel <= 1e-4, (name, tag, rel)


# ------------------------------------------------------------------------------------------------ 3. parameter gradients

def _grad_inputs(name):
    D = CASES[name][0]
    B = 64
    return sorted_walkers(B, D, 9.5, 5), np.ones(B, np.float32), np.full(B, -0.5, np.float32)


def _psi_vjp_refs(name):
    """(fp64 autograd gradient, relative l2 deviation of the fp32 autograd gradient from it)"""
    import torch
    from oracle import energy_torch as et
    c = case(name)
    x, wp, wl = _grad_inputs(name)

    def make():
        g64 = et.psi_vjp(torch_model(name, torch.float64), c["flat"], x.astype(np.float64), wp, wl)
        g32 = et.psi_vjp(torch_model(name, torch.float32), c["flat"], x, wp, wl)
        return g64, rel_l2(g32, g64)
    return ref(name, "psi_vjp", make)


@pytest.mark.parametrize("name", ALL)
def test_psi_vjp_on_the_reverse_wave_sweeps(name, monkeypatch):
    """wf_psi_vjp with w_psi = 1, w_lap = -1/2 on 64 walkers against energy_torch.psi_vjp in fp64, relative l2 over the whole gradient: within 3 x the
    fp32 torch model's own relative l2 deviation from fp64 (the project's margin for another fp32 evaluation of equal quality) + 1e-6.
    Measured pairs: DESIGN.md 4.19."""
    c = case(name)
    x, wp, wl = _grad_inputs(name)
    g64, rel_o = _psi_vjp_refs(name)
    monkeypatch.setenv("WF_GRAD_TILE_MIN", "0")
    got = c["m"].psi_vjp(x, wp, wl).cpu().numpy().astype(np.float64)
    rel_g = rel_l2(got, g64)
    print(f"[psi_vjp {name} wave] rel l2 vs fp64 autograd: device {rel_g:.2e}, fp32 autograd {rel_o:.2e}")
    assert np.isfinite(got).all() and rel_g <= 3 * rel_o + 1e-6, (name, rel_g, rel_o)


@pytest.mark.parametrize("name", TWO)
def test_psi_vjp_on_the_matrix_cores(name, monkeypatch):
    """The same gradient with WF_GRAD_TILE_MIN lowered: k_efused + k_ebwd (wf_dispatch.cpp: grad_tile_capable_at asks for a batch of at least
    WF_GRAD_TILE_MIN walkers and a workspace of one 32-walker tile: 64 walkers are two tiles).  Same rule; the forced path is another kernel."""
    c = case(name)
    x, wp, wl = _grad_inputs(name)
    g64, rel_o = _psi_vjp_refs(name)
    monkeypatch.setenv("WF_GRAD_TILE_MIN", "0")
    wave = c["m"].psi_vjp(x, wp, wl).cpu().numpy().astype(np.float64)
    monkeypatch.setenv("WF_GRAD_TILE_MIN", "1")
    got = c["m"].psi_vjp(x, wp, wl).cpu().numpy().astype(np.float64)
    rel_g = rel_l2(got, g64)
    print(f"[psi_vjp {name} tile] rel l2 vs fp64 autograd: device {rel_g:.2e}, fp32 autograd {rel_o:.2e}; vs the wave sweeps {rel_l2(got, wave):.2e}")
    assert not np.array_equal(got, wave), "the forced run took the wave sweeps"
    assert np.isfinite(got).all() and rel_g <= 3 * rel_o + 1e-6, (name, rel_g, rel_o)


@pytest.mark.parametrize("name", ["k1", "k8", "m4001"])
def test_logpdf_vjp(name):
    """wf_logpdf_vjp with w = -1/B against energy_torch.logpdf_vjp in fp64 under the same rule."""
    import torch
    from oracle import energy_torch as et
    c = case(name)
    x, _, _ = _grad_inputs(name)
    w = np.full(len(x), -1.0 / len(x), np.float32)

    def make():
        g64 = et.logpdf_vjp(torch_model(name, torch.float64), c["flat"], x.astype(np.float64), w)
        return g64, rel_l2(et.logpdf_vjp(torch_model(name, torch.float32), c["flat"], x, w), g64)
    g64, rel_o = ref(name, "logpdf_vjp", make)
    got = c["m"].logpdf_vjp(x, w).cpu().numpy().astype(np.float64)
    rel_g = rel_l2(got, g64)
    print(f"[logpdf_vjp {name}] rel l2 vs fp64 autograd: device {rel_g:.2e}, fp32 autograd {rel_o:.2e}")
    assert np.isfinite(got).all() and rel_g <= 3 * rel_o + 1e-6, (name, rel_g, rel_o)


@pytest.mark.parametrize("name", ["k1", "m4001"])
def test_psi_jacobian_column_sums(name):
    """wf_psi_jac on 67 walkers: the column sums are wf_psi_vjp up to the order of the additions (test_gpu_param_jacobian.py: _column_sums_ok)."""
    import torch
    from test_gpu_param_jacobian import _column_sums_ok, _ring_coefs
    c = case(name)
    m = c["m"]
    B = 67
    x = torch.as_tensor(sorted_walkers(B, 2, 9.5, 6)).cuda()
    wp, wl = torch.ones(B), torch.full((B,), -0.5)
    _column_sums_ok(m.psi_jacobian(x, wp, wl), m.psi_vjp(x, wp, wl), B, _ring_coefs(m, True), f"psi - laplacian / 2, {name}")


# ------------------------------------------------------------------------------------------------ 4. inverse and samplers

KERNELS = {"wave": {"WF_WAVE_SAMPLE_MAX": "100000000", "WF_SAMPLE_TILE_MIN": "0"},     # one wave per walker
           "lane": {"WF_WAVE_SAMPLE_MAX": "0", "WF_SAMPLE_TILE_MIN": "0"}}             # one lane per walker


def _on(monkeypatch, kernel, B):
    """Route wf_inverse_fwd / wf_sample of B walkers to `kernel` ("staged": WF_SAMPLE_TILE_MIN lowered to the batch)"""
    monkeypatch.delenv("WF_WAVE_SAMPLE_MAX", raising=False)
    for k, v in (KERNELS[kernel] if kernel in KERNELS else {"WF_SAMPLE_TILE_MIN": str(B)}).items():
        monkeypatch.setenv(k, v)


def _round_trip(m, x, u):
    """|direct(x) - u| per entry (x: numpy, or a device tensor)"""
    u2, _ = m.flow(x)
    return np.abs((u2.cpu().numpy() if hasattr(u2, "cpu") else np.asarray(u2)) - u)


@pytest.mark.parametrize("name", TWO)
def test_exact_inverse_on_every_kernel(name, monkeypatch):
    """x = inverse(u, exact=True) of 3000 latent points on the wave kernel, the one-lane kernel and the staged kernel (wf_dispatch.cpp:
    tile_sample_capable_at admits every two-particle case): direct(x) = u and x against oracle.Model.inverse to the bounds of
    test_serial_inverse_vs_oracle; the kernels pairwise to those of test_wave_and_one_lane_samplers_draw_from_the_same_distribution.  The staged
    kernel's band-limited I-rows (degrees <= 7; full rows at degree 8) give the bits of the full rows (test_staged_sampler_of_large_batches).

    Before the wave kernel's search was widened it reached mesh points 0 .. 2048: m2049 passed as it stood, m4001 had 71 % of the walkers off the oracle by
    more than 2e-3 (median 3.8e-2, maximum 0.154) and a round trip of up to 8.8e-3."""
    c = case(name)
    m, om, flat = c["m"], c["om"], c["flat"]
    u = np.random.default_rng(0).uniform(0.02, 0.98, size=(3000, 2)).astype(np.float32)
    xo = ref(name, "inverse", lambda: om.inverse(flat, u, exact=True))
    xs = {}
    for kernel in ("wave", "lane", "staged"):
        _on(monkeypatch, kernel, len(u))
        xs[kernel] = np.asarray(m.inverse(u, exact=True))
        if kernel == "staged":
            monkeypatch.setenv("WF_SAMPLE_FULL_ROWS", "1")
            assert np.array_equal(xs[kernel], m.inverse(u, exact=True))
            monkeypatch.delenv("WF_SAMPLE_FULL_ROWS")
    assert not np.array_equal(xs["staged"], xs["wave"]) and not np.array_equal(xs["lane"], xs["wave"])   # three kernels, three sets of bits
    for kernel, x in xs.items():
        e, d = _round_trip(m, x, u), np.abs(x - xo)
        print(f"[inverse {name} {kernel}] round trip: median {np.median(e):.2e} max {e.max():.2e}; vs oracle: median {np.median(d):.2e} max {d.max():.2e} "
              f"beyond 2e-3: {(d > 2e-3).mean():.4f}")
    for kernel, x in xs.items():
        e, d = _round_trip(m, x, u), np.abs(x - xo)
        assert np.isfinite(x).all(), kernel
        assert np.median(e) < 2e-5 and e.max() < 5e-3, (name, kernel, np.median(e), e.max())
        assert np.median(d) < 1e-5 and (d > 2e-3).mean() < 5e-3, (name, kernel, np.median(d), d.max())
    for a, b in (("wave", "lane"), ("wave", "staged"), ("lane", "staged")):
        d = np.abs(xs[a] - xs[b])
        assert np.median(d) < 1e-6 and np.quantile(d, 0.999) < 2e-4 and d.max() < 2e-3, (name, a, b, np.median(d), d.max())


def test_reference_mode_inverse_on_a_large_mesh(monkeypatch):
    """exact=False (made.py:88: the conditioner sees the values being inverted) at 4001 mesh points on the wave kernel against the oracle, to the
    bounds of test_serial_inverse_vs_oracle."""
    c = case("m4001")
    u = np.random.default_rng(0).uniform(0.02, 0.98, size=(3000, 2)).astype(np.float32)
    _on(monkeypatch, "wave", len(u))
    d = np.abs(np.asarray(c["m"].inverse(u, exact=False)) - c["om"].inverse(c["flat"], u, exact=False))
    assert np.median(d) < 1e-5 and (d > 2e-3).mean() < 5e-3, (np.median(d), d.max())


@pytest.mark.parametrize("name", ["d3m", "d3k8"])
def test_inverse_round_trip_beyond_two_particles(name, monkeypatch):
    """direct(inverse(u)) = u on the wave and the one-lane kernel, walkers sorted and inside the box: the bounds of
    test_mean_type_box_inverse_beyond_two_particles."""
    c = case(name)
    m = c["m"]
    u = np.random.default_rng(0).uniform(0.02, 0.98, size=(3000, 3)).astype(np.float32)
    for kernel in ("wave", "lane"):
        _on(monkeypatch, kernel, len(u))
        x = np.asarray(m.inverse(u, exact=True))
        e = _round_trip(m, x, u)
        print(f"[inverse {name} {kernel}] round trip: median {np.median(e):.2e} max {e.max():.2e}")
        assert np.all(np.diff(x, axis=1) >= 0) and np.abs(x).max() <= L + 1e-4
        assert np.median(e) < 3e-5 and e.max() < 1e-2, (name, kernel, np.median(e), e.max())


@pytest.mark.parametrize("name", ["k7", "k8", "m33", "m4001"])
def test_samplers_draw_from_the_same_distribution(name, monkeypatch):
    """30 000 draws of the wave kernel and of the staged kernel against 40 000 of the one-lane kernel (other seeds): two-sample Kolmogorov-Smirnov on
    every coordinate and latent column, p > 1e-4 (test_wave_and_one_lane_samplers_draw_from_the_same_distribution,
    test_staged_sampler_of_large_batches).  No NaN walker (the bounded rejection loops are not exhausted); the same seed gives the same bits.
    Degree 8 (k8): wf_dispatch.cpp admits prior degrees <= 8 to the staged sampler, whose proposals read a 12-row window that holds the k + 1 <= 9
    live B-splines; its I-spline sums take full rows there (wf_kernels_etile_sample.hip: the band form is for degrees <= 7) -- it applies."""
    import torch
    from scipy import stats
    m = case(name)["m"]
    draws = {}
    for kernel, seed, n in (("wave", 7, 30000), ("lane", 8, 40000), ("staged", 7, 30000)):
        _on(monkeypatch, kernel, n)
        x, lat = m.sample(seed, n, return_latent=True, exact=True)
        x2, lat2 = m.sample(seed, n, return_latent=True, exact=True)
        assert torch.equal(x, x2) and torch.equal(lat, lat2), kernel
        assert torch.isfinite(x).all() and torch.isfinite(lat).all(), (kernel, int((~torch.isfinite(x)).any(dim=1).sum()))
        draws[kernel] = (x.cpu().numpy(), lat.cpu().numpy())
        assert lat.min().item() >= 0 and lat.max().item() <= 1 and np.abs(draws[kernel][0]).max() <= L + 1e-3
    assert not np.array_equal(draws["staged"][0], draws["wave"][0])   # same seed, another kernel: other proposal sequences
    for kernel in ("wave", "staged"):
        for col in range(2):
            for what, a, b in zip(("x", "latent"), draws[kernel], draws["lane"]):
                p = stats.ks_2samp(a[:, col], b[:, col]).pvalue
                assert p > 1e-4, (name, kernel, what, col, p)


def test_training_steps_sample_through_the_large_mesh():
    """wf_vqmc_train_step samples through the wave kernel: three fused steps of 128 walkers on the 4001-point model give the losses of the same steps
    issued call by call (wf_sample with the step's stream, wf_vqmc_loss_grad, wf_adam_step), as the fused step of tests/test_gpu_grad.py; the
    walkers of a step invert to their latent points."""
    import torch
    c = case("m4001")
    m, flat = c["m"], c["flat"]
    protons = np.array([0.0, 0.0])
    seed, Bt, lr, steps = 77, 128, 1e-3, 3

    def fresh():
        xs = torch.as_tensor(flat).cuda()
        return xs, torch.zeros_like(xs), torch.zeros_like(xs)
    try:
        xa, ma, va = fresh()
        st = m.make_train_state(xa, ma, va, 0, ring_len=8)
        m.set_params_device(xa)
        for _ in range(steps):
            m.train_step(st, seed, Bt, protons, lr, exact_sampler=True)
        torch.cuda.synchronize()
        assert int(st["counter"].item()) == steps
        ring = st["ring"].cpu().numpy()[:steps]
        xb, mb, vb = fresh()
        means = []
        for i in range(steps):
            m.set_params_device(xb)
            # the step's sampler stream: seed advanced by the step counter (wf_kernels_wave.hip: seed += counter * 0x9E3779B97F4A7C15)
            xs_i, lat_i = m.sample((seed + i * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF, Bt, return_latent=True, exact=True)
            e = _round_trip(m, xs_i, lat_i.cpu().numpy())
            assert np.median(e) < 2e-5 and e.max() < 5e-3, (i, np.median(e), e.max())
            sums_i, grad_i = m.vqmc_loss_grad(xs_i, protons, running_average=0.0)
            m.adam_step(xb, grad_i, mb, vb, i, lr)
            means.append(float(sums_i[0] / sums_i[2]))
        torch.cuda.synchronize()
        assert np.isfinite(ring).all() and (ring[:, 2] == Bt).all()
        # (Adam's bias corrections come from the host's powf in one path and the device's in the other: last-bit differences of the step size, 2e-9 + 1e-6 lr
        # in tests/test_gpu_grad.py -- and where such a difference moves an updated parameter across a rounding boundary, one ulp of the parameter per step.
        # Measured: 2.98e-8 = one ulp of a parameter in [0.25, 0.5), ten times the 3e-9 of that bound alone, which this model's 24 408 parameters over three
        # steps do not meet; the losses, which the comparison is about, agree to 1e-9 relative.)
        pa, pb = xa.cpu().numpy().astype(np.float64), xb.cpu().numpy().astype(np.float64)
        print(f"[train m4001] losses {ring[:, 0] / ring[:, 2]} call by call {means}; max parameter difference {np.abs(pa - pb).max():.2e}")
        assert (np.abs(pa - pb) <= 2e-9 + 1e-6 * lr + steps * 2.0 ** -23 * np.abs(pb)).all(), np.abs(pa - pb).max()
        assert np.allclose(ring[:, 0] / ring[:, 2], means, rtol=1e-6), (ring[:, 0] / ring[:, 2], means)
        assert np.abs(xa.cpu().numpy() - flat).max() > 1e-4
    finally:
        m.set_params(flat)


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_prior_mesh_smaller_than_its_basis_count_is_refused():
    """28 orthogonalised bases (k = 6, 23 knots) sampled on 17 or 27 mesh points have a singular Gram matrix: wf_model_create fails with WF_ERR_NUMERIC
    and a message instead of building tables from rounding residue."""
    from waveflow_amd import _lib, flows, model_factory, wavefunctions
    mt = model_factory.get_masked_transform
    for n_mesh in (17, 27):
        init = wavefunctions.Waveflow(
            flows.Serial(flows.BoxTransformLayer(L, "mean"), flows.IMADE(mt(), 6, 23, 0.05, 1e-6, {0: 0}, {0: 1}, n_spline_base_mesh_points=n_mesh), flows.Reverse()),
            mt(allow_negative_params=True), 6, 23, constraints_dict_left={0: 0}, constraints_dict_right={0: 0}, constrained_dimension_indices_left=[0],
            set_nn_output_grad_to_zero=False, n_spline_base_mesh_points=n_mesh)
        with pytest.raises(_lib.WfError) as e:
            init(0, 2)
        assert e.value.status == -6 and "table" in str(e.value), (n_mesh, str(e.value))


def test_two_mesh_points_with_an_m_spline_prior():
    """n_mesh = 2 (the smallest wf_model_create accepts) with MFlow's M-spline prior at degree 2: either refused with a negative status, or log_pdf of 256
    walkers equals the oracle's of the same two-point tables.  On two mesh points the prior's density vanishes with its boundary coefficients:
    log_pdf is 2 log(1e-7) + the layers' log-determinants, about -32.2 for every walker, and the fp32 oracle equals the rounded fp64 result on most
    of them -- the yardstick "as close as the fp32 oracle" has no width here.  The bound is that of the number format: D (layers + 1) = 6
    logarithms within one ulp each (none larger in magnitude than the sum), five additions and the rounding of the fp64 result, < 8 ulp of
    |log_pdf| (9.5e-7 relative; the oracle's own fp32 result is held to it as well)."""
    from waveflow_amd import _lib, flatten_params, flows, model_factory
    mt = model_factory.get_masked_transform
    init = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=2, n_internal_knots=5, spline_regularization=0.05, reverse_fun_tol=1e-6,
                                                  n_spline_base_mesh_points=2), flows.Reverse()) * 2), mt(), spline_degree=2, n_internal_knots=5,
                       n_spline_base_mesh_points=2)
    try:
        params, log_pdf, _ = init(0, 2)
    except _lib.WfError as e:
        assert e.status < 0 and str(e)
        return
    om = oracle.Model(D=2, n_layers=2, i_k=2, i_knots=5, i_reg=0.05, prior="mflow", p_k=2, p_knots=5, n_mesh=2)
    flat = flatten_params(params)
    x = np.random.default_rng(1).uniform(0.0, 1.0, size=(256, 2)).astype(np.float32)
    lp32, lp64 = om.log_pdf(flat, x).astype(np.float64), om.log_pdf(flat, x, f64=True).astype(np.float64)
    bound = 8 * 2.0 ** -23 * np.abs(lp64)
    assert (np.abs(lp32 - lp64) <= bound).all()
    for kernel in ("scalar", "mfma", "wave"):
        try:
            log_pdf.model.set_kernel(kernel)
        except _lib.WfError:
            continue
        lp = np.asarray(log_pdf(params, x), np.float64)
        err = np.abs(lp - lp64)
        print(f"[mflow on two mesh points, {kernel}] max |log_pdf - fp64 oracle| {err.max():.2e} = {(err / (2.0 ** -23 * np.abs(lp64))).max():.2f} ulp; fp32 oracle "
              f"{np.abs(lp32 - lp64).max():.2e}")
        assert np.isfinite(lp).all() and (err <= bound).all(), (kernel, err.max())
    log_pdf.model.set_kernel("auto")
