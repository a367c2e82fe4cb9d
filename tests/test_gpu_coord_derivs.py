"""wf_psi_coord_derivs: d psi / d x_d and d^2 psi / d x_d^2 per walker on the three paths of wf_hamiltonian_fwd (wave sweep, k_edir, k_efused /
launch-per-net), against the fp64 autograd reference pinned in tests/test_coord_derivs_host.py.  No walker is excluded from any comparison."""
import numpy as np
import pytest

from conftest import sorted_walkers
from test_coord_derivs_host import psi_grad_hdiag
from test_gpu_energy import he
from test_gpu_wide_chains import wide

pytestmark = pytest.mark.gpu


def dmodel(D):
    """the D-particle models of test_local_energy_on_the_matrix_cores_beyond_two_particles"""
    from waveflow_amd import flatten_params, model_factory
    n_layers = 2 if D < 8 else 3
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=n_layers, box_size=10.0)
    params, psi, log_pdf, sample = init_fun(11, D)
    psi.model.ensure_params(params)
    return params, psi, flatten_params(params), n_layers


def derivs(m, x, monkeypatch, tile_min=None, fused=None, hessian_diag=True):
    """(grad, hdiag, psi) as float64 on a forced path (tile_min "1": the matrix cores, "0": the wave sweep, None: the default switch)"""
    for name, v in (("WF_ENERGY_TILE_MIN", tile_min), ("WF_ENERGY_FUSED", fused)):
        monkeypatch.delenv(name, raising=False)
        if v is not None:
            monkeypatch.setenv(name, v)
    out = m.psi_derivatives(x, hessian_diag=hessian_diag, return_psi=True)
    monkeypatch.delenv("WF_ENERGY_TILE_MIN", raising=False)
    monkeypatch.delenv("WF_ENERGY_FUSED", raising=False)
    return [np.asarray(t, dtype=np.float64) for t in out]


def energy(m, x, protons, monkeypatch, tile_min=None, fused=None):
    for name, v in (("WF_ENERGY_TILE_MIN", tile_min), ("WF_ENERGY_FUSED", fused)):
        monkeypatch.delenv(name, raising=False)
        if v is not None:
            monkeypatch.setenv(name, v)
    out = m.hamiltonian(x, protons, return_psi=True, return_laplacian=True)
    monkeypatch.delenv("WF_ENERGY_TILE_MIN", raising=False)
    monkeypatch.delenv("WF_ENERGY_FUSED", raising=False)
    return [np.asarray(t, dtype=np.float64) for t in out]


def cases(he_flat, golden):
    """name -> (device model, fp64 / fp32 torch models' maker, flat parameters, walkers, forced paths [(tag, tile_min, fused)])"""
    import torch  # noqa: F401
    from oracle import energy_torch as et
    from waveflow_amd import flatten_params, flows, model_factory, wavefunctions
    WAVE, TILE = ("wave", "0", None), ("tile", "1", None)

    def he_case():
        params, psi, _, _ = he(he_flat)
        psi.model.ensure_params(params)
        x = np.concatenate([np.sort(golden["he_golden"]["sample_points"], -1), sorted_walkers(250, 2, 10.0, 5)]).astype(np.float32)
        return psi.model, et.he_model, he_flat, x, [WAVE, TILE, ("tile, launch per net", "1", "0")]

    def d_case(D):
        params, psi, flat, n_layers = dmodel(D)
        mk = lambda dt: et.TorchWaveflow(D, n_layers, "mean", 10.0, 6, 23, 0.05, tuple(range(D - 1)), dtype=dt)
        return psi.model, mk, flat, sorted_walkers(300 if D < 8 else 120, D, 9.5, 3).astype(np.float32), [WAVE, TILE]

    def wide_case():
        params, psi, _, _ = wide(5, L=5.0)
        mk = lambda dt: et.TorchWaveflow(5, 2, "mean", 5.0, 6, 33, 0.05, (0, 1, 2, 3), dtype=dt)
        return psi.model, mk, flatten_params(params), sorted_walkers(37, 5, 4.5, 21), [WAVE, ("wave (tiles asked for: none exist)", "1", None)]

    def first_case():
        params, psi, _, _ = wide(3, box="first", kn=23, L=5.0)
        mk = lambda dt: et.TorchWaveflow(3, 2, "first", 5.0, 6, 23, 0.05, (1, 2), dtype=dt)
        return psi.model, mk, flatten_params(params), sorted_walkers(96, 3, 4.5, 21), [WAVE]

    def gated_case():
        mt = model_factory.get_masked_transform
        init = wavefunctions.Waveflow(
            flows.Serial(flows.BoxTransformLayer(3.0), *(flows.IMADE(mt(), 6, 23, 0.05, 1e-6, set_nn_output_grad_to_zero=True), flows.Reverse()) * 2),
            mt(allow_negative_params=True), 6, 23, constraints_dict_left={0: 0}, constraints_dict_right={0: 0}, constrained_dimension_indices_left=[0])
        params, psi, _, _ = init(6, 2)
        psi.model.ensure_params(params)
        mk = lambda dt: et.TorchWaveflow(2, 2, "mean", 3.0, 6, 23, 0.05, (0,), dtype=dt, i_gate=True, p_gate=True)
        return psi.model, mk, flatten_params(params), sorted_walkers(96, 2, 2.7, 17), [WAVE, ("wave (tiles asked for: gated heads stay)", "1", None)]

    return {"He": he_case, "D3": lambda: d_case(3), "D4": lambda: d_case(4), "D8": lambda: d_case(8), "D5 at 33 knots": wide_case,
            "first-type box": first_case, "gated heads": gated_case}


@pytest.mark.parametrize("name", ["He", "D3", "D4", "D8", "D5 at 33 knots", "first-type box", "gated heads"])
def test_against_the_fp64_autograd_reference_on_every_path(name, golden, he_flat, monkeypatch):
    """The project's yardstick for the Laplacian (tests/test_gpu_energy.py:36-41, 169-174, 269-275), applied to the gradient and to the Hessian
    diagonal separately: with e_g = |gpu - fp64|, e_o = |fp32 autograd - fp64|, scale = max|fp64| of the array:
    median(e_g) <= 3 median(e_o) + 1e-6 scale; max(e_g) <= 4 max(e_o) + 2e-5 scale on the wave path, 3 max(e_o) + 2e-5 scale on the tile paths."""
    import torch
    m, mk, flat, x, paths = cases(he_flat, golden)[name]()
    p64, g64, h64 = psi_grad_hdiag(mk(torch.float64), flat, x.astype(np.float64))
    p32, g32, h32 = psi_grad_hdiag(mk(torch.float32), flat, x)
    seen = {}
    for tag, tile_min, fused in paths:
        grad, hdiag, psi = derivs(m, x, monkeypatch, tile_min, fused)
        seen[tag] = (grad, hdiag)
        assert grad.shape == g64.shape and hdiag.shape == h64.shape and np.isfinite(grad).all() and np.isfinite(hdiag).all()
        np.testing.assert_allclose(psi, p64, rtol=0, atol=3e-5 * np.abs(p64).max() + 3 * np.abs(p32 - p64).max())
        factor = 4 if tag.startswith("wave") else 3
        for what, a, r64, r32 in (("grad", grad, g64, g32), ("hdiag", hdiag, h64, h32)):
            scale = np.abs(r64).max()
            e_g, e_o = np.abs(a - r64), np.abs(r32 - r64)
            print(f"[coord derivs {name}, {tag}] {what} vs fp64 autograd: max {e_g.max():.2e} = {e_g.max() / e_o.max():.2f} x the fp32 autograd's, median "
                  f"{np.median(e_g):.2e} = {np.median(e_g) / np.median(e_o):.2f} x; scale {scale:.2e}")
            assert np.median(e_g) <= 3 * np.median(e_o) + 1e-6 * scale, (name, tag, what, np.median(e_g), np.median(e_o))
            assert e_g.max() <= factor * e_o.max() + 2e-5 * scale, (name, tag, what, e_g.max(), e_o.max(), scale)
    if "tile" in seen:   # the forced path is another kernel
        assert not np.array_equal(seen["tile"][1], seen["wave"][1])
    if "tile, launch per net" in seen:
        assert not np.array_equal(seen["tile, launch per net"][1], seen["tile"][1])


@pytest.mark.parametrize("name", ["He", "D3", "D8", "D5 at 33 knots"])
def test_consistent_with_the_local_energy_entry_point(name, golden, he_flat, monkeypatch):
    """Same forced path as wf_hamiltonian_fwd: psi bit for bit on the wave path (the value channel of the R3 sweep is that of the one-pass sweep) and
    on k_edir (the same launches); sum_d hdiag against its Laplacian to the 1e-4 in relative L2 that
    test_forward_laplacian_sweep_matches_directional_sweeps puts between two summation orders of the same numbers.  Two particles on the matrix
    cores with hdiag: the five-component jet is another instantiation -- psi and the sum within 1e-4 max|.|, the bound between the two forms of
    that path (tests/test_gpu_energy.py:181-182)."""
    m, mk, flat, x, paths = cases(he_flat, golden)[name]()
    protons = np.linspace(-3, 3, m.D)
    for tag, tile_min, fused in paths:
        grad, hdiag, psi = derivs(m, x, monkeypatch, tile_min, fused)
        grad_only, psi_only = derivs(m, x, monkeypatch, tile_min, fused, hessian_diag=False)
        hp, ps, lap = energy(m, x, protons, monkeypatch, tile_min, fused)
        rel = np.linalg.norm(hdiag.sum(1) - lap) / np.linalg.norm(lap)
        print(f"[coord derivs {name}, {tag}] sum hdiag vs laplacian: rel L2 {rel:.2e}; psi equal: {np.array_equal(psi, ps)}; "
              f"grad (gradient-only call) equal: {np.array_equal(grad_only, grad)}, max diff {np.abs(grad_only - grad).max() / np.abs(grad).max():.2e}")
        if name == "He" and tag.startswith("tile"):
            # k_efused / the head kernels with J5: another instantiation than the gradient-only call and than H psi (J)
            for a, b in ((psi, ps), (psi_only, ps), (hdiag.sum(1), lap), (grad_only, grad)):
                assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (tag, np.abs(a - b).max() / np.abs(b).max())
        else:
            # one instantiation writes the gradient with and without hdiag (wave: k_derivs_out, D >= 3 tiles: k_edir<D, true, true>): bit for bit
            assert np.array_equal(psi, ps) and np.array_equal(psi_only, ps)
            assert np.array_equal(grad_only, grad)
            assert rel <= 1e-4, (name, tag, rel)


@pytest.mark.parametrize("name", ["He", "D3", "D8"])
def test_tile_against_wave_on_large_ragged_batches(name, golden, he_flat, monkeypatch):
    """70 001 (He) / 20 001 (D = 3, 8) walkers up to the box edge, not a multiple of the 32-walker tile: per array the bounds the local-energy tests
    put on the Laplacian between the same two paths (test_gpu_energy.py:189, 282).  The default switch: tiles at these sizes, the wave sweep at 5 000."""
    m, mk, flat, _, _ = cases(he_flat, golden)[name]()
    D = m.D
    xb = sorted_walkers(70001 if D == 2 else 20001, D, 10.0, 21)
    tile = derivs(m, xb, monkeypatch, "1")
    wave = derivs(m, xb, monkeypatch, "0")
    mx, md = (2e-4, 1e-7) if D == 2 else (5e-4, 1e-6)
    for what, a, b in zip(("grad", "hdiag", "psi"), tile, wave):
        d = np.abs(a - b)
        print(f"[coord derivs {name}] {what} tile vs wave: max {d.max() / np.abs(b).max():.2e}, median {np.median(d) / np.abs(b).max():.2e} of max|wave|")
        assert np.isfinite(a).all() and d.max() <= mx * np.abs(b).max() and np.median(d) <= md * np.abs(b).max(), (name, what)
    for hd in (True, False):
        default = derivs(m, xb, monkeypatch, hessian_diag=hd)
        forced = derivs(m, xb, monkeypatch, "1", hessian_diag=hd)
        small = derivs(m, xb[:5000], monkeypatch, hessian_diag=hd)
        small_wave = derivs(m, xb[:5000], monkeypatch, "0", hessian_diag=hd)
        for a, b in zip(default + small, forced + small_wave):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["He", "D8"])
def test_launch_to_launch_bits_and_buffer_ends(name, golden, he_flat):
    """Repeated calls give the same bits (2^18 walkers of He, 20 001 of D = 8: the matrix-core paths); a ragged batch leaves no NaN of the suite's
    WF_POISON fill in its outputs and the element behind the end of an over-allocated output untouched."""
    import torch
    from waveflow_amd import _lib
    m, mk, flat, _, _ = cases(he_flat, golden)[name]()
    D = m.D
    xt = torch.as_tensor(sorted_walkers(1 << 18 if D == 2 else 20001, D, 10.0, 77)).cuda()
    for hd in (True, False):
        first = [t.clone() for t in m.psi_derivatives(xt, hessian_diag=hd, return_psi=True)]
        for _ in range(4):
            for a, b in zip(m.psi_derivatives(xt, hessian_diag=hd, return_psi=True), first):
                assert torch.equal(a, b)
    for B in (20001, 777):   # matrix cores, wave sweep
        x = torch.as_tensor(sorted_walkers(B, D, 10.0, 5)).cuda()
        grad = torch.full((B * D + 1,), 7.5, device="cuda")
        hdiag = torch.full((B * D + 1,), -7.5, device="cuda")
        psi = torch.full((B + 1,), 2.5, device="cuda")
        rc = _lib.lib().wf_psi_coord_derivs(m._h, m._p(x), B, m._p(psi), m._p(grad), m._p(hdiag), m._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.isfinite(grad).all() and torch.isfinite(hdiag).all() and torch.isfinite(psi).all()
        assert grad[-1] == 7.5 and hdiag[-1] == -7.5 and psi[-1] == 2.5
        assert not (grad[:-1] == 7.5).any() and not (hdiag[:-1] == -7.5).any()


def test_shapes_errors_and_the_physics_closures(golden, he_flat):
    import torch
    from waveflow_amd import _lib, model_factory
    from waveflow_amd.utils import physics
    params, psi, log_pdf, sample = he(he_flat)
    m = psi.model
    m.ensure_params(params)
    g0, h0, p0 = m.psi_derivatives(np.zeros((0, 2), np.float32), hessian_diag=True, return_psi=True)
    assert g0.shape == (0, 2) and h0.shape == (0, 2) and p0.shape == (0,)
    x = sorted_walkers(64, 2, 9.0, 3)
    g, h, p = m.psi_derivatives(x, hessian_diag=True, return_psi=True)
    g1, h1, p1 = m.psi_derivatives(x[:1], hessian_diag=True, return_psi=True)
    assert g1.shape == (1, 2) and h1.shape == (1, 2) and p1.shape == (1,)
    assert np.array_equal(g1, g[:1]) and np.array_equal(h1, h[:1]) and np.array_equal(p1, p[:1])
    assert isinstance(g, np.ndarray) and m.psi_derivatives(x).shape == (64, 2)
    # device tensors on a stream of their own: torch in, torch out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xt = torch.as_tensor(x).cuda()
        gt, ht = m.psi_derivatives(xt, hessian_diag=True)
        side.synchronize()
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy(), g) and np.array_equal(ht.cpu().numpy(), h)
    L = _lib.lib()
    xt = torch.as_tensor(x).cuda()
    assert L.wf_psi_coord_derivs(m._h, m._p(xt), 64, None, None, m._p(ht), m._stream()) == -1     # grad_dev is required
    assert L.wf_psi_coord_derivs(m._h, None, 4, None, None, None, None) == -1
    assert L.wf_psi_coord_derivs(m._h, None, 0, None, None, None, None) == 0
    # a model wf_hamiltonian_fwd refuses (MFlow prior): the same status
    p2, lp2, _ = model_factory.get_model(n_flow_layers=1)(0, 2)
    lp2.model.ensure_params(p2)
    xu = np.random.default_rng(0).uniform(0.1, 0.9, size=(8, 2)).astype(np.float32)
    with pytest.raises(_lib.WfError) as e_h:
        lp2.model.hamiltonian(xu, [0.0])
    with pytest.raises(_lib.WfError) as e_d:
        lp2.model.psi_derivatives(xu)
    assert e_d.value.status == e_h.value.status
    # the physics closures
    grad_fn = physics.construct_gradient_function(psi)
    hdiag_fn = physics.construct_hessian_diagonal_function(psi)
    assert grad_fn(params, x).shape == (64, 2) and hdiag_fn(params, x).shape == (64, 2)
    assert np.array_equal(grad_fn(params, x), g) and np.array_equal(hdiag_fn(params, x), h)
    drift = grad_fn(params, x) / (psi(params, x)[:, None] + 1e-8)      # the reference's regulariser (vqmc.py:196)
    assert drift.shape == (64, 2) and np.isfinite(drift).all()
