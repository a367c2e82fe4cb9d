"""Coordinate derivatives of psi (wf_psi_coord_derivs): the fp64 yardstick of tests/test_gpu_coord_derivs.py, pinned on the host, and the
Python surface.  No GPU."""
import numpy as np
import pytest

from conftest import sorted_walkers


def psi_grad_hdiag(model, flat, x):
    """oracle.energy_torch.hamiltonian (energy_torch.py:201-212) keeping the gradient and each Hessian diagonal entry instead of their sum:
    -> (psi [B], d psi / d x_d [B, D], d^2 psi / d x_d^2 [B, D]) with the reference's autodiff semantics (jax.grad / diag jax.hessian)."""
    import torch
    x = torch.as_tensor(np.asarray(x), dtype=model.dtype).clone().requires_grad_(True)
    ps = model.psi(flat, x)
    (g,) = torch.autograd.grad(ps.sum(), x, create_graph=True)
    hd = torch.zeros_like(g)
    for i in range(x.shape[1]):
        (gi,) = torch.autograd.grad(g[:, i].sum(), x, retain_graph=True)
        hd[:, i] = gi[:, i]
    return ps.detach().numpy(), g.detach().numpy(), hd.numpy()


def _d3_model(dtype, n_mesh=2000):
    from oracle import energy_torch as et
    return et.TorchWaveflow(3, 2, "mean", 10.0, 6, 23, 0.05, (0, 1), dtype=dtype, n_mesh=n_mesh)


def _d3_flat(model):
    """random parameters in the flat leaf order TorchWaveflow._net reads: two layer nets and the prior's"""
    n_net = lambda nb: 3 * 64 + 64 + 64 * 64 + 64 + 64 * nb * 3 + nb * 3 + 3 * nb
    return (0.1 * np.random.default_rng(5).normal(size=2 * n_net(model.i_nb) + n_net(model.p_nb))).astype(np.float32)


@pytest.mark.parametrize("which", ["he", "d3"])
def test_fp64_reference_sums_to_the_laplacian_and_matches_central_differences(which, he_flat):
    """The reference of the GPU tests before any GPU runs.  (1) sum_d hdiag is et.hamiltonian's Laplacian.  (2) grad and hdiag against central
    differences, with a bound derived here, not tuned.

    psi is built on table lerps whose derivative is, by the reference's rule, the lerp of the next derivative table -- not the slope of the
    lerp itself.  With f the lerped function on the shipped mesh (2000 points) and F the same model on a mesh four times as fine (the lerp
    error falls with the square of the spacing, so 16/15 |f - F| bounds f's own lerp error e against the exact splines S), for the central
    difference C_h[f] = (f(x + h) - f(x - h)) / 2h:
        |C_h[f] - f'_rule| <= |C_h[f] - C_h[S]| + |C_h[S] - S'| + |S' - f'_rule| <= e_0 / h + h^2 max|S'''| / 6 + e_1,
    e_0 the lerp error of the differenced quantity, e_1 that of its rule derivative, max|S'''| estimated by the third difference on the same
    stencil (x -+ h, x -+ 2h; centred at x - h, x and x + h, to cover the interval) of the fine-mesh function, plus the rounding of the fp64 difference, 4 eps max|f| / h (a few operations' worth).
    grad: f = psi;  hdiag: f = d psi / d x_d (the autograd gradient), differenced along d.  h: two cells of the shipped mesh in x
    (2 L / 2000 per cell), so that e_0 / h -- the term that grows as h shrinks -- and the truncation term are of one order."""
    import torch
    from oracle import energy_torch as et
    if which == "he":
        D, flat = 2, he_flat
        coarse, fine = et.he_model(torch.float64), et.TorchWaveflow(2, 3, "mean", 10.0, 6, 23, 0.05, (0,), dtype=torch.float64, n_mesh=8000)
    else:
        D = 3
        coarse, fine = _d3_model(torch.float64), _d3_model(torch.float64, 8000)
        flat = _d3_flat(coarse)
    h = 2 * (2 * 10.0 / 2000)
    # 64 sorted walkers whose seven-point stencils stay sorted (the model's domain): the first 64 of a pool with gaps > 6 h.  Inside |x| <= 9 of the
    # box of 10: at the edge the reference clips the prior's argument (wavefunctions.py:45) and psi has a kink there, where no bound in terms of
    # a third derivative holds (and the antisymmetric third difference does not see a kink at the centre of its stencil)
    pool = sorted_walkers(1024, D, 9.0, 31).astype(np.float64)
    x = pool[np.diff(pool, axis=1).min(1) > 6 * h][:64]
    assert x.shape == (64, D)
    ps, g, hd = psi_grad_hdiag(coarse, flat, x)
    _, _, lap = et.hamiltonian(coarse, flat, x, np.zeros(D))
    assert np.abs(hd.sum(1) - lap).max() <= 1e-12 * np.abs(lap).max()
    assert np.abs(g).max() > 0 and np.abs(hd).max() > 0

    eps = np.finfo(np.float64).eps
    for d in range(D):
        e = np.zeros(D); e[d] = h
        pts = [x + k * e for k in range(-3, 4)]
        fc = [psi_grad_hdiag(coarse, flat, p) for p in pts]
        ff = [psi_grad_hdiag(fine, flat, p) for p in pts]
        for name, idx, target in (("grad", 0, g[:, d]), ("hdiag", 1, hd[:, d])):
            pick = (lambda r: r[0]) if idx == 0 else (lambda r: r[1][:, d])          # the differenced quantity: psi, or d psi / d x_d
            rule = (lambda r: r[1][:, d]) if idx == 0 else (lambda r: r[2][:, d])    # its derivative by the reference's rule
            c = [pick(r) for r in fc]
            f = [pick(r) for r in ff]
            central = (c[4] - c[2]) / (2 * h)
            # the maximum of the third derivative over [x - h, x + h]: the third differences centred at x - h, x and x + h
            third = np.max([np.abs(f[k + 2] - 2 * f[k + 1] + 2 * f[k - 1] - f[k - 2]) for k in (2, 3, 4)], axis=0) / (2 * h ** 3)
            e0 = 16 / 15 * max(np.abs(a - b).max() for a, b in zip(c, f))
            e1 = 16 / 15 * np.abs(rule(fc[3]) - rule(ff[3])).max()
            bound = e0 / h + h * h * third.max() / 6 + e1 + 4 * eps * max(np.abs(a).max() for a in c) / h
            err = np.abs(central - target).max()
            print(f"[{which} d={d} {name}] central difference vs rule: {err:.3e}, bound {bound:.3e} (lerp {e0 / h:.2e} + {e1:.2e}, truncation {h * h * third.max() / 6:.2e}); scale {np.abs(target).max():.2e}")
            assert err <= bound, (which, d, name, err, bound)
            assert bound <= 0.25 * np.abs(target).max()      # ... and the bound says something: a derivative off by a factor, or missing, is far outside it


def test_python_surface():
    from waveflow_amd import _lib
    from waveflow_amd.utils import physics
    assert "wf_psi_coord_derivs" in _lib.EXPORTS
    for make in (physics.construct_gradient_function, physics.construct_hessian_diagonal_function):
        with pytest.raises(TypeError):
            make(lambda params, x: x)
    from waveflow_amd.core import DeviceModel
    assert callable(DeviceModel.psi_derivatives)
