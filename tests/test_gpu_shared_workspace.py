"""DeviceModel keeps one workspace (_vjp_ws) for every gradient and Jacobian entry, grown on demand and never shrunk.  What an entry finds
there -- another entry's tape, a buffer larger than it asked for -- must not reach its result: each call of a mixed sequence on one model
gives the bits of the same call on a fresh model."""
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

B_SMALL, B_BIG = 3, 67   # one chunk of the fixed-order wave path each; 67: odd, larger than a wave


def test_entries_sharing_one_workspace_match_fresh_models(he_flat):
    import torch
    from waveflow_amd import core, model_factory
    init = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                            i_spline_reg=0.05, n_flow_layers=3, box_size=10)
    desc = init(0, 2)[1].model.desc

    def fresh():
        m = core.DeviceModel(desc)
        m.set_params(he_flat)
        return m

    x = torch.as_tensor(sorted_walkers(B_BIG, 2, 8.0, 5)).cuda()
    g = torch.Generator().manual_seed(11)
    w1, w2 = torch.randn(B_BIG, generator=g), torch.randn(B_BIG, generator=g)
    protons = [0.0, 0.0]
    s, b = B_SMALL, B_BIG
    sequence = [("logpdf_vjp(3)", lambda m: m.logpdf_vjp(x[:s], w1[:s])),
                ("psi_jacobian(67)", lambda m: m.psi_jacobian(x[:b], w1[:b], w2[:b])),
                ("psi_vjp(3)", lambda m: m.psi_vjp(x[:s], w1[:s], w2[:s])),
                ("logpdf_loss_grad(67)", lambda m: m.logpdf_loss_grad(x[:b], -1.0 / b)),
                ("vqmc_loss_grad(3)", lambda m: m.vqmc_loss_grad(x[:s], protons, -2.5)),
                ("logpdf_jacobian(3)", lambda m: m.logpdf_jacobian(x[:s], return_logp=True)),
                ("psi_vjp(67)", lambda m: m.psi_vjp(x[:b], w1[:b], w2[:b]))]
    shared = fresh()
    assert shared._vjp_ws is None
    sizes = []
    for what, call in sequence:
        got, want = call(shared), call(fresh())
        sizes.append(shared._vjp_ws.numel())
        got, want = (got, want) if isinstance(got, torch.Tensor) else (torch.cat([t.double().reshape(-1) for t in got]),
                                                                        torch.cat([t.double().reshape(-1) for t in want]))
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0, what
        assert torch.equal(got, want), (what, float((got - want).abs().max()))
    print(f"[shared workspace] bytes after each call: {sizes}")
    assert all(later >= earlier for earlier, later in zip(sizes, sizes[1:])), sizes
    assert sizes[1] > sizes[0]   # (the sequence does grow the buffer, so the small calls after it run in an oversized one)
