"""The chunk loops of the forward and energy entry points (wf_dispatch.cpp): every loop cuts the batch at multiples of its chunk and offsets three
to six pointers by c0 or c0 * D per chunk.  Each seam is crossed here: the entry once on the whole batch, then by hand on each slice
[c0, c0 + bc) cut where the loop cuts, in the same environment -- every returned array of the whole call is the concatenation of the slices bit
for bit, and a second whole call gives the same bits.  "Whole and slices wrong alike" is excluded by the project's fp64 yardsticks on the 64
walkers before and the 64 after each seam.

    wave evaluation (dispatch)                 2^20   set_kernel("wave")
    wave energy sweeps (run_energy_paths)      2^20   WF_ENERGY_TILE_MIN=0
    directional tile path, D >= 3              2^18   WF_ENERGY_TILE_MIN=1
    launch-per-net tile path, D = 2            WF_ENERGY_TILE_CHUNK (here 1024, its floor)   WF_ENERGY_FUSED=0 WF_ENERGY_TILE_MIN=1"""
import numpy as np
import pytest

import oracle
from conftest import sorted_walkers
from test_coord_derivs_host import psi_grad_hdiag
from test_gpu_coord_derivs import dmodel
from test_gpu_energy import he
from test_gpu_parity import as_accurate_as_fp32_reference

pytestmark = pytest.mark.gpu


def cuts(B, chunk):
    """[(c0, bc)] as `for (c0 = 0; c0 < B; c0 += chunk) bc = min(chunk, B - c0)` cuts"""
    return [(c0, min(chunk, B - c0)) for c0 in range(0, B, chunk)]


def seam_sample(B, chunk, n=64):
    """the n walkers before and the n after every interior seam"""
    idx = np.concatenate([np.arange(max(c0 - n, 0), min(c0 + n, B)) for c0, _ in cuts(B, chunk)[1:]])
    return np.unique(idx)


def assert_same_bits(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(ai, bi):
        rows = (ai != bi).reshape(a.shape[0], -1).any(dim=1).nonzero().flatten()
        raise AssertionError((what, f"{rows.numel()} of {a.shape[0]} rows differ", rows[:8].tolist(), rows[-1:].tolist()))


def whole_and_slices(call, names, x, chunk, tag):
    """call(x) -> tuple of device tensors.  The whole batch twice and every slice; -> the whole call's outputs."""
    import torch
    whole, again = call(x), call(x)
    parts = [call(x[c0:c0 + bc]) for c0, bc in cuts(x.shape[0], chunk)]
    assert len(parts) >= 2 and len(whole) == len(names)
    for k, name in enumerate(names):
        assert_same_bits(whole[k], again[k], (tag, name, "second whole call"))
        assert_same_bits(whole[k], torch.cat([p[k] for p in parts]), (tag, name, "whole call vs concatenated slices"))
    return dict(zip(names, whole))


def model_of(which, he_flat):
    """-> (device model, flat parameters, C oracle, torch oracle maker, protons, L of the energy walkers).  The walkers of the energy seams are those
    of the tests whose bounds are applied: up to the box edge for He, 0.95 L beyond two particles."""
    from oracle import energy_torch as et
    from waveflow_amd.utils import physics
    if which == "He":
        params, psi, _, _ = he(he_flat)
        psi.model.ensure_params(params)
        return psi.model, he_flat, oracle.he_model(10.0), et.he_model, physics.system_catalogue[1]["He"][0].reshape(-1), 10.0
    D = 3
    params, psi, flat, n_layers = dmodel(D)
    om = oracle.Model(D=D, n_layers=n_layers, box="mean", box_L=10.0, i_k=6, i_knots=23, i_reg=0.05, i_left={0: 0}, i_right={0: 1},
                      prior="waveflow", p_k=6, p_knots=23, p_left={0: 0}, p_right={0: 0}, constr_left=tuple(range(D - 1)))
    mk = lambda dt: et.TorchWaveflow(D, n_layers, "mean", 10.0, 6, 23, 0.05, tuple(range(D - 1)), dtype=dt)
    return psi.model, flat, om, mk, np.linspace(-3, 3, D), 9.5


# ---- forward entries

EVAL_NAMES = ("log_pdf", "log_pdf u", "psi", "flow u", "flow logdet")
UNSORTED_NAMES = ("psi_antisym", "inversions", "log_pdf_unsorted")


def eval_entries(m):
    def call(x):
        lp, u = m.log_pdf(x, return_sample=True)
        fu, fld = m.flow(x)
        return lp, u, m.psi(x), fu, fld
    return call


def unsorted_entries(m):
    def call(xu):
        ps, inv = m.psi_antisym(xu, return_inversions=True)
        return ps, inv, m.log_pdf_unsorted(xu)
    return call


@pytest.mark.parametrize("extra", [1, 77])
@pytest.mark.parametrize("which", ["He", "D3"])
def test_wave_evaluation_seam(which, extra, he_flat):
    """dispatch(): launch_wave_eval per 2^20 walkers with x + c0 * D, out + c0, u + c0 * D; with the presort bit the sorted rows sit behind the
    wave tails of one chunk in the scratch and the loop reads them at c0 * D, the sign is applied to the whole batch behind the loop."""
    import torch
    from waveflow_amd.utils.coordinates import get_num_inversion_count
    m, flat, om, _, _, _ = model_of(which, he_flat)
    D, chunk = m.D, 1 << 20
    B = chunk + extra
    m.set_kernel("wave")
    xn = sorted_walkers(B, D, 10.0, 600 + extra)
    xun = np.random.default_rng(601 + extra).permuted(xn, axis=1)          # each row's coordinates shuffled
    x, xu = torch.from_numpy(xn).cuda(), torch.from_numpy(xun).cuda()
    tag = (which, "wave evaluation", B)
    out = whole_and_slices(eval_entries(m), EVAL_NAMES, x, chunk, tag)
    uns = whole_and_slices(unsorted_entries(m), UNSORTED_NAMES, xu, chunk, tag)
    # the unsorted entries against the sorted ones of the same whole batch: integers and bits
    inv_host = get_num_inversion_count(xun)
    assert (inv_host[chunk:] > 0).any() or extra == 1
    assert np.array_equal(uns["inversions"].cpu().numpy(), inv_host)
    flip = torch.from_numpy(np.where(inv_host & 1, np.int32(-2 ** 31), np.int32(0))).cuda()
    assert torch.equal(uns["psi_antisym"].view(torch.int32), out["psi"].view(torch.int32) ^ flip)
    assert_same_bits(uns["log_pdf_unsorted"], out["log_pdf"], (tag, "log_pdf_unsorted vs log_pdf of the sorted rows"))
    if extra == 77:
        sel = seam_sample(B, chunk)
        assert len(sel) == 128
        xs = xn[sel]
        lp, ps = out["log_pdf"].cpu().numpy()[sel], out["psi"].cpu().numpy()[sel]
        as_accurate_as_fp32_reference(lp, om.log_pdf(flat, xs, threads=8), om.log_pdf(flat, xs, threads=8, f64=True), what=f"{which} log_pdf across the 2^20 seam")
        o64 = om.psi(flat, xs, threads=8, f64=True)
        # (psi's atol: that of the tests of the same models -- test_he_checkpoint_vs_reference_golden_grid, test_waveflow_other_shapes_vs_oracle)
        as_accurate_as_fp32_reference(ps, om.psi(flat, xs, threads=8), o64, atol=1e-5 if which == "He" else 1e-6 * np.abs(o64).max(),
                                      what=f"{which} psi across the 2^20 seam")


# ---- energy entries

ENERGY_NAMES = ("H psi", "psi", "laplacian")
DERIV_NAMES = ("grad", "hdiag", "psi")


def check_energy_sample(which, mk, flat, xs, protons, got, derivs, factor_derivs, tag):
    """The bounds of test_local_energy_on_the_matrix_cores_vs_oracle_and_wave_kernel / ..._beyond_two_particles on (H psi, psi, laplacian), those of
    test_against_the_fp64_autograd_reference_on_every_path on (grad, hdiag, psi): e_g = |gpu - fp64|, e_o = |fp32 autograd - fp64|."""
    import torch
    from oracle import energy_torch as et
    hp, ps, lap = (np.asarray(got[n].cpu().numpy(), np.float64) for n in ENERGY_NAMES)
    ho64, po64, lo64 = et.hamiltonian(mk(torch.float64), flat, xs.astype(np.float64), protons)
    ho32, po32, lo32 = et.hamiltonian(mk(torch.float32), flat, xs, protons)
    psi_atol = 3e-5 if which == "He" else 3e-5 * np.abs(po64).max() + 3 * np.abs(po32 - po64).max()
    scale = np.abs(lo64).max()
    e_g, e_o = np.abs(lap - lo64), np.abs(lo32 - lo64)
    hp_atol = 3 * np.abs(ho32 - ho64).max() + 2e-5 * np.abs(ho64).max()
    print(f"[seam {tag}] laplacian vs fp64: max {e_g.max():.2e} ({e_o.max():.2e} fp32 oracle) median {np.median(e_g):.2e} ({np.median(e_o):.2e}) scale {scale:.2e}; "
          f"H psi max err {np.abs(hp - ho64).max():.2e} (bound {hp_atol:.2e}); psi max err {np.abs(ps - po64).max():.2e} (bound {psi_atol:.2e})")
    np.testing.assert_allclose(ps, po64, rtol=0, atol=psi_atol)
    assert np.median(e_g) <= 3 * np.median(e_o) + 1e-6 * scale, (tag, np.median(e_g), np.median(e_o))
    assert e_g.max() <= 3 * e_o.max() + 2e-5 * scale, (tag, e_g.max(), e_o.max(), scale)
    np.testing.assert_allclose(hp, ho64, rtol=0, atol=hp_atol)
    grad, hdiag, psi = (np.asarray(derivs[n].cpu().numpy(), np.float64) for n in DERIV_NAMES)
    p64, g64, h64 = psi_grad_hdiag(mk(torch.float64), flat, xs.astype(np.float64))
    p32, g32, h32 = psi_grad_hdiag(mk(torch.float32), flat, xs)
    np.testing.assert_allclose(psi, p64, rtol=0, atol=3e-5 * np.abs(p64).max() + 3 * np.abs(p32 - p64).max())
    for what, a, r64, r32 in (("grad", grad, g64, g32), ("hdiag", hdiag, h64, h32)):
        scale = np.abs(r64).max()
        e_g, e_o = np.abs(a - r64), np.abs(r32 - r64)
        print(f"[seam {tag}] {what} vs fp64 autograd: max {e_g.max():.2e} = {e_g.max() / e_o.max():.2f} x the fp32 autograd's, median "
              f"{np.median(e_g):.2e} = {np.median(e_g) / np.median(e_o):.2f} x; scale {scale:.2e}")
        assert np.median(e_g) <= 3 * np.median(e_o) + 1e-6 * scale, (tag, what, np.median(e_g), np.median(e_o))
        assert e_g.max() <= factor_derivs * e_o.max() + 2e-5 * scale, (tag, what, e_g.max(), e_o.max(), scale)


def energy_seam(which, he_flat, monkeypatch, env, chunk, B, with_fp64, factor_derivs, seed):
    import torch
    m, flat, _, mk, protons, L = model_of(which, he_flat)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    xn = sorted_walkers(B, m.D, L, seed)
    x = torch.from_numpy(xn).cuda()
    tag = (which, " ".join(f"{k}={v}" for k, v in env.items()), B)
    got = whole_and_slices(lambda t: m.hamiltonian(t, protons, return_psi=True, return_laplacian=True), ENERGY_NAMES, x, chunk, tag)
    der = whole_and_slices(lambda t: m.psi_derivatives(t, hessian_diag=True, return_psi=True), DERIV_NAMES, x, chunk, tag)
    for o in list(got.values()) + list(der.values()):
        assert bool(torch.isfinite(o).all()), tag
    if with_fp64:
        sel = seam_sample(B, chunk)
        assert len(sel) == 128 * (len(cuts(B, chunk)) - 1)
        t = torch.from_numpy(sel).cuda()
        check_energy_sample(which, mk, flat, xn[sel], protons, {n: v[t] for n, v in got.items()}, {n: v[t] for n, v in der.items()}, factor_derivs, tag)
    return m, x, protons, got, der


@pytest.mark.parametrize("extra", [1, 77])
@pytest.mark.parametrize("which", ["He", "D3"])
def test_wave_energy_sweep_seam(which, extra, he_flat, monkeypatch):
    """run_energy_paths: launch_wave_energy / launch_wave_derivs per 2^20 walkers (x + c0 * D, hpsi + c0, psi(c0), lap(c0), grad + c0 * D, hd(c0))"""
    energy_seam(which, he_flat, monkeypatch, {"WF_ENERGY_TILE_MIN": "0"}, 1 << 20, (1 << 20) + extra, extra == 77, 4, 610 + extra)


@pytest.mark.parametrize("extra", [1, 77])
def test_directional_tile_path_seam(extra, he_flat, monkeypatch):
    """run_energy_paths: launch_energy_dir / launch_derivs_dir per 2^18 walkers; a short last slice stays on the path (WF_ENERGY_TILE_MIN=1)"""
    m, x, protons, got, der = energy_seam("D3", he_flat, monkeypatch, {"WF_ENERGY_TILE_MIN": "1"}, 1 << 18, (1 << 18) + extra, extra == 77, 3, 620 + extra)
    # the forced path is another kernel than the wave sweep
    monkeypatch.setenv("WF_ENERGY_TILE_MIN", "0")
    lap_wave = m.hamiltonian(x[-1000:], protons, return_laplacian=True)[1]
    assert not bool((lap_wave == got["laplacian"][-1000:]).all())


def test_launch_per_net_tile_path_seams(he_flat, monkeypatch):
    """run_energy_paths: launch_energy_tile / launch_derivs_tile per WF_ENERGY_TILE_CHUNK walkers, the conditioner and head kernels exchanging through
    the scratch re-used by every chunk.  1024 is the floor of the knob: three seams in 3 * 1024 + 77 walkers."""
    import torch
    env = {"WF_ENERGY_FUSED": "0", "WF_ENERGY_TILE_CHUNK": "1024", "WF_ENERGY_TILE_MIN": "1"}
    m, x, protons, got, der = energy_seam("He", he_flat, monkeypatch, env, 1024, 3 * 1024 + 77, True, 3, 630)
    # the knob is read: a chunk of the whole batch gives the same bits (one chunk, no seam), and the launch-per-net form is another kernel than
    # the one-launch form
    monkeypatch.setenv("WF_ENERGY_TILE_CHUNK", str(1 << 19))
    one = m.hamiltonian(x, protons, return_psi=True, return_laplacian=True)
    for name, o in zip(ENERGY_NAMES, one):
        assert_same_bits(got[name], o, ("one chunk vs four", name))
    monkeypatch.delenv("WF_ENERGY_FUSED")
    fused = m.hamiltonian(x, protons, return_laplacian=True)[1]
    assert not torch.equal(fused, got["laplacian"])
