"""The law of wf_sample's draws on every sampler kernel against the oracle's fp64 conditional densities (tests/sampler_law.py; the yardstick itself is
verified on a CPU in tests/test_sampler_law_host.py).

Per case and path: lat = sample(seed, N, return_latent=True), v = F(lat) by the oracle's Rosenblatt transform on the CPU, and every statistic of
sampler_law.uniform_statistics(v) -- Kolmogorov-Smirnov per column, 8 x 8 chi-squares of every pair of columns and of neighbouring walkers -- has
p > 1e-6; column 0, which does not depend on the walker, additionally on 2^19 walkers.  The file holds fewer than 1000 statistics and its seeds are
fixed: a correct sampler fails with probability below 1e-3, and that outcome would be reproducible rather than flaky.  Also: no NaN draw, flow(x) gives
back the latent (exact inverse), walkers sorted and inside the box, other seeds are other streams, and a batch is the prefix of a larger one.

Paths: wave (WF_SAMPLE_TILE_MIN=0: one wave per walker), lane (additionally WF_WAVE_SAMPLE_MAX=0: one lane per walker, k_sample), staged (the default
from 16 384 walkers on, wf_kernels_etile_sample.hip; shown to be taken by draws that differ from the wave kernel's at the same seed)."""
import numpy as np
import pytest

import sampler_law as sl

pytestmark = pytest.mark.gpu

ENV = {
    "wave": {"WF_SAMPLE_TILE_MIN": "0", "WF_WAVE_SAMPLE_MAX": "100000000"},
    "lane": {"WF_SAMPLE_TILE_MIN": "0", "WF_WAVE_SAMPLE_MAX": "0"},
    "staged": {},
    # (phase 2 -- the inverse -- by eight lanes per walker: the default with two row blocks, forced with one; and everything on the walker's own lane)
    "staged_group_phase2": {"WF_SAMPLE_GROUP_PHASE2": "1"},
    "staged_one_lane": {"WF_SAMPLE_ONE_LANE": "1"},
}
SWITCHES = ("WF_SAMPLE_TILE_MIN", "WF_WAVE_SAMPLE_MAX", "WF_SAMPLE_GROUP_PHASE2", "WF_SAMPLE_ONE_LANE", "WF_SAMPLE_FULL_ROWS", "WF_SAMPLE_DENSE_ENVELOPE")
BOTH = ("wave", "lane")
RUNS = [("he", p) for p in BOTH + ("staged",)] + \
       [("two_row_blocks", p) for p in BOTH + ("staged", "staged_group_phase2", "staged_one_lane")] + \
       [("envelope_k8", p) for p in ("staged", "lane")] + [("envelope_k1", p) for p in ("staged", "lane")] + \
       [(n, p) for n in ("d3_mean_box", "d5", "d8", "first_box", "gated") for p in BOTH] + \
       [("boundary_d2", p) for p in BOTH + ("staged",)] + [("boundary_d3", p) for p in BOTH] + \
       [("mflow", p) for p in BOTH] + [("flow_normal", p) for p in BOTH]
_models = {}


def model(name):
    if name not in _models:
        _models[name] = sl.device_model(name)
    return _models[name]


def select(monkeypatch, path):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV[path].items():
        monkeypatch.setenv(k, v)


def shared_values_by_chance(name, n):
    """Two independent batches of n draws of column 0 share some values: the proposals carry 24 random bits (wf_philox.h), so two draws coincide with
    probability 2^-24 int p^2 -- lambda = n^2 2^-24 int p^2 shared values are expected (Poisson); the bound is lambda + 6 sqrt(lambda) + 3."""
    if name == "flow_normal":
        p2 = 0.5 / np.sqrt(np.pi)
    else:
        om = sl.oracle_model(name)
        g = np.linspace(0.0, 1.0, 4001).astype(np.float32)
        pts = np.zeros((g.size, om.D), np.float32)
        pts[:, 0] = g
        _, Z, dens, _ = om.prior_rosenblatt(sl.flat_params(name), pts, ncol=1, return_density=True)
        p = dens[:, 0] / Z[0, 0]
        p2 = float(np.sum(0.5 * (p[1:] ** 2 + p[:-1] ** 2) * np.diff(g.astype(np.float64))))
    lam = n * n * p2 / 2.0 ** 24
    return lam + 6.0 * np.sqrt(lam) + 3.0


@pytest.mark.parametrize("name,path", RUNS)
def test_law_of_the_draws(name, path, monkeypatch):
    import torch
    m, om, c = model(name), sl.oracle_model(name), sl.CASES[name]
    D, N = om.D, c["N"]
    seed = 4000 + 10 * RUNS.index((name, path))
    select(monkeypatch, path)
    x, lat = m.sample(seed, N, return_latent=True, exact=True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(lat).all()), "NaN draw"
    latn, xn = lat.cpu().numpy(), x.cpu().numpy()
    if path.startswith("staged"):
        # the staged path was taken: other draws than the wave kernel's at the same seed (and the variants of its launches draw what it draws)
        select(monkeypatch, "wave")
        assert not torch.equal(lat, m.sample(seed, N, return_latent=True, exact=True)[1])
        select(monkeypatch, path)
    # ---- the law: conditional columns on N walkers, column 0 on N0
    v, _ = sl.rosenblatt(name, latn)
    sl.assert_uniform(v, f"{name}, {path}")
    if N < sl.N0:
        lat0 = m.sample(seed + 1, sl.N0, return_latent=True, exact=False)[1]
        assert bool(torch.isfinite(lat0).all())
        v0, _ = sl.rosenblatt(name, lat0.cpu().numpy(), ncol=1)
        sl.assert_uniform(v0, f"{name}, {path}, column 0 of 2^19 walkers")
    # ---- x = inverse(lat): the forward pass gives the latent point back; walkers sorted and inside the box
    u, _ = m.flow(x)
    back = np.abs(u.cpu().numpy() - latn)
    print(f"[sampler law] {name}, {path}: |flow(x) - lat| median {np.median(back):.2e} max {back.max():.2e}")
    assert np.median(back) < 2e-5, np.median(back)
    if om.c.prior_kind in (0, 1):
        assert latn.min() >= 0.0 and latn.max() <= 1.0
    if om.c.box_kind:
        assert np.all(np.diff(xn, axis=1) >= -1e-4) and np.abs(xn).max() <= om.c.box_L + 1e-3
    elif om.c.prior_kind == 1:
        assert xn.min() >= 0.0 and xn.max() <= 1.0
    if name == "he":
        # the reference's inverse (conditioner on its inputs, made.py:88) of the same latent points
        xr, latr = m.sample(seed, N, return_latent=True, exact=False)
        assert torch.equal(latr, lat) and bool(torch.isfinite(xr).all()) and not torch.equal(xr, x)
        xr = xr.cpu().numpy()
        assert np.all(xr[:, 0] <= xr[:, 1] + 1e-4) and np.abs(xr).max() <= om.c.box_L + 1e-3
    # ---- another seed is another stream: no more shared values in column 0 than 24-bit proposals give by chance, none at the same walker (up to one)
    n2 = min(N, 16384)
    other = m.sample(seed + 1, n2, return_latent=True, exact=False)[1].cpu().numpy()
    shared = np.intersect1d(latn[:n2, 0], other[:, 0]).size
    assert shared <= shared_values_by_chance(name, n2), (shared, shared_values_by_chance(name, n2))
    assert (latn[:n2, 0] == other[:, 0]).sum() <= 1
    # ---- a batch is the prefix of a larger one (a walker's stream is keyed by its index)
    # (staged: 16 390 walkers end in a partial wave, whose lanes finish their own rejection loops; in the larger batch the same walkers sit in a full wave)
    small, big = (16390, 20000) if path.startswith("staged") else (1000, 5000)
    xs, ls = m.sample(seed + 2, small, return_latent=True, exact=True)
    xb, lb = m.sample(seed + 2, big, return_latent=True, exact=True)
    assert torch.equal(ls, lb[:small]) and torch.equal(xs, xb[:small])
