"""The two-tile k_mfma of the headline family (D = 2, one row block, SPEC) in its own-walker layout (wf_mfma_impl.h: lane L of a wave owns
walker pair * 64 + L, the MFMA phases keep walker = lane & 31 per tile, v_permlane32_swap joins the two).  Its arithmetic per walker is that of
the one-tile kernel, so every output must equal, bit for bit, the same call under WF_MFMA_WAVES=16 WF_MFMA_TILES=1 -- at 8 and at 4 waves, at
the batch sizes where a pair can go wrong (a lone walker, an empty or partial second tile, more than one chunk with a one-walker last pair),
with the walkers that take another path (outside the box: the FAR branch; on the box edge; equal coordinates) in a pair's first tile only, in
its second tile only and in both."""
import contextlib
import os

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

SHAPES = ((8, 2), (4, 2))
BATCHES = (1, 31, 32, 33, 63, 64, 65, 96, 513, 1000, 16384 + 33)


@contextlib.contextmanager
def _shape(waves, tiles):
    keys = {"WF_MFMA_WAVES": str(waves), "WF_MFMA_TILES": str(tiles)}
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(keys)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _he_model(flat):
    from waveflow_amd import checkpoint, model_factory
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, i_spline_reverse_fun_tol=1e-6, n_flow_layers=3, box_size=10, xu_coord_type="mean")
    params, psi, log_pdf, _ = init_fun(0, 2)
    m = psi.model
    m.ensure_params(checkpoint.unflatten_like(params, flat))
    m.set_kernel("mfma")
    return m


@pytest.fixture(scope="module")
def model(he_flat):
    m = _he_model(he_flat)
    yield m
    m.set_kernel("auto")


# the special walkers: (name, row, lane of the first tile).  A pair is 64 consecutive walkers, its first tile the first 32 of them.
KINDS = (("outside", (-10.002, 3.0), 3),     # u_1 of the box layer in (-1/1999, 0): x_l = -1 wraps, x_r = 0 -- the FAR branch
         ("edge", (-10.0, 10.0), 7),         # both electrons on the box edge
         ("equal", (1.25, 1.25), 11))        # x0 == x1: sorted either way, no inversion


def placements(B):
    """index -> row of the special walkers of a batch of B.  Kind k goes to three pairs: first tile only, second tile only, both.  With at
    least nine full pairs (B >= 576) those are nine different pairs, so each kind meets each placement in a pair that holds no other special
    walker; smaller batches take the pairs they have, in turn."""
    n_pairs = max(1, B // 64)
    put = {}
    for k, (_, row, lane) in enumerate(KINDS):
        for place, tiles in enumerate(((0,), (1,), (0, 1))):
            pair = (3 * k + place) % n_pairs
            for t in tiles:
                i = pair * 64 + 32 * t + lane
                if i < B:
                    put[i] = row
    return put


def walkers(B):
    x = sorted_walkers(B, 2, 10.0, 4000 + B)
    for i, row in placements(B).items():
        x[i] = row
    return x


def unsorted(x):
    """the same rows, every other one with its electrons exchanged (rows of equal coordinates stay what they are)"""
    xu = x.copy()
    xu[1::2] = xu[1::2, ::-1]
    return xu


def outputs(m, B):
    """log_pdf and the u of wf_logpdf_fwd, psi, the flow alone, psi_antisym of the unsorted rows: device tensors"""
    import torch
    x = walkers(B)
    xs, xu = torch.from_numpy(x).cuda(), torch.from_numpy(unsorted(x)).cuda()
    lp, u = m.log_pdf(xs, return_sample=True)
    fu, fld = m.flow(xs)
    return {"log_pdf": lp, "u": u, "psi": m.psi(xs), "flow_u": fu, "flow_logdet": fld, "psi_antisym": m.psi_antisym(xu)}


_REF = {}


def reference(m, B):
    """the one-tile kernel at 16 waves, once per batch size"""
    if B not in _REF:
        with _shape(16, 1):
            _REF[B] = outputs(m, B)
    return _REF[B]


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_placements_cover_each_tile_alone_and_both():
    """(no GPU work) from nine full pairs on, every kind sits in a first tile only, a second tile only and both, in pairs of its own"""
    for B in (1000, 16384 + 33):
        put = placements(B)
        pairs = {}
        for i, row in put.items():
            pairs.setdefault(i // 64, set()).add((row, (i % 64) // 32))
        assert len(pairs) == 9
        for _, row, _ in KINDS:
            seen = sorted(tuple(sorted(t for r, t in s)) for s in pairs.values() if {r for r, _ in s} == {row})
            assert seen == [(0,), (0, 1), (1,)], (B, row, seen)


@pytest.mark.parametrize("waves,tiles", SHAPES)
@pytest.mark.parametrize("B", BATCHES)
def test_paired_kernel_equals_one_tile_kernel_bit_for_bit(model, B, waves, tiles):
    import torch
    ref = reference(model, B)
    with _shape(waves, tiles):
        got = outputs(model, B)
    x = walkers(B)
    for name, r in ref.items():
        g = got[name]
        assert torch.equal(torch.isnan(g), torch.isnan(r)), (name, B, waves, tiles)
        bad = (g.contiguous().view(torch.int32) != r.contiguous().view(torch.int32)).reshape(B, -1).any(dim=1)
        assert same_bits(g, r), (name, B, waves, tiles, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
    # the reference itself saw what the batch was built for: an index below zero (outside), finite values elsewhere
    if B >= 64:
        inside = np.ones(B, bool)
        inside[list(placements(B))] = False
        assert bool(torch.isfinite(ref["log_pdf"][torch.from_numpy(inside).cuda()]).all())
        assert (x[:, 0] < -10.0).any() and (x[:, 0] == x[:, 1]).any()


@pytest.mark.parametrize("waves,tiles", SHAPES)
def test_paired_kernel_is_the_same_from_launch_to_launch(model, waves, tiles):
    import torch
    B = 16384 + 33
    xs = torch.from_numpy(walkers(B)).cuda()
    with _shape(waves, tiles):
        first_lp, first_psi = model.log_pdf(xs), model.psi(xs)
        for _ in range(10):
            assert same_bits(model.log_pdf(xs), first_lp) and same_bits(model.psi(xs), first_psi), (waves, tiles)
    assert same_bits(first_lp, reference(model, B)["log_pdf"])


@pytest.mark.parametrize("waves,tiles", SHAPES)
def test_paired_kernel_poisons_both_tiles_when_a_weight_leaves_the_fp16_range(he_flat, waves, tiles):
    """The entry points route around k_mfma while a packed weight is outside the fp16 range (test_fp16_range_guard_routes_around_the_matrix_cores:
    the same weight of 3e4); a launch that was captured into a graph before the upload runs anyway, and then every walker of both tiles must
    come back NaN -- full pairs, a pair with a partial second tile."""
    import torch
    m = _he_model(he_flat)
    B = 64 * 9 + 32 + 5
    xs = torch.from_numpy(sorted_walkers(B, 2, 9.5, 31)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with _shape(waves, tiles), torch.cuda.stream(side):
        warm = m.log_pdf(xs)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m.log_pdf(xs)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and same_bits(out, warm)
    bad_flat = he_flat.copy()
    D, H = 2, 64
    bad_flat[D * H + H + 5 * H + 7] = 3.0e4          # W1 of the first flow net: |(-2 * 2 log2 e) * 3e4| > 65 504
    m.set_params(bad_flat)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), int(torch.isnan(out).sum())
    m.set_params(he_flat)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, warm)
    m.set_kernel("auto")
