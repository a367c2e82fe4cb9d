"""Per-walker parameter Jacobians (wf_logpdf_jac, wf_psi_jac; the jax.jacrev(log_pdf, argnums=0)(params, batch) of vqmc.py:179): the rows whose
sum over the walkers is wf_logpdf_vjp / wf_psi_vjp.  Column sums against those entries, rows bit for bit independent of the batch and the
chunking, rows against the fp64 autograd oracle and fp64 central differences, the pytree surface, the refusals."""
import ctypes

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

B_BIG = 67   # odd, larger than a wave, no multiple of k_wgrad's 8 / 16 / 32-sample slabs


def rel_l2(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _waveflow(D, k, knots, layers, box, kind="mean", i_left=None, gated=False, seed=7):
    from waveflow_amd import flows, model_factory, wavefunctions
    if i_left is None and not gated:
        init = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                                i_spline_reg=0.05, n_flow_layers=layers, box_size=box, xu_coord_type=kind)
    else:
        mt = model_factory.get_masked_transform
        imade = flows.IMADE(mt(), k, knots, 0.05, 1e-6, i_left or {0: 0}, {0: 1}, set_nn_output_grad_to_zero=gated)
        init = wavefunctions.Waveflow(flows.Serial(flows.BoxTransformLayer(box), *(imade, flows.Reverse()) * layers), mt(allow_negative_params=True), k, knots,
                                      constraints_dict_left={0: 0}, constraints_dict_right={0: 0}, constrained_dimension_indices_left=list(range(D - 1)),
                                      set_nn_output_grad_to_zero=gated)
    return init(seed, D)


# name -> (builder of (params, psi or None, log_pdf), walkers(B)); the smallest models that reach each path of the sweeps and of k_wjac
def _build(name, he_flat):
    from waveflow_amd import checkpoint, flows, model_factory
    mt = model_factory.get_masked_transform
    unit = lambda B: (np.random.default_rng(31).random((B, 2)) * 0.9 + 0.05).astype(np.float32)
    if name == "he":                 # D = 2, k = 6, 23 knots, 3 layers: RF<2>, one row block
        params, psi, log_pdf, _ = _waveflow(2, 6, 23, 3, 10.0)
        return checkpoint.unflatten_like(params, he_flat), psi, log_pdf, lambda B: sorted_walkers(B, 2, 8.0, 5)
    if name == "he_gated":           # the same with gated heads: the zero_params leaves take the adjoints of zws
        params, psi, log_pdf, _ = _waveflow(2, 6, 23, 3, 10.0, gated=True, seed=6)
        return params, psi, log_pdf, lambda B: sorted_walkers(B, 2, 8.0, 5)
    if name == "left_dict":          # derivative constraints on the left of the I layers
        params, psi, log_pdf, _ = _waveflow(2, 6, 23, 1, 3.0, i_left={0: 0.0, 2: 0.0, 3: 0.0}, seed=4)
        return params, psi, log_pdf, lambda B: sorted_walkers(B, 2, 2.7, 13)
    if name == "d3_first":           # three particles, the 'first' box: RF<3>, two output passes
        params, psi, log_pdf, _ = _waveflow(3, 4, 13, 2, 5.0, kind="first")
        return params, psi, log_pdf, lambda B: sorted_walkers(B, 3, 4.5, 21)
    if name == "d2_wide":            # 33 knots: two row blocks per dimension
        params, psi, log_pdf, _ = _waveflow(2, 6, 33, 2, 5.0)
        return params, psi, log_pdf, lambda B: sorted_walkers(B, 2, 4.5, 21)
    if name == "d5_wide":            # 33 knots at D = 5: the R3 ring, five samples per walker (k = 6: 38 prior bases, the orthogonalisation needs an even count)
        params, psi, log_pdf, _ = _waveflow(5, 6, 33, 1, 5.0)
        return params, psi, log_pdf, lambda B: sorted_walkers(B, 5, 4.5, 21)
    if name == "MFlow":
        params, log_pdf, _ = flows.MFlow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=15, spline_regularization=0.01, reverse_fun_tol=1e-6),
                                                         flows.Reverse()) * 3), mt(), spline_degree=3, n_internal_knots=15)(0, 2)
        return params, None, log_pdf, unit
    if name == "IFlow":
        params, log_pdf, _ = flows.Flow(flows.Serial(*(flows.IMADE(mt(), spline_degree=5, n_internal_knots=15, spline_regularization=0.1, reverse_fun_tol=1e-6),
                                                        flows.Reverse()) * 2), flows.Uniform(), prior_support=(0.0, 1.0))(2, 2)
        return params, None, log_pdf, unit
    if name == "Flow":               # MADE + Normal
        params, log_pdf, _ = flows.Flow(flows.Serial(*(flows.MADE(mt(return_simple_masked_transform=True)), flows.Reverse()) * 3), flows.Normal(-0.5))(3, 2)
        return params, None, log_pdf, lambda B: (np.random.default_rng(31).normal(size=(B, 2)) * 0.7 + 0.5).astype(np.float32)
    raise KeyError(name)


def _oracle_head(name):
    import oracle
    return {"MFlow": lambda: oracle.Model(D=2, n_layers=3, i_k=5, i_knots=15, i_reg=0.01, prior="mflow", p_k=3, p_knots=15),
            "IFlow": lambda: oracle.Model(D=2, n_layers=2, i_k=5, i_knots=15, i_reg=0.1, prior="uniform"),
            "Flow": lambda: oracle.Model(D=2, n_layers=3, layer_kind="made", prior="normal", normal_offset=-0.5)}[name]()


WAVE = ["he", "he_gated", "left_dict", "d3_first", "d2_wide", "d5_wide"]
HEADS = ["MFlow", "IFlow", "Flow"]
_cache = {}


@pytest.fixture
def case(request, he_flat):
    """(name, params, model, x [B_BIG, D] on the device): built once per module run; the parameters are uploaded again per test (cheap, and
    a test may not rely on what another left on the device)."""
    import torch
    name = request.param
    if name not in _cache:
        params, psi, log_pdf, walkers = _build(name, he_flat)
        _cache[name] = (params, log_pdf.model, psi is not None, torch.as_tensor(walkers(B_BIG)).cuda())
    params, model, has_psi, x = _cache[name]
    model.ensure_params(params)
    return name, params, model, has_psi, x


def _ring_coefs(model, second_order):
    """NC of the sweep the entry runs (wf_internal.h: ring_coefs, rf_block, second_order_rf; no ring switch is set in the suite)."""
    if not second_order:
        return 1
    D, wide = model.D, max(model.i_nb, model.p_nb) > 32
    if wide and D > 4:
        return 3
    return (D if D <= 5 else (3 if D == 6 else 4)) + 2


def _column_sums_ok(jac, vjp, B, NC, what):
    """Both sides add the same fp32 products and differ in the order of the additions only: |diff_p| <= (B + NC) 2^-23 sum_b |jac[b][p]|
    (+ 1e-30).  Entries the VJP has exactly 0 (masked weights, zero_params of ungated models) are exactly 0 in every row."""
    jac64, vjp64 = jac.double().cpu().numpy(), vjp.double().cpu().numpy()
    assert jac64.shape == (B, vjp64.size) and np.isfinite(jac64).all() and np.isfinite(vjp64).all(), what
    diff = np.abs(jac64.sum(0) - vjp64)
    bound = (B + NC) * 2.0 ** -23 * np.abs(jac64).sum(0) + 1e-30
    worst = float((diff / bound).max())
    print(f"[column sums {what}] B {B} NC {NC}: worst |diff| / bound {worst:.3f}, zero columns {int((vjp64 == 0).sum())} of {vjp64.size}")
    assert (diff <= bound).all(), (what, worst, int(np.argmax(diff / bound)))
    assert (jac64[:, vjp64 == 0] == 0).all(), what
    assert np.abs(vjp64).max() > 0, what


# ---- 1. column sums equal the existing vector-Jacobian products

@pytest.mark.parametrize("B", [1, B_BIG])
@pytest.mark.parametrize("case", WAVE + HEADS, indirect=True)
def test_logpdf_jacobian_column_sums_equal_logpdf_vjp(case, B):
    import torch
    name, params, m, has_psi, x = case
    jac, lp = m.logpdf_jacobian(x[:B], return_logp=True)
    _column_sums_ok(jac, m.logpdf_vjp(x[:B], torch.ones(B)), B, 1, f"log_pdf {name}")
    assert torch.equal(lp, m.logpdf_loss_grad(x[:B], 1.0)[0])   # log_pdf of the same taped sweep


@pytest.mark.parametrize("B", [1, B_BIG])
@pytest.mark.parametrize("case", WAVE, indirect=True)
def test_psi_jacobian_column_sums_equal_psi_vjp(case, B):
    import torch
    name, params, m, has_psi, x = case
    g = torch.Generator().manual_seed(11)
    one, zero = torch.ones(B), torch.zeros(B)
    NC = _ring_coefs(m, True)
    for what, wp, wl in (("psi", one, zero), ("laplacian", zero, one), ("random", torch.randn(B, generator=g), torch.randn(B, generator=g))):
        _column_sums_ok(m.psi_jacobian(x[:B], wp, wl), m.psi_vjp(x[:B], wp, wl), B, NC, f"{what} {name}")
    # the defaults: w_psi = 1, w_lap = NULL (zeros)
    assert torch.equal(m.psi_jacobian(x[:B]), m.psi_jacobian(x[:B], one, zero))


# ---- 2. a row depends on its walker alone, bit for bit

def _raw_call(m, which, x, ws_bytes, w=None):
    """The C entry with a caller's workspace of ws_bytes (poisoned like every workspace of the suite)."""
    import torch
    from waveflow_amd import _lib
    L = _lib.lib()
    B = x.shape[0]
    jac = torch.full((B, m.n_params), float("nan"), device=x.device)
    ws = m._workspace(ws_bytes, x.device)
    if which == "logpdf":
        rc = L.wf_logpdf_jac(m._h, x.data_ptr(), B, jac.data_ptr(), None, ws.data_ptr(), ws.numel(), m._stream())
    else:
        rc = L.wf_psi_jac(m._h, x.data_ptr(), B, w[0].data_ptr(), w[1].data_ptr(), jac.data_ptr(), ws.data_ptr(), ws.numel(), m._stream())
    assert rc == 0, rc
    return jac


@pytest.mark.parametrize("case", WAVE + HEADS, indirect=True)
def test_rows_do_not_depend_on_the_batch_or_the_chunking(case):
    import torch
    from waveflow_amd import _lib
    L = _lib.lib()
    name, params, m, has_psi, x = case
    g = torch.Generator().manual_seed(12)
    w = (torch.randn(B_BIG, generator=g).cuda(), torch.randn(B_BIG, generator=g).cuda())
    for which in ("logpdf", "psi") if has_psi else ("logpdf",):
        full = m.logpdf_jacobian(x) if which == "logpdf" else m.psi_jacobian(x, *w)
        assert not torch.isnan(full).any(), (name, which)                      # WF_POISON: every entry was written
        again = m.logpdf_jacobian(x) if which == "logpdf" else m.psi_jacobian(x, *w)
        assert torch.equal(full, again), (name, which)
        for b in (0, 31, 32, 63, 64, 66):
            one = m.logpdf_jacobian(x[b:b + 1]) if which == "logpdf" else m.psi_jacobian(x[b:b + 1], w[0][b:b + 1], w[1][b:b + 1])
            assert torch.equal(one[0], full[b]), (name, which, b)
        # a workspace for 5 walkers: 14 chunks, the last of 2
        fn = L.wf_logpdf_jac_workspace_bytes if which == "logpdf" else L.wf_psi_jac_workspace_bytes
        small = fn(m._h, 5)
        assert small > 0 and small * B_BIG == fn(m._h, B_BIG) * 5   # (the tape of 5 of the 67 walkers)
        chunked = _raw_call(m, which, x, small, w)
        assert torch.equal(chunked, full), (name, which)


# ---- 3. rows against fp64 references

@pytest.fixture(scope="module")
def he_oracle_rows(golden, he_flat):
    """Reference rows of 8 He walkers from the fp64 autograd oracle, one walker with weight 1 per call: (x [8, 2], {"psi", "laplacian", "logpdf"} -> [8, n_params])."""
    import torch
    from oracle import energy_torch as et
    x = np.concatenate([np.sort(golden["he_golden"]["sample_points"], -1)[:4], sorted_walkers(4, 2, 8.0, 5)]).astype(np.float32)
    mo = et.he_model(torch.float64)
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    rows = {"psi": [], "laplacian": [], "logpdf": []}
    for b in range(8):
        xb = x[b:b + 1].astype(np.float64)
        rows["psi"].append(et.psi_vjp(mo, he_flat, xb, one, zero))
        rows["laplacian"].append(et.psi_vjp(mo, he_flat, xb, zero, one))
        rows["logpdf"].append(et.logpdf_vjp(mo, he_flat, xb, one))
    return x, {k: np.stack(v) for k, v in rows.items()}


@pytest.mark.parametrize("case", ["he"], indirect=True)
def test_rows_vs_autograd_oracle(case, he_oracle_rows):
    """A row is a B = 1 gradient: held to the yardsticks tests/test_gpu_grad.py applies to the contracted gradients of this model (psi and Laplacian:
    rel_l2 < 2e-3 and large entries within 5e-2, test_psi_vjp_vs_autograd_oracle; log_pdf: rel_l2 < 1e-3, test_logpdf_vjp_waveflow_vs_autograd_oracle)."""
    import torch
    name, params, m, has_psi, _ = case
    x, want = he_oracle_rows
    one, zero = torch.ones(8), torch.zeros(8)
    got = {"psi": m.psi_jacobian(x, one, zero), "laplacian": m.psi_jacobian(x, zero, one), "logpdf": m.logpdf_jacobian(x)}
    for what, bound in (("psi", 2e-3), ("laplacian", 2e-3), ("logpdf", 1e-3)):
        g = got[what].cpu().numpy().astype(np.float64)
        r = [rel_l2(g[b], want[what][b]) for b in range(8)]
        print(f"[rel_l2 rows {what}] measured " + " ".join(f"{v:.2e}" for v in r) + f" (bound {bound:g})")
        for b in range(8):
            assert ((want[what][b] == 0) <= (g[b] == 0)).all(), (what, b)
            assert r[b] < bound, (what, b, r[b])
            if what != "logpdf":
                big = np.abs(want[what][b]) > 1e-3 * np.abs(want[what][b]).max()
                assert np.abs(g[b][big] / want[what][b][big] - 1).max() < 5e-2, (what, b)


def _directional_check_row(row, flat, om, xb, seed, n_dirs=6, tol=2e-3):
    """tests/test_gpu_grad.py's _directional_check on one row: row . d vs central differences of the fp64 C oracle's log_pdf at that walker, along
    random parameter directions and directions confined to one block of leaves."""
    g = np.random.default_rng(seed)
    assert row.shape == flat.shape and np.isfinite(row).all() and np.abs(row).max() > 0
    F = lambda f: float(om.log_pdf(f.astype(np.float32), xb, f64=True).sum())
    for i in range(n_dirs):
        d = g.normal(size=flat.size)
        if i >= 2:
            lo = g.integers(0, flat.size - 64)
            mask = np.zeros(flat.size)
            mask[lo:lo + g.integers(16, 4096)] = 1
            d = d * mask
        d = (d / np.linalg.norm(d)).astype(np.float32)
        eps = 2e-3
        fd = (F(flat + eps * d) - F(flat - eps * d)) / (2 * eps)
        an = float(row @ d.astype(np.float64))
        scale = max(abs(fd), 1e-2 * np.linalg.norm(row) / np.sqrt(flat.size) * 10, 1e-6)
        print(f"[directional row] fd {fd:.6e} analytic {an:.6e}")
        assert abs(fd - an) <= tol * scale + 1e-4 * np.linalg.norm(row), (i, fd, an)


@pytest.mark.parametrize("case", HEADS, indirect=True)
def test_density_model_rows_vs_fp64_finite_differences(case):
    from waveflow_amd import flatten_params
    name, params, m, has_psi, x = case
    om = _oracle_head(name)
    flat = flatten_params(params)
    jac = m.logpdf_jacobian(x[:3]).cpu().numpy().astype(np.float64)
    xh = x[:3].cpu().numpy()
    for b in (0, 2):
        _directional_check_row(jac[b], flat, om, xh[b:b + 1], seed=40 + b)


# ---- 4. the pytree surface

@pytest.mark.parametrize("case", ["he", "he_gated"], indirect=True)
def test_closures_return_the_pytree_with_a_batch_axis(case, he_flat):
    import torch
    from waveflow_amd import core, vqmc
    name, params, m, has_psi, x = case
    _, psi, log_pdf, _ = _build(name, he_flat)   # closures of a model of the same description
    xb = x[:5]
    for make, rows in ((vqmc.log_pdf_jacobian, lambda mm: mm.logpdf_jacobian(xb)),
                       (vqmc.log_psi_jacobian, lambda mm: mm.psi_jacobian(xb) / (mm.psi(xb) + 1e-8)[:, None])):
        fn = make(log_pdf if make is vqmc.log_pdf_jacobian else psi)
        tree = fn(params, xb)
        want = rows(fn.model)
        leaves, tleaves = core.tree_leaves(tree), core.tree_leaves(params)
        assert [tuple(a.shape) for a in leaves] == [(5,) + tuple(np.shape(t)) for t in tleaves]
        assert torch.equal(torch.cat([a.reshape(5, -1) for a in leaves], 1), want)
        assert torch.isfinite(want).all() and want.abs().max() > 0


def test_a_jacobian_larger_than_the_free_memory_is_refused(he_flat):
    import torch
    params, psi, log_pdf, _ = _build("he", he_flat)
    m = psi.model
    m.ensure_params(params)
    B = 4_000_000   # 4e6 x 32 588 x 4 B = 521 GB: more than the card has
    need = B * m.n_params * 4
    assert need > torch.cuda.get_device_properties(0).total_memory
    x = torch.zeros(B, 2)   # (host: refused before anything is uploaded)
    for call in (m.logpdf_jacobian, m.psi_jacobian):
        with pytest.raises(ValueError, match=str(need)):
            call(x)


# ---- 5. refusals: the status of the VJP sibling

def test_abi_error_paths(he_flat):
    import torch
    from waveflow_amd import _lib, flows, model_factory
    L = _lib.lib()
    params, psi, log_pdf, _ = _build("he", he_flat)
    m = psi.model
    m.ensure_params(params)
    x = torch.as_tensor(sorted_walkers(8, 2, 5.0, 1)).cuda()
    w = torch.ones(8, device="cuda")
    g = torch.empty(m.n_params, device="cuda")
    jac = torch.empty(8, m.n_params, device="cuda")
    ws = torch.empty(int(L.wf_psi_jac_workspace_bytes(m._h, 8)), device="cuda", dtype=torch.uint8)
    X, W, G, J, S, n = x.data_ptr(), w.data_ptr(), g.data_ptr(), jac.data_ptr(), ws.data_ptr(), ws.numel()
    # the workspace is the tape of the wave sweeps: what the VJP entries ask for below the matrix-core switch point
    assert L.wf_psi_jac_workspace_bytes(m._h, 8) == L.wf_psi_vjp_workspace_bytes(m._h, 8) > 0
    assert L.wf_logpdf_jac_workspace_bytes(m._h, 8) == L.wf_logpdf_vjp_workspace_bytes(m._h, 8) > 0
    # each refusal next to its sibling's
    pairs = [
        (L.wf_psi_jac(None, X, 8, W, W, J, S, n, None), L.wf_psi_vjp(None, X, 8, W, W, G, S, n, None)),                  # no model
        (L.wf_psi_jac(m._h, None, 8, W, W, J, S, n, None), L.wf_psi_vjp(m._h, None, 8, W, W, G, S, n, None)),            # no walkers
        (L.wf_psi_jac(m._h, X, 8, None, W, J, S, n, None), L.wf_psi_vjp(m._h, X, 8, None, W, G, S, n, None)),            # no weights
        (L.wf_psi_jac(m._h, X, 8, W, W, None, S, n, None), L.wf_psi_vjp(m._h, X, 8, W, W, None, S, n, None)),            # no output
        (L.wf_psi_jac(m._h, X, 8, W, W, J, None, n, None), L.wf_psi_vjp(m._h, X, 8, W, W, G, None, n, None)),            # no workspace
        (L.wf_psi_jac(m._h, X, 8, W, W, J, S, 16, None), L.wf_psi_vjp(m._h, X, 8, W, W, G, S, 16, None)),                # not one walker fits
        (L.wf_psi_jac(m._h, X, -1, W, W, J, S, n, None), L.wf_psi_vjp(m._h, X, -1, W, W, G, S, n, None)),                # B < 0
        (L.wf_psi_jac(m._h, None, 0, None, None, J, None, 0, None), L.wf_psi_vjp(m._h, None, 0, None, None, G, None, 0, None)),   # B = 0: nothing to do
        (L.wf_logpdf_jac(None, X, 8, J, None, S, n, None), L.wf_logpdf_vjp(None, X, 8, W, G, S, n, None)),
        (L.wf_logpdf_jac(m._h, None, 8, J, None, S, n, None), L.wf_logpdf_vjp(m._h, None, 8, W, G, S, n, None)),
        (L.wf_logpdf_jac(m._h, X, 8, None, None, S, n, None), L.wf_logpdf_vjp(m._h, X, 8, W, None, S, n, None)),
        (L.wf_logpdf_jac(m._h, X, 8, J, None, None, n, None), L.wf_logpdf_vjp(m._h, X, 8, W, G, None, n, None)),
        (L.wf_logpdf_jac(m._h, X, 8, J, None, S, 16, None), L.wf_logpdf_vjp(m._h, X, 8, W, G, S, 16, None)),
        (L.wf_logpdf_jac(m._h, X, -1, J, None, S, n, None), L.wf_logpdf_vjp(m._h, X, -1, W, G, S, n, None)),
        (L.wf_logpdf_jac(m._h, None, 0, J, None, None, 0, None), L.wf_logpdf_vjp(m._h, None, 0, None, G, None, 0, None)),
        (L.wf_psi_jac_workspace_bytes(None, 8), L.wf_psi_vjp_workspace_bytes(None, 8)),
        (L.wf_psi_jac_workspace_bytes(m._h, -1), L.wf_psi_vjp_workspace_bytes(m._h, -1)),
        (L.wf_logpdf_jac_workspace_bytes(None, 8), L.wf_logpdf_vjp_workspace_bytes(None, 8)),
    ]
    assert [a for a, _ in pairs] == [b for _, b in pairs], pairs
    assert [a for a, _ in pairs] == [-1, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1], pairs
    # the Jacobian of psi needs the Waveflow prior, like wf_psi_vjp
    p2, lp2, _ = model_factory.get_model(n_flow_layers=1)(0, 2)
    lp2.model.ensure_params(p2)
    h2 = lp2.model._h
    assert L.wf_psi_jac_workspace_bytes(h2, 8) == L.wf_psi_vjp_workspace_bytes(h2, 8) == -2
    assert L.wf_psi_jac(h2, X, 8, W, W, J, S, n, None) == L.wf_psi_vjp(h2, X, 8, W, W, G, S, n, None) == -2
    # the coupling stack has no reverse sweep
    layer = lambda: flows.NeuralSplineCoupling(K=5, B=3, hidden_dim=8)
    p3, lp3, _ = flows.Flow(flows.Serial(layer(), flows.Reverse(), layer(), flows.Reverse()), flows.Normal(-0.25))(0, 2)
    lp3.model.ensure_params(p3)
    h3 = lp3.model._h
    assert L.wf_logpdf_jac_workspace_bytes(h3, 8) == L.wf_logpdf_vjp_workspace_bytes(h3, 8) == -2
    assert L.wf_logpdf_jac(h3, X, 8, J, None, S, n, None) == L.wf_logpdf_vjp(h3, X, 8, W, G, S, n, None) == -2
    with pytest.raises(_lib.WfError):
        lp3.model.logpdf_jacobian(x)
    with pytest.raises(ValueError):
        m.psi_jacobian(x, w_psi=torch.ones(7))
