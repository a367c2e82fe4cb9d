"""Stochastic reconfiguration on the device (include/waveflow_sr.h, waveflow_amd/sr.py, vqmc.sr_natural_gradient / train_step_sr / ModelTrainer.optimizer).

Synthetic rows against fp64 numpy on the same fp32 rows, each of the three entries on its own; the bad-pivot status; the He model: the P-space
equation matrix-free, the large-damping limit against the contracted gradient path (wf_psi_vjp), descent, the training step and the trainer.

Bounds (eps = 2^-53):
  gram    max |T - T_ref| <= 8 P eps max_b |row_b|^2: the products are exact, only the fp64 sums round (the centred matrix is that over B).
  solve   |y - y_ref| / |y_ref| <= 1e-12 B kappa, kappa = cond(T + lambda I) from numpy (<= B / 1e-3 + 1): the backward-error bound of an fp64
          Cholesky with a generous constant; and |L L^T - A| <= 2 (B + 1) eps max diag(A) (|L||L^T|_ij <= sqrt(a_ii a_jj)).
          B = 1: the centred 1 x 1 matrix is exactly 0 and so is a shift relative to its trace -- the documented outcome is info = 1 and y = NaN.
  apply   |out_p - ref_p| <= 2^-23 |ref_p| + 8 B eps |scale| sum_b |y_b - ybar| |r_bp|: one fp32 rounding plus the fp64 sum.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BS = [1, 15, 16, 67, 193]        # below, at and across a 16-row MFMA tile, across 64-row block tiles and 32-column Cholesky panels
PS = [3, 64, 1001]               # P < B: rank-deficient; 1001: no multiple of the K step (32), four 256-column chunks with a ragged last one
CASES = [(B, P, pad) for B in BS for P in PS for pad in (0, 5)] + [(67, 40000, 0)]   # 40 000 columns: 97 chunks of 416
_cache = {}


def _rows(B, P, pad):
    """fp32 normal rows [B, P] as a column slice of a contiguous [B, P + pad] matrix (NaN in the padding: reading it would show)."""
    import torch
    g = np.random.default_rng(1000 * B + P + pad)
    host = np.full((B, P + pad), np.nan, np.float32)
    host[:, :P] = g.normal(size=(B, P)).astype(np.float32)
    return host[:, :P].copy(), torch.as_tensor(host).cuda()[:, :P]


def _ws(B, P, shifted=False):
    """A poisoned workspace of the size the library asks for; `shifted`: at another address (256 bytes into a larger allocation)."""
    import torch
    from waveflow_amd import sr
    n = int(sr.lib().wf_sr_workspace_bytes(B, P))
    assert n > 0
    buf = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf[256:] if shifted else buf[:n]


def _case(B, P, pad):
    """Device results and fp64 numpy references of one synthetic case, computed once and shared by the tests below."""
    import torch
    from waveflow_amd import sr
    key = (B, P, pad)
    if key in _cache:
        return _cache[key]
    host, dev = _rows(B, P, pad)
    assert dev.stride(0) == P + pad and (B == 1 or (pad == 0) == dev.is_contiguous())
    g = np.random.default_rng(7 * B + P)
    O = host.astype(np.float64)
    H = np.eye(B) - np.ones((B, B)) / B
    c = {"dev": dev, "O": O, "H": H}
    # gram
    c["T"] = sr.gram(dev, workspace=_ws(B, P))
    c["T_ref"] = H @ (O @ O.T) @ H / B
    # solve, on the device's own matrix (the solve is judged on its own)
    A = c["T"].cpu().numpy()
    lam = 1e-3 * np.trace(A) / B
    rhs = H @ (g.normal(size=B) + 2.0)
    c["A"], c["lam"], c["rhs"] = A + lam * np.eye(B), lam, rhs
    c["rhs_dev"] = torch.as_tensor(rhs).cuda()
    c["L"] = c["T"].clone()
    c["y"], c["info"] = sr.solve(c["L"], c["rhs_dev"], 0.0, 1e-3, workspace=_ws(B, P))
    # apply, with a vector of its own
    yv = g.normal(size=B) + 0.5
    c["yv"], c["yv_dev"], c["scale"] = yv, torch.as_tensor(yv).cuda(), 2.0 / B
    c["out"] = sr.apply(dev, c["yv_dev"], c["scale"], workspace=_ws(B, P))
    torch.cuda.synchronize()
    _cache[key] = c
    return c


@pytest.mark.parametrize("B,P,pad", CASES)
def test_gram_vs_fp64_numpy(B, P, pad):
    c = _case(B, P, pad)
    T = c["T"].cpu().numpy()
    bound = 8 * P * EPS * (c["O"] ** 2).sum(1).max()
    err = np.abs(T - c["T_ref"]).max()
    rowsum = np.abs(T.sum(1)).max()
    print(f"[gram] B {B} P {P} ld {P + pad}: max err {err:.3e}, max |row sum| {rowsum:.3e}, bound {bound:.3e}")
    assert np.isfinite(T).all() and T.shape == (B, B)
    assert err <= bound
    assert np.array_equal(T, T.T)            # exactly symmetric, bit for bit
    assert rowsum <= bound                   # H 1 = 0: the rows of the centred matrix sum to zero in exact arithmetic


@pytest.mark.parametrize("B,P,pad", CASES)
def test_solve_vs_fp64_numpy(B, P, pad):
    c = _case(B, P, pad)
    info, y = int(c["info"].item()), c["y"].cpu().numpy()
    if B == 1:   # T = [0] exactly and lambda = 1e-3 * 0: no positive pivot (see the module docstring)
        assert c["T"].item() == 0.0 and info == 1 and np.isnan(y).all()
        return
    assert info == 0 and np.isfinite(y).all()
    A = c["A"]
    kappa = np.linalg.cond(A)
    assert kappa <= B / 1e-3 + 1 + 1e-6 * B / 1e-3
    y_ref = np.linalg.solve(A, c["rhs"])
    rel = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
    L = np.tril(c["L"].cpu().numpy())
    fact = np.abs(L @ L.T - A).max()
    print(f"[solve] B {B} P {P} ld {P + pad}: kappa {kappa:.3e} rel err {rel:.3e} (bound {1e-12 * B * kappa:.3e}), |L L^T - A| {fact:.3e}")
    assert rel <= 1e-12 * B * kappa
    assert fact <= 2 * (B + 1) * EPS * np.diag(A).max()
    assert np.array_equal(np.triu(c["L"].cpu().numpy(), 1), np.triu(c["T"].cpu().numpy(), 1))   # the strict upper triangle is left alone


@pytest.mark.parametrize("B,P,pad", CASES)
def test_apply_vs_fp64_numpy(B, P, pad):
    c = _case(B, P, pad)
    out = c["out"].cpu().numpy().astype(np.float64)
    yc = c["yv"] - c["yv"].mean()
    ref = c["scale"] * (yc @ c["O"])
    bound = 2.0 ** -23 * np.abs(ref) + 8 * B * EPS * c["scale"] * (np.abs(yc) @ np.abs(c["O"]))
    worst = float((np.abs(out - ref) / np.maximum(bound, 1e-300)).max()) if B > 1 else 0.0
    print(f"[apply] B {B} P {P} ld {P + pad}: worst |err| / bound {worst:.3f}")
    assert out.shape == (P,) and np.isfinite(out).all()
    assert (np.abs(out - ref) <= bound).all()


@pytest.mark.parametrize("B,P,pad", [(193, 1001, 0), (193, 1001, 5), (67, 40000, 0), (16, 3, 0)])
def test_results_are_bitwise_repeatable_and_do_not_depend_on_the_workspace_address(B, P, pad):
    import torch
    from waveflow_amd import sr
    c = _case(B, P, pad)
    for shifted in (False, True):
        ws = _ws(B, P, shifted)
        T = sr.gram(c["dev"], workspace=ws)
        assert torch.equal(T, c["T"])
        y, info = sr.solve(T, c["rhs_dev"], 0.0, 1e-3, workspace=ws)
        assert torch.equal(y, c["y"]) and torch.equal(T, c["L"]) and int(info.item()) == 0
        assert torch.equal(sr.apply(c["dev"], c["yv_dev"], c["scale"], workspace=ws), c["out"])


def test_natural_gradient_is_the_three_calls_and_matches_the_p_space_solution():
    """sr.natural_gradient on synthetic rows (B = 67, P = 64: S is 64 x 64, solved directly in fp64 numpy)."""
    import torch
    from waveflow_amd import sr
    c = _case(67, 64, 0)
    B, O, H = 67, c["O"], c["H"]
    e = np.random.default_rng(3).normal(size=B).astype(np.float32) - 2.5
    d = sr.natural_gradient(c["dev"], torch.as_tensor(e).cuda()).cpu().numpy().astype(np.float64)
    lam = 1e-3 * np.trace(c["T_ref"]) / B
    ref = np.linalg.solve(O.T @ H @ O / B + lam * np.eye(64), 2.0 / B * O.T @ H @ e.astype(np.float64))
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    print(f"[natural gradient, synthetic] rel. error vs the P-space solve {rel:.3e}")
    assert rel <= 2.0 ** -23 + 1e-12 * B * (B / 1e-3 + 1)   # one fp32 rounding of d, and the solve's bound


# ---- a pivot that is not positive is a status, not a fault

@pytest.mark.parametrize("B,bad", [(16, 1), (67, 41)])
def test_bad_pivot_gives_info_and_nan(B, bad):
    import torch
    from waveflow_amd import sr
    L = sr.lib()
    T = torch.eye(B, dtype=torch.float64, device="cuda")
    if bad == 1:
        T = -T
    else:
        T[bad - 1, bad - 1] = -1.0   # in the second panel: the first one factors
    rhs = torch.ones(B, dtype=torch.float64, device="cuda")
    y = torch.zeros(B, dtype=torch.float64, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = _ws(B, 1)
    rc = L.wf_sr_solve(T.data_ptr(), B, rhs.data_ptr(), 0.0, 0.0, y.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and L.wf_last_hip_error() == 0
    assert int(info.item()) == bad and bool(torch.isnan(y).all())


def test_natural_gradient_raises_not_positive_definite():
    import torch
    from waveflow_amd import sr
    rows = torch.zeros(16, 8, device="cuda")   # T = 0 and a shift relative to its trace: pivot 1 is 0
    with pytest.raises(sr.NotPositiveDefinite, match="pivot 1") as ei:
        sr.natural_gradient(rows, torch.ones(16, device="cuda"))
    assert ei.value.pivot == 1
    assert bool(torch.isfinite(sr.natural_gradient(rows, torch.ones(16, device="cuda"), damping=1e-3)).all())   # an absolute shift: d = 0


# ---- the He model (the recipe and the walkers of tests/test_gpu_param_jacobian.py)

B_HE = 67
# (a) residual of the P-space equation, (b) rel. l2 of lambda d against the contracted gradient: measured values and their bounds in DESIGN.md 4.18
BOUND_RESIDUAL = 1e-5
# (b) has no measured value yet: until it has, the bound is the one the arithmetic gives -- B * 1e-6 from the damping itself
# (|lambda (S + lambda)^-1 g - g| <= |g| trace(S) / lambda, lambda = 1e6 trace / B) plus the fp32 contraction of wf_psi_vjp against the exact
# column sums, (B + NC + 2) 2^-23 sum_b |w_b| |row_b| (tests/test_gpu_param_jacobian.py: _column_sums_ok, NC = 4 for He; + 2: the fp32
# weights and the fp32 result), taken in the l2 norm relative to the gradient.  Once measured, the rule is 3 x the measured value.
BOUND_LIMIT = None


def _waveflow(D, k, knots, layers, box, kind="mean", seed=7):
    from waveflow_amd import model_factory
    init = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                            i_spline_reg=0.05, n_flow_layers=layers, box_size=box, xu_coord_type=kind)
    return init(seed, D)


def _he(he_flat):
    """(params, psi, h_fn, x [67, 2] on the device); one model per module run."""
    import torch
    from waveflow_amd import checkpoint
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        params, psi, log_pdf, _ = _waveflow(2, 6, 23, 3, 10.0)
        params = checkpoint.unflatten_like(params, he_flat)
        protons, _ = physics.system_catalogue[1]["He"]
        h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
        _cache["he"] = (params, psi, h_fn, torch.as_tensor(sorted_walkers(B_HE, 2, 8.0, 5)).cuda())
    params, psi, h_fn, x = _cache["he"]
    psi.model.ensure_params(params)
    return params, psi, h_fn, x


def _he_terms(he_flat):
    """fp64 numpy O, e and g of the He walkers from the device rows and energies (the very tensors sr_natural_gradient feeds the solver)."""
    from waveflow_amd import vqmc
    params, psi, h_fn, x = _he(he_flat)
    model, xd, hpsi, ps, _ = vqmc._energy_terms(params, psi, h_fn, x)
    inv = 1.0 / (ps + 1e-8)
    e32 = hpsi * inv
    rows = model.psi_jacobian(xd, w_psi=inv)
    O, e = rows.double().cpu().numpy(), e32.double().cpu().numpy()
    ec = e - e.mean()
    g = 2.0 / B_HE * (O.T @ ec)
    return rows, e32, O, e, g


def _centred(O, v):
    """O^T H (O v) / B without the P x P matrix."""
    t = O @ v
    return O.T @ (t - t.mean()) / O.shape[0]


def test_he_natural_gradient_solves_the_p_space_equation(he_flat):
    """(a) |S d + lambda d - g| / |g| with S = O^T H O / B applied matrix-free in fp64, (c) g . d > 0, and the loss is the mean local energy."""
    from waveflow_amd import sr, vqmc
    params, psi, h_fn, x = _he(he_flat)
    rows, e32, O, e, g = _he_terms(he_flat)
    d32, loss = vqmc.sr_natural_gradient(params, psi, h_fn, x)
    d = d32.double().cpu().numpy()
    Oc = O - O.mean(0)
    trace = (Oc * Oc).sum() / B_HE            # trace(H O O^T H / B)
    lam = 1e-3 * trace / B_HE
    res = np.linalg.norm(_centred(O, d) + lam * d - g) / np.linalg.norm(g)
    print(f"[He, P-space residual] measured {res:.3e} (bound {BOUND_RESIDUAL:g}); lambda {lam:.3e}, |d| {np.linalg.norm(d):.3e}, g.d {g @ d:.3e}, loss {loss:.6f}")
    assert d.shape == (psi.model.n_params,) and np.isfinite(d).all()
    assert abs(loss - e.mean()) <= 1e-6 * max(1.0, abs(e.mean()))
    assert g @ d > 0                          # a descent direction
    assert res <= BOUND_RESIDUAL


def test_he_large_damping_limit_is_the_contracted_gradient(he_flat):
    """(b) lambda d -> g for lambda >> S: g from code this feature does not touch (wf_psi_vjp with w_psi = 2 (e_b - ebar) / (B (psi_b + 1e-8)))."""
    import torch
    from waveflow_amd import sr, vqmc
    params, psi, h_fn, x = _he(he_flat)
    rows, e32, O, e, g = _he_terms(he_flat)
    model, xd, hpsi, ps, _ = vqmc._energy_terms(params, psi, h_fn, x)
    trace = float(torch.diagonal(sr.gram(rows)).sum())
    damping = 1e6 * trace / B_HE
    d32, _ = vqmc.sr_natural_gradient(params, psi, h_fn, x, damping=damping, relative_damping=0.0)
    ec = torch.as_tensor(e - e.mean(), dtype=torch.float64, device=ps.device)
    w_psi = (2.0 * ec / (B_HE * (ps.double() + 1e-8))).float()
    want = model.psi_vjp(xd, w_psi, torch.zeros(B_HE)).double().cpu().numpy()
    got = damping * d32.double().cpu().numpy()
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    rel_g = np.linalg.norm(got - g) / np.linalg.norm(g)
    spread = np.linalg.norm((2.0 / B_HE * np.abs(e - e.mean())) @ np.abs(O)) / np.linalg.norm(g)
    bound = BOUND_LIMIT if BOUND_LIMIT is not None else B_HE * 1e-6 + (B_HE + 4 + 2) * 2.0 ** -23 * spread
    print(f"[He, large-damping limit] measured rel. l2 vs wf_psi_vjp {rel:.3e}, vs the fp64 column sums of the rows {rel_g:.3e} (bound {bound:.3e}, "
          f"sum |w||row| over |g| {spread:.2f})")
    assert rel <= bound


def test_he_train_step_sr_returns_new_parameters_and_leaves_the_old_ones(he_flat):
    """(d) the result is shaped like `params`, `params` is untouched, and the model follows whichever tree it is asked about."""
    import torch
    from waveflow_amd import core, vqmc
    params, psi, h_fn, x = _he(he_flat)
    before = core.flatten_params(params).copy()
    d32, _ = vqmc.sr_natural_gradient(params, psi, h_fn, x)
    new, loss = vqmc.train_step_sr(1, psi, h_fn, params, x, 1e-2)
    assert np.array_equal(core.flatten_params(params), before)
    shapes = lambda t: [tuple(np.shape(a)) for a in core.tree_leaves(t)]
    assert shapes(new) == shapes(params) and np.isfinite(loss)
    want = before - np.float32(1e-2) * d32.cpu().numpy()
    assert np.array_equal(core.flatten_params(new), want) and not np.array_equal(want, before)
    # a fresh model of the same description, given the new parameters, agrees bit for bit; and the old tree still gives the old values
    p2, psi2, _, _ = _waveflow(2, 6, 23, 3, 10.0)
    assert torch.equal(psi(new, x), psi2(new, x))
    assert torch.equal(psi(params, x), psi2(params, x)) and not torch.equal(psi(new, x), psi(params, x))
    # device-resident parameters: a new DeviceParams, the old vector untouched
    flat = torch.as_tensor(before).cuda()
    dp = core.DeviceParams(params, flat, 0)
    new_dp, _ = vqmc.train_step_sr(1, psi, h_fn, dp, x, 1e-2)
    assert isinstance(new_dp, core.DeviceParams) and new_dp.flat is not flat and torch.equal(flat.cpu(), torch.as_tensor(before))
    assert torch.equal(psi(new_dp, x), psi2(new, x))


def test_model_trainer_with_sr_runs_and_adam_is_unchanged(tmp_path):
    """(e) optimizer='sr': three eager steps, the reference's artefacts on disk.  optimizer='adam' (the default): the losses of a trainer that
    never heard of the attribute."""
    from waveflow_amd import vqmc

    def trainer(name):
        t = vqmc.ModelTrainer(system_name="He", learning_rate=1e-3, box_length=10, num_epochs=3, batch_size=64)
        t.save_dir = str(tmp_path / name)
        return t

    t = trainer("sr")
    t.optimizer = 'sr'
    params, loss = t.start_training(verbose=False)
    assert len(loss[1:]) == 3 and np.isfinite(np.asarray(loss[1:], dtype=np.float64)).all()
    for f in ("checkpoints", "loss.npy", "energies.npy", "system_info.json", "outputs/wavefunctions_2d/values_epoch1.npy",
              "outputs/sample_points/values_epoch1.npy", "outputs/density_1e/onproton_values_epoch1.npy"):
        assert os.path.exists(os.path.join(t.save_dir, f)), f
    assert not os.path.exists(os.path.join(t.save_dir, "optimizer_state.npz"))   # there are no Adam moments to save
    a = trainer("adam")
    assert a.optimizer == 'adam'
    _, loss_a = a.start_training(verbose=False)
    b = trainer("plain")
    del b.optimizer, b.sr_damping
    _, loss_b = b.start_training(verbose=False)
    assert len(loss_a) == 4 and loss_a == loss_b
    assert loss_a[1:] != loss[1:]
