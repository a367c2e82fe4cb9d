"""The matrix-free solve of stochastic reconfiguration on the GPU (include/waveflow_sr_cg.h; sr.solve_cg, solver='cg' of sr.natural_gradient /
sr.spring_direction and of the vqmc steps).  Inputs are synthetic fp32 rows (normal entries, column scales exp(N(0, 0.5)), column offsets) in a
wider matrix whose padding is NaN, unless the test names He; relative_damping = 1e-2, tol = 1e-8.

Bounds.  With A = Tbar + lambda I, kappa its condition number (numpy.linalg.eigvalsh of the dense fp64 matrix for B <= 1024, B / relative_damping
beyond: lambda >= relative_damping trace / B >= relative_damping lambda_max / B), eps = 2.2e-16 and n_it the iterations `info` reports:

  true residual   |A y - rhs| / |rhs| <= tol + C eps kappa n_it.  The recurrence's residual is <= tol at status 0; what the true one adds is the
                  drift between the two.  sr.cg_reference, run in fp64 on the inputs of every case below with both `precondition` values and
                  with tol 1e-8 and 1e-13, shows a largest drift, over every iteration of every run, of 2.8e-3 eps kappa n_it (this module's
                  _measure_reference_drift()); the device sums in another order and gets the factor 4: C = 1.1e-2.
  solution        |y - y*| / |y*| <= kappa * (that residual): |y - y*| <= |A^-1| |A y - rhs| and |rhs| <= |A| |y*|.  y* by numpy in fp64 (the
                  dense solve for B <= 1024, the P x P form of the same system beyond), itself good to 8 B eps kappa, which the test adds.
  directions      d = mu prev + (2 / B) O^T H y is linear in y with |(2 / B) O^T H| = (2 / B) sqrt(B lambda_max(Tbar)), so
                  |d_cg - d_chol| <= (2 / B) sqrt(B lambda_max) (|y_cg - y*| + |y_chol - y*|) + 2 * 2^-24 |d|   (two fp32 roundings),
                  |y_cg - y*| <= (tol + C eps kappa n_it) |rhs| / lambda_min(A), and for the dense path 8 (B + P) eps kappa |y*|: Cholesky's backward
                  error (Higham, Accuracy and Stability, thm. 10.4: of order B eps |A|) and the Gram sums' (P eps |Tbar|), through kappa.
  parameters      theta' = fl32(theta - lr d): lr times the direction bound plus 2^-23 (|theta| + lr |d|).
  iterations      within 2 of sr.cg_reference at the same tol where that takes at most 100 iterations, within 10 % beyond.  Within 2 does not
                  hold for the long runs even between two fp64 NumPy runs of the same recurrences: with rows and columns of the inputs permuted
                  (the same system, other orders of summation) cg_reference takes 288 .. 305 iterations at (1024, 333) and 282 .. 294 at
                  (5000, 129) with the Jacobi preconditioner -- P < B there, Tbar has rank P, the preconditioner spreads the one cluster at
                  lambda, and once the Lanczos vectors have lost orthogonality rounding decides how long the last eigenvalues take: 6 % spread.
                  The runs of at most 150 iterations moved by at most one iteration under the same permutations.
"""
import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
C_DRIFT = 1.1e-2          # 4 x the 2.76e-3 measured on sr.cg_reference (module docstring)
TOL = 1e-8
REL = 1e-2
# (B, P, ld): ld > P; 132 / 260 / 336 keep 16-byte loads with an unaligned tail (P = 129, 257, 333), 7 and 1002 take the 4-byte path
CASES = [(1, 1, 4), (2, 5, 7), (67, 257, 260), (300, 1000, 1002), (1024, 333, 336), (5000, 129, 132)]
B_HE = 512
_cache = {}


def _inputs(B, P):
    """(rows fp32 [B, P], rhs fp64 [B] centred, damping) on the host."""
    g = np.random.default_rng(77 * B + P)
    rows = (g.normal(size=(B, P)) * np.exp(0.5 * g.normal(size=P)) + 0.3 * g.normal(size=P)).astype(np.float32)
    rhs = g.normal(size=B)
    rhs -= rhs.mean()
    if B == 1:
        return rows, np.array([0.7]), 1e-3     # Tbar = 0: the shift is the absolute damping, y = rhs / lambda
    return rows, rhs, 0.0


def _measure_reference_drift():
    """The figure in the module docstring: max over cases, `precondition`, tol and iterations of |true - recursive residual| / (eps kappa n_it)."""
    from waveflow_amd import sr
    worst = 0.0
    for B, P, _ in CASES:
        rows, rhs, damping = _inputs(B, P)
        kappa = _spectrum(rows.astype(np.float64), damping)[3]
        for pre in (True, False):
            for tol in (1e-8, 1e-13):
                _, info, steps = sr.cg_reference(rows, rhs, damping=damping, relative_damping=REL, tol=tol, precondition=pre, history=True)
                for it, (rec, true) in enumerate(steps, 1):
                    worst = max(worst, abs(true - rec) / (EPS * kappa * it))
                print(f"B {B} P {P} precondition {pre} tol {tol:g}: {int(info[1])} iterations, status {int(info[0])}, kappa {kappa:.3e}, worst so far {worst:.3e}")
    return worst


def _spectrum(O, damping):
    """-> (lambda, lambda_max(Tbar), lambda_min(A), kappa(A)): eigvalsh of the dense matrix for B <= 1024, the bounds of the docstring beyond."""
    B = O.shape[0]
    Oc = O - O.mean(0)
    lam = damping + REL * (Oc ** 2).sum() / B / B
    if B <= 1024:
        w = np.linalg.eigvalsh(Oc @ Oc.T / B)
        top, low = float(w.max()), max(float(w.min()), 0.0)
        return lam, top, low + lam, (top + lam) / (low + lam)
    top = float(np.linalg.eigvalsh(Oc.T @ Oc / B).max())     # (the same non-zero spectrum, P x P)
    return lam, top, lam, B / REL


def _dense_solution(O, rhs, lam):
    B, P = O.shape
    Oc = O - O.mean(0)
    if B <= 1024:
        return np.linalg.solve(Oc @ Oc.T / B + lam * np.eye(B), rhs)
    # (Oc Oc^T / B + lam I)^-1 rhs = (rhs - Oc (Oc^T Oc / B + lam I)^-1 Oc^T rhs / B) / lam
    return (rhs - Oc @ np.linalg.solve(Oc.T @ Oc / B + lam * np.eye(P), Oc.T @ rhs) / B) / lam


def _device_rows(host, ld):
    import torch
    B, P = host.shape
    wide = np.full((B, ld), np.nan, np.float32)      # NaN in the padding: reading it would show
    wide[:, :P] = host
    return torch.as_tensor(wide).cuda()[:, :P]


def _case(B, P, ld):
    import torch
    key = (B, P)
    if key not in _cache:
        host, rhs, damping = _inputs(B, P)
        O = host.astype(np.float64)
        c = {"host": host, "O": O, "rhs": rhs, "damping": damping, "dev": _device_rows(host, ld), "rhs_dev": torch.as_tensor(rhs).cuda()}
        c["lam"], c["top"], c["low"], c["kappa"] = _spectrum(O, damping)
        c["want"] = _dense_solution(O, rhs, c["lam"])
        _cache[key] = c
    return _cache[key]


def _solved(B, P, ld, pre):
    """solve_cg of one case, once: (case, y numpy, info numpy, y tensor, info tensor)"""
    import torch
    from waveflow_amd import sr
    c = _case(B, P, ld)
    if ("solved", pre) not in c:
        y, info = sr.solve_cg(c["dev"], c["rhs_dev"], damping=c["damping"], relative_damping=REL, tol=TOL, precondition=pre)
        torch.cuda.synchronize()
        c[("solved", pre)] = (y.cpu().numpy(), info.cpu().numpy(), y, info)
    return (c,) + c[("solved", pre)]


def _apply_a(O, lam, y):
    B = O.shape[0]
    z = O.T @ (y - y.mean())
    q = O @ z
    return (q - q.mean()) / B + lam * y


@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("B,P,ld", CASES)
def test_true_residual_solution_and_iteration_count(B, P, ld, pre):
    """Checks 1 and 3 of the module docstring: the residual NumPy forms matrix-free from the returned y, the distance to the dense solution,
    lambda, and the iteration count against sr.cg_reference."""
    from waveflow_amd import sr
    c, y, info, _, _ = _solved(B, P, ld, pre)
    status, n_it, rec, lam = info
    assert status == 0 and np.isfinite(y).all() and y.shape == (B,)
    assert abs(lam - c["lam"]) <= 1e-12 * c["lam"]
    res = np.linalg.norm(_apply_a(c["O"], c["lam"], y) - c["rhs"]) / np.linalg.norm(c["rhs"])
    bound = TOL + C_DRIFT * EPS * c["kappa"] * max(n_it, 1)
    err = np.linalg.norm(y - c["want"]) / np.linalg.norm(c["want"])
    _, ref_info = sr.cg_reference(c["host"], c["rhs"], damping=c["damping"], relative_damping=REL, tol=TOL, precondition=pre)
    print(f"[cg] B {B} P {P} ld {ld} precondition {pre}: {int(n_it)} iterations (reference {int(ref_info[1])}), kappa {c['kappa']:.3e}, recurrence "
          f"{rec:.3e}, true residual {res:.3e} (bound {bound:.3e}), drift {abs(res - rec) / (EPS * c['kappa'] * max(n_it, 1)):.2e} eps kappa n_it, "
          f"|y - y*| / |y*| {err:.3e} (bound {c['kappa'] * res:.3e})")
    assert rec <= TOL
    assert res <= bound
    assert err <= c["kappa"] * res + 8 * B * EPS * c["kappa"]
    assert ref_info[0] == 0 and abs(int(n_it) - int(ref_info[1])) <= (2 if ref_info[1] <= 100 else int(0.1 * ref_info[1]))
    if B == 1:
        assert n_it == 0 and y[0] == c["rhs"][0] / lam


def _direction_bound(c, rhs, y_star, d, n_it):
    B, P = c["O"].shape
    dy_cg = (TOL + C_DRIFT * EPS * c["kappa"] * max(n_it, 1)) * np.linalg.norm(rhs) / c["low"]
    dy_dense = 8 * (B + P) * EPS * c["kappa"] * np.linalg.norm(y_star)
    return 2.0 / B * np.sqrt(B * c["top"]) * (dy_cg + dy_dense) + 2 * 2.0 ** -24 * np.linalg.norm(d)


@pytest.mark.parametrize("B,P,ld", [k for k in CASES if 1 < k[0] <= 1024])
def test_directions_against_the_dense_path(B, P, ld):
    """Check 2: natural_gradient and spring_direction (momentum 0.9, clip 5) with solver='cg' against solver='cholesky' on the same rows."""
    import torch
    from waveflow_amd import sr
    c = _case(B, P, ld)
    g = np.random.default_rng(B + P)
    e = torch.as_tensor((g.normal(size=B) + 3.0).astype(np.float32)).cuda()
    prev = torch.as_tensor((1e-2 * g.normal(size=P)).astype(np.float32)).cuda()
    for name, mu in (("natural_gradient", 0.0), ("spring_direction", 0.9)):
        if mu == 0.0:
            dense = sr.natural_gradient(c["dev"], e, relative_damping=REL)
            got = sr.natural_gradient(c["dev"], e, relative_damping=REL, solver="cg", tol=TOL)
            r = e.double()
        else:
            dense = sr.spring_direction(c["dev"], e, prev, mu, relative_damping=REL, clip=5.0)
            got = sr.spring_direction(c["dev"], e, prev, mu, relative_damping=REL, clip=5.0, solver="cg", tol=TOL)
            r = sr.clip_local_energies(e, 5.0) - (0.5 * mu) * sr.matvec(c["dev"], prev)
        rhs = r - r.mean()
        _, info = sr.solve_cg(c["dev"], rhs, relative_damping=REL, tol=TOL, precondition=False)      # the solve the direction made: its iteration count
        rhs = rhs.cpu().numpy()
        lam = _spectrum(c["O"], 0.0)[0]
        y_star = _dense_solution(c["O"], rhs, lam)
        d = dense.double().cpu().numpy()
        diff = np.linalg.norm(got.double().cpu().numpy() - d)
        bound = _direction_bound(c, rhs, y_star, d, info.cpu().numpy()[1])
        print(f"[{name}] B {B} P {P}: |d_cg - d_cholesky| / |d| {diff / np.linalg.norm(d):.3e} (bound {bound / np.linalg.norm(d):.3e})")
        assert got.dtype == torch.float32 and got.shape == (P,) and bool(torch.isfinite(got).all())
        assert diff <= bound


def _raw(c, rhs_dev, n_iter, restart, pre=True, tol=1e-13, y=None, info=None, ws=None):
    """One wf_sr_cg_solve through sr._cg_call -> (y, info, workspace), allocated here unless given."""
    import torch
    from waveflow_amd import sr
    dev = c["dev"]
    B, P, ld = sr._check_rows(dev)
    y = torch.full((B,), 7.0, dtype=torch.float64, device="cuda") if y is None else y
    info = torch.full((4,), 7.0, dtype=torch.float64, device="cuda") if info is None else info
    ws = sr._cg_workspace(B, P, dev.device).clone() if ws is None else ws
    sr._cg_call(dev, B, P, ld, rhs_dev, c["damping"], REL, tol, n_iter, restart, pre, y, info, ws)
    return y, info, ws


def _bits(t):
    import torch
    return t.view(torch.int64)


@pytest.mark.parametrize("B,P,ld", [(67, 257, 260), (300, 1000, 1002), (5000, 129, 132)])
def test_bitwise_repeatable_and_resumable(B, P, ld):
    """Check 4: two calls give the same bits; 64 iterations in one call equal 32 and 32 more (restart, then continue)."""
    import torch
    from waveflow_amd import sr
    c = _case(B, P, ld)
    _, _, _, y0, info0 = _solved(B, P, ld, True)
    y1, info1 = sr.solve_cg(c["dev"], c["rhs_dev"], damping=c["damping"], relative_damping=REL, tol=TOL, precondition=True)
    assert torch.equal(_bits(y1), _bits(y0)) and torch.equal(_bits(info1), _bits(info0))
    ya, ia, _ = _raw(c, c["rhs_dev"], 64, 1)
    yb, ib, wsb = _raw(c, c["rhs_dev"], 32, 1)
    half = ib.cpu().numpy().copy()
    _raw(c, c["rhs_dev"], 32, 0, y=yb, info=ib, ws=wsb)
    torch.cuda.synchronize()
    assert half[1] == 32 or half[0] == 0
    assert torch.equal(_bits(ya), _bits(yb)) and torch.equal(_bits(ia), _bits(ib))


def test_finished_solve_ignores_further_calls():
    """Check 5: after status 0 a continuing call changes no byte of y, info or the workspace."""
    import torch
    c = _case(300, 1000, 1002)
    y, info, ws = _raw(c, c["rhs_dev"], 200, 1, tol=TOL)
    torch.cuda.synchronize()
    assert info.cpu().numpy()[0] == 0 and 0 < info.cpu().numpy()[1] < 200
    y0, info0, ws0 = y.clone(), info.clone(), ws.clone()
    _raw(c, c["rhs_dev"], 16, 0, tol=TOL, y=y, info=info, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y0)) and torch.equal(_bits(info), _bits(info0)) and torch.equal(ws, ws0)
    # and a tighter tolerance does not wake it: finished is finished until a restart
    _raw(c, c["rhs_dev"], 4, 0, tol=1e-13, y=y, info=info, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y0)) and torch.equal(ws, ws0)


def test_edge_states():
    """Check 6: a zero right-hand side; a NaN row; max_iter = 1."""
    import torch
    from waveflow_amd import sr
    c = _case(300, 1000, 1002)
    y, info = sr.solve_cg(c["dev"], torch.zeros(300, dtype=torch.float64, device="cuda"), relative_damping=REL)
    assert not bool(y.any()) and info.cpu().tolist()[:3] == [0.0, 0.0, 0.0] and abs(info.cpu().numpy()[3] - c["lam"]) <= 1e-12 * c["lam"]
    bad = c["host"].copy()
    bad[17, 333] = np.nan
    cb = {"dev": _device_rows(bad, 1002), "damping": 0.0}
    yb, ib, _ = _raw(cb, c["rhs_dev"], 8, 1)
    torch.cuda.synchronize()
    assert ib.cpu().numpy()[0] == 2 and bool(torch.isnan(yb).all())
    with pytest.raises(sr.NotFinite):
        sr.solve_cg(cb["dev"], c["rhs_dev"], relative_damping=REL)
    with pytest.raises(ArithmeticError):
        sr.natural_gradient(cb["dev"], c["rhs_dev"].float(), relative_damping=REL, solver="cg")
    with pytest.raises(sr.NotConverged, match=r"\|r\| / \|rhs\| = \d\.\d{3}e[-+]\d\d after 1 iterations") as ei:
        sr.solve_cg(c["dev"], c["rhs_dev"], relative_damping=REL, tol=TOL, max_iter=1)
    assert ei.value.iterations == 1 and TOL < ei.value.residual < 10.0      # (the 2-norm of a preconditioned residual need not fall in a step)
    # rounds: the same bits whatever the round length, and max_iter is honoured when it is no multiple of it
    _, _, _, y0, info0 = _solved(300, 1000, 1002, True)
    y7, info7 = sr.solve_cg(c["dev"], c["rhs_dev"], relative_damping=REL, tol=TOL, round_iters=7, precondition=True)
    assert torch.equal(_bits(y7), _bits(y0)) and torch.equal(_bits(info7), _bits(info0))
    with pytest.raises(sr.NotConverged) as ei:
        sr.solve_cg(c["dev"], c["rhs_dev"], relative_damping=REL, tol=1e-13, max_iter=5, round_iters=3)
    assert ei.value.iterations == 5


@pytest.mark.parametrize("B,P,ld", [(67, 257, 260), (300, 1000, 1002)])
def test_captured_solve_replays_bit_for_bit(B, P, ld):
    """Check 7: restart = 1, n_iter = 48 captured once and replayed on two right-hand sides equals the eager calls.  (67, 257) converges inside
    the 48 iterations (the tail of the captured sequence returns at once), (300, 1000) does not."""
    import torch
    c = _case(B, P, ld)
    g = np.random.default_rng(3)
    sides = []
    for _ in range(2):
        r = g.normal(size=B)
        sides.append(torch.as_tensor(r - r.mean()).cuda())
    eager = [_raw(c, r, 48, 1, tol=TOL)[:2] for r in sides]       # (also the warm call outside the capture)
    rhs = sides[0].clone()
    y, info, ws = _raw(c, rhs, 1, 1, tol=TOL)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            _raw(c, rhs, 48, 1, tol=TOL, y=y, info=info, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    for r, (ye, ie) in zip(sides, eager):
        rhs.copy_(r)
        y.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(ye)) and torch.equal(_bits(info), _bits(ie))
        status, n_it = ie.cpu().numpy()[:2]
        print(f"[capture] B {B} P {P}: status {int(status)} after {int(n_it)} iterations")
        assert (status == 0 and n_it < 48) if B == 67 else (status == 1 and n_it == 48)


def _he(he_flat):
    from waveflow_amd import checkpoint, model_factory
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        init = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
        params, psi, _, _ = init(0, 2)
        params = checkpoint.unflatten_like(params, he_flat)
        protons, _ = physics.system_catalogue[1]["He"]
        h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
        _cache["he"] = (params, psi, h_fn)
    return _cache["he"]


def _he_terms(params, psi, h_fn, x):
    from waveflow_amd import vqmc
    model, xd, hpsi, ps, _ = vqmc._energy_terms(params, psi, h_fn, x)
    inv = 1.0 / (ps + 1e-8)
    return model.psi_jacobian(xd, w_psi=inv), hpsi * inv


def test_he_sr_step_with_cg_against_the_dense_step(he_flat):
    """Check 8, first half: vqmc.train_step_sr on 512 He walkers, solver='cg' against 'cholesky': parameters within the propagated bound."""
    import torch
    from waveflow_amd import core, sr, vqmc
    params, psi, h_fn = _he(he_flat)
    x = torch.as_tensor(sorted_walkers(B_HE, 2, 8.0, 5)).cuda()
    lr = 1e-2
    dense, loss_d = vqmc.train_step_sr(1, psi, h_fn, params, x, lr, relative_damping=REL)
    got, loss_c = vqmc.train_step_sr(1, psi, h_fn, params, x, lr, relative_damping=REL, solver="cg", tol=TOL)
    assert loss_d == loss_c
    rows, e32 = _he_terms(params, psi, h_fn, x)
    assert tuple(rows.shape) == (B_HE, psi.model.n_params)
    O = rows.double().cpu().numpy()
    e = e32.double()
    rhs = e - e.mean()
    _, info = sr.solve_cg(rows, rhs, relative_damping=REL, tol=TOL, precondition=False)       # (what natural_gradient runs)
    c = {"O": O}
    lam, c["top"], c["low"], c["kappa"] = _spectrum(O, 0.0)
    rhs = rhs.cpu().numpy()
    y_star = _dense_solution(O, rhs, lam)
    theta = core.flatten_params(params).astype(np.float64)
    t_dense, t_cg = core.flatten_params(dense).astype(np.float64), core.flatten_params(got).astype(np.float64)
    d = (theta - t_dense) / lr
    bound = lr * _direction_bound(c, rhs, y_star, d, info.cpu().numpy()[1]) + 2.0 ** -23 * (np.linalg.norm(theta) + lr * np.linalg.norm(d))
    diff = np.linalg.norm(t_cg - t_dense)
    print(f"[He sr step] B {B_HE}: {int(info.cpu().numpy()[1])} iterations, kappa {c['kappa']:.3e}, |theta_cg - theta_cholesky| {diff:.3e} (bound {bound:.3e}), "
          f"|lr d| {lr * np.linalg.norm(d):.3e}")
    assert np.isfinite(t_cg).all() and not np.array_equal(t_cg, theta)
    assert diff <= bound


def test_he_spring_step_beyond_the_dense_limit(he_flat):
    """Check 8, second half: one train_step_spring on 8192 He walkers with solver='cg' (the dense path refuses the batch): finite parameters, and
    the direction lowers the batch's quadratic model (1 / B) |H O phi - 2 H e~|^2 below its value at mu phi_prev -- d minimises that model plus
    lambda |phi - mu phi_prev|^2, which at phi = mu phi_prev is the model alone."""
    import torch
    from waveflow_amd import core, sr, vqmc
    params, psi, h_fn = _he(he_flat)
    B, mu, clip = 8192, 0.9, 5.0
    x = torch.as_tensor(sorted_walkers(B, 2, 8.0, 11)).cuda()
    prev = torch.as_tensor((1e-3 * np.random.default_rng(2).normal(size=psi.model.n_params)).astype(np.float32)).cuda()
    with pytest.raises(ValueError, match="at most 4096"):
        vqmc.train_step_spring(1, psi, h_fn, params, x, 1e-2, prev, mu, 0.1, clip, relative_damping=REL)
    new, d, loss = vqmc.train_step_spring(1, psi, h_fn, params, x, 1e-2, prev, mu, 0.1, clip, relative_damping=REL, solver="cg", tol=TOL)
    flat = core.flatten_params(new)
    assert np.isfinite(flat).all() and np.isfinite(loss) and not np.array_equal(flat, core.flatten_params(params))
    assert bool(torch.isfinite(d).all()) and d.dtype == torch.float32
    rows, e32 = _he_terms(params, psi, h_fn, x)
    et = sr.clip_local_energies(e32, clip)
    target = 2.0 * (et - et.mean())

    def model_value(phi):
        q = sr.matvec(rows, phi.contiguous())
        return float((((q - q.mean()) - target) ** 2).sum() / B)
    at_d, at_start = model_value(d), model_value((mu * prev.double()).float())
    print(f"[He spring step] B {B}: quadratic model {at_start:.6e} at mu phi_prev -> {at_d:.6e} at d")
    assert at_d < at_start
