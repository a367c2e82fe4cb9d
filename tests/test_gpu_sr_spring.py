"""The SPRING optimiser on the GPU (include/waveflow_sr_spring.h; sr.matvec / apply_add / spring_rhs / spring_direction, DeviceModel.spring_step,
ModelTrainer.optimizer = 'spring').  Inputs are synthetic fp32 normal rows unless the test names He.

Bounds.  matvec: products of fp32 operands are exact in fp64, the sum of P terms in any order errs by at most (P - 1) 2^-53 sum |terms|; the
test allows 8 P 2^-53.  apply_add: the bound of wf_sr_apply's test plus the same factor on mu |prev|, and one fp32 rounding.  The right-hand side:
median, w and the clamp bounds exact (numpy sums in the kernel's order: walkers t, t + 256, ... per thread, then the tree over 256 threads),
rhs to 4 B 2^-53 max |r|.  The step against the eager step:
the bound of tests/test_gpu_sr_step.py with the applied step size in the place of the learning rate.
"""
import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BS = [1, 15, 67]
PS = [3, 64, 1001, 2500]        # 2500: two full passes of 1024 columns and a third, partial one
CASES = [(B, P, pad) for B in BS for P in PS for pad in (0, 5)]   # pad 5: the row stride is no multiple of 4, the unaligned path
B_HE = 67
LR = 1e-2
SEED = 20240607
FIRST = 5
_cache = {}


def _rows(B, P, pad):
    """fp32 normal rows [B, P] as a column slice of a contiguous [B, P + pad] matrix (NaN in the padding: reading it would show)."""
    import torch
    g = np.random.default_rng(1000 * B + P + pad)
    host = np.full((B, P + pad), np.nan, np.float32)
    host[:, :P] = g.normal(size=(B, P)).astype(np.float32)
    return host[:, :P].copy(), torch.as_tensor(host).cuda()[:, :P]


def _case(B, P, pad):
    """Device results and fp64 operands of one synthetic case, computed once and shared by the tests below."""
    import torch
    from waveflow_amd import sr
    key = (B, P, pad)
    if key in _cache:
        return _cache[key]
    host, dev = _rows(B, P, pad)
    g = np.random.default_rng(7 * B + P)
    c = {"dev": dev, "O": host.astype(np.float64)}
    v = g.normal(size=P).astype(np.float32)
    c["v"], c["v_dev"] = v.astype(np.float64), torch.as_tensor(v).cuda()
    c["q"] = sr.matvec(dev, c["v_dev"])
    yv = g.normal(size=B) + 0.5
    c["yv"], c["yv_dev"], c["scale"] = yv, torch.as_tensor(yv).cuda(), 2.0 / B
    prev = g.normal(size=P).astype(np.float32)
    c["prev"], c["prev_dev"] = prev.astype(np.float64), torch.as_tensor(prev).cuda()
    c["out"] = sr.apply_add(dev, c["yv_dev"], c["scale"], prev=c["prev_dev"], mu=0.9)
    torch.cuda.synchronize()
    _cache[key] = c
    return c


@pytest.mark.parametrize("B,P,pad", CASES)
def test_matvec_vs_fp64_numpy(B, P, pad):
    import torch
    from waveflow_amd import sr
    c = _case(B, P, pad)
    q = c["q"].cpu().numpy()
    ref = c["O"] @ c["v"]
    bound = 8 * P * EPS * (np.abs(c["O"]) @ np.abs(c["v"]))
    worst = float((np.abs(q - ref) / np.maximum(bound, 1e-300)).max())
    print(f"[matvec] B {B} P {P} ld {P + pad}: worst |err| / bound {worst:.3f}")
    assert q.shape == (B,) and np.isfinite(q).all()
    assert (np.abs(q - ref) <= bound).all()
    assert torch.equal(sr.matvec(c["dev"], c["v_dev"]), c["q"])                     # bitwise repeatable
    if P > 1:   # v at an address that is no multiple of 16: the same sums
        wide = torch.zeros(P + 1, device="cuda")
        wide[1:] = c["v_dev"]
        assert torch.equal(sr.matvec(c["dev"], wide[1:]), c["q"])


@pytest.mark.parametrize("B,P,pad", CASES)
def test_apply_add_vs_fp64_numpy(B, P, pad):
    import torch
    from waveflow_amd import sr
    c = _case(B, P, pad)
    mu = 0.9
    out = c["out"].cpu().numpy().astype(np.float64)
    yc = c["yv"] - c["yv"].mean()
    ref = mu * c["prev"] + c["scale"] * (yc @ c["O"])
    bound = 2.0 ** -23 * np.abs(ref) + 8 * B * EPS * (abs(c["scale"]) * (np.abs(yc) @ np.abs(c["O"])) + mu * np.abs(c["prev"]))
    worst = float((np.abs(out - ref) / np.maximum(bound, 1e-300)).max())
    print(f"[apply_add] B {B} P {P} ld {P + pad}: worst |err| / bound {worst:.3f}")
    assert out.shape == (P,) and np.isfinite(out).all()
    assert (np.abs(out - ref) <= bound).all()
    plain = sr.apply(c["dev"], c["yv_dev"], c["scale"])
    assert torch.equal(sr.apply_add(c["dev"], c["yv_dev"], c["scale"], prev=c["prev_dev"], mu=0.0).view(torch.int32), plain.view(torch.int32))
    assert torch.equal(sr.apply_add(c["dev"], c["yv_dev"], c["scale"], prev=None, mu=0.9).view(torch.int32), plain.view(torch.int32))
    alias = c["prev_dev"].clone()
    got = sr.apply_add(c["dev"], c["yv_dev"], c["scale"], prev=alias, mu=mu, out=alias)
    assert got is alias and torch.equal(alias.view(torch.int32), c["out"].view(torch.int32))


def _kernel_sum(v):
    """The fp64 sum of v in the order of the one-workgroup kernels: thread t adds entries t, t + 256, ... in that order, then the tree over 256."""
    part = np.zeros(256)
    for i in range(v.size):
        part[i % 256] += v[i]
    s = 128
    while s:
        part[:s] += part[s:2 * s]
        s //= 2
    return float(part[0])


def _rhs_reference(e32, q, mu, k):
    """-> ((c, w, c - k w, c + k w), r, r - mean(r)) in fp64, every sum in the kernel's order: the statistics are the kernel's bit for bit."""
    e = e32.astype(np.float64)
    B = e.size
    c = w = lo = hi = 0.0
    r = e.copy()
    if k > 0:
        key = np.sort(np.where(np.isfinite(e32), e32, np.float32(np.inf)))
        c = float(key[B // 2]) if B % 2 else 0.5 * (float(key[B // 2 - 1]) + float(key[B // 2]))
        w = _kernel_sum(np.abs(e - c)) / B
        lo, hi = c - k * w, c + k * w
        r = np.where(e < lo, lo, np.where(e > hi, hi, e))
    if mu:
        r = r - (0.5 * mu) * q
    return (c, w, lo, hi), r, r - _kernel_sum(r) / B


RHS_BS = [1, 2, 15, 16, 67, 193]
RHS_KS = [0.0, 1.0, 5.0]


@pytest.mark.parametrize("B", RHS_BS)
@pytest.mark.parametrize("k", RHS_KS)
def test_right_hand_side_median_clamp_and_centring(B, k):
    """wf_spring_rhs on synthetic H psi and psi; at B >= 15 two walkers carry e = +1e5 and -1e5 (psi = 1, H psi = +-1e5), which a clamp must cut."""
    import torch
    from waveflow_amd import sr
    g = np.random.default_rng(31 * B + int(k))
    psi = g.uniform(0.5, 2.0, size=B).astype(np.float32)
    hpsi = (g.normal(size=B) - 1.8).astype(np.float32) * psi
    if B >= 15:
        psi[[3, 11]] = 1.0
        hpsi[[3, 11]] = [1e5, -1e5]
    q = g.normal(size=B)
    mu = 0.9
    e_loc, inv, rhs, stats = sr.spring_rhs(torch.as_tensor(hpsi).cuda(), torch.as_tensor(psi).cuda(), torch.as_tensor(q).cuda(), mu, k)
    e32, inv32 = e_loc.cpu().numpy(), inv.cpu().numpy()
    want_inv = (np.float32(1.0) / (psi + np.float32(1e-8))).astype(np.float32)
    assert np.array_equal(inv32, want_inv) and np.array_equal(e32, (hpsi * want_inv).astype(np.float32))
    if B >= 15:
        assert e32[3] == 1e5 and e32[11] == -1e5
    (c, w, lo, hi), r, ref = _rhs_reference(e32, q, mu, k)
    got_c, got_w, got_lo, got_hi = stats.cpu().tolist()
    got = rhs.cpu().numpy()
    bound = 4 * B * EPS * np.abs(r).max()
    print(f"[rhs] B {B} k {k}: median {got_c!r} vs {c!r}; w {got_w!r} vs {w!r}; bounds [{got_lo!r}, {got_hi!r}] vs [{lo!r}, {hi!r}]; "
          f"max |rhs err| {np.abs(got - ref).max():.3e} (bound {bound:.3e})")
    assert got_c == c and got_w == w and got_lo == lo and got_hi == hi      # exact
    assert np.abs(got - ref).max() <= bound
    if k > 0 and B >= 15:   # the two outliers sit on the clamp bounds
        assert r[3] == hi - 0.5 * mu * q[3] and r[11] == lo - 0.5 * mu * q[11] and hi < 1e5 and lo > -1e5
    # momentum and clip off: e_loc - mean(e_loc), the bits of the fp64 expression the sr step writes
    _, _, plain, stats0 = sr.spring_rhs(torch.as_tensor(hpsi).cuda(), torch.as_tensor(psi).cuda())
    e = e32.astype(np.float64)
    assert np.array_equal(plain.cpu().numpy(), e - _kernel_sum(e) / B) and not stats0.any()


def test_values_that_are_not_finite_sort_last_in_the_median():
    """A NaN and a -inf among the energies (psi = 1: e_loc is H psi) count as +inf in the sort: the median is that of the finite values and
    two +inf, on the device as in sr.clip_local_energies."""
    import torch
    from waveflow_amd import sr
    nan, inf = float("nan"), float("inf")
    for values, want in (([5.0, nan, 1.0, 2.0, -inf], 5.0), ([5.0, nan, 1.0, 2.0, -inf, 0.0], 3.5), ([nan, -1.5, inf], inf)):
        e = torch.tensor(values, dtype=torch.float32).cuda()
        e_loc, _, _, stats = sr.spring_rhs(e, torch.ones_like(e), None, 0.0, 1.0)
        eager_c, _ = sr._median_and_deviation(e)
        print(f"[rhs, not finite] {values}: median {float(stats[0])!r}, eager {float(eager_c)!r}")
        assert torch.equal(torch.isnan(e_loc), torch.isnan(e)) and torch.equal(torch.nan_to_num(e_loc), torch.nan_to_num(e))
        assert float(stats[0]) == want == float(eager_c)


@pytest.mark.parametrize("mu", [0.0, 0.9])
def test_spring_direction_matches_the_p_space_solution(mu):
    """B = 67, P = 1001 against (S + lambda I) d = g + lambda mu phi solved in fp64 numpy; the bound of
    test_natural_gradient_is_the_three_calls_and_matches_the_p_space_solution (one fp32 rounding of d, and the solve's bound)."""
    import torch
    from waveflow_amd import sr
    c = _case(67, 1001, 0)
    B, P, O = 67, 1001, c["O"]
    H = np.eye(B) - np.ones((B, B)) / B
    e = np.random.default_rng(3).normal(size=B).astype(np.float32) - 2.5
    d = sr.spring_direction(c["dev"], torch.as_tensor(e).cuda(), c["prev_dev"], mu).cpu().numpy().astype(np.float64)
    lam = 1e-3 * np.trace(H @ O @ O.T @ H / B) / B
    ref = np.linalg.solve(O.T @ H @ O / B + lam * np.eye(P), 2.0 / B * O.T @ H @ e.astype(np.float64) + lam * mu * c["prev"])
    rel = np.linalg.norm(d - ref) / np.linalg.norm(ref)
    bound = 2.0 ** -23 + 1e-12 * B * (B / 1e-3 + 1)
    print(f"[spring direction, synthetic] mu {mu}: rel. error vs the P-space solve {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound
    if mu == 0.0:
        assert torch.equal(sr.spring_direction(c["dev"], torch.as_tensor(e).cuda(), c["prev_dev"], 0.0),
                           sr.natural_gradient(c["dev"], torch.as_tensor(e).cuda()))


# ---- the whole step

def _waveflow(D, k, knots, layers, box, kind="mean", seed=7):
    from waveflow_amd import model_factory
    init = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                            i_spline_reg=0.05, n_flow_layers=layers, box_size=box, xu_coord_type=kind)
    return init(seed, D)


def _he(he_flat):
    """(params, psi, h_fn, x [67, 2] on the device, flat parameters on the device): the model and walkers of tests/test_gpu_sr_step.py."""
    import torch
    from waveflow_amd import checkpoint
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        params, psi, _, _ = _waveflow(2, 6, 23, 3, 10.0)
        params = checkpoint.unflatten_like(params, he_flat)
        protons, _ = physics.system_catalogue[1]["He"]
        h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
        x = torch.as_tensor(sorted_walkers(B_HE, 2, 8.0, 5)).cuda()
        _cache["he"] = (params, psi, h_fn, x, torch.as_tensor(np.asarray(he_flat, dtype=np.float32)).cuda())
    return _cache["he"]


def _three():
    """D = 3 (degree 6, 23 knots, 2 layers, box 10) at its initial parameters, 16 sorted walkers, two protons."""
    import torch
    from waveflow_amd import core
    from waveflow_amd.utils import physics
    if "three" not in _cache:
        params, psi, _, _ = _waveflow(3, 6, 23, 2, 10.0)
        protons, _ = physics.system_catalogue[1]["H2"]
        h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
        x = torch.as_tensor(sorted_walkers(16, 3, 8.0, 5)).cuda()
        _cache["three"] = (params, psi, h_fn, x, torch.as_tensor(core.flatten_params(params).astype(np.float32)).cuda())
    return _cache["three"]


def _poisoned(n, shifted=False):
    import torch
    buf = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf[256:] if shifted else buf[:n]


def _fresh_state(model, flat0, lr=LR, first=FIRST, shifted=False, batch=B_HE, phi=None, old=False):
    """Parameters back at flat0 (a copy of their own), the model's images with them, a train state (`old`: that of wf_vqmc_sr_step) and its
    poisoned workspace; `shifted`: 256 bytes into a larger allocation."""
    xs = flat0.clone()
    model.set_params_device(xs)
    if old:
        st = model.make_sr_train_state(xs, first, lr)
        st["ws"] = _poisoned(model.sr_step_workspace_bytes(batch), shifted)
    else:
        st = model.make_spring_train_state(xs, first, lr, phi=None if phi is None else phi.clone())
        st["ws"] = _poisoned(model.spring_step_workspace_bytes(batch), shifted)
    return xs, st


NAMES = ("ring", "norm_ring", "status", "counter")


def _views(model, st, batch):
    """What the last spring_step of `batch` walkers left at the head of its workspace, as views: e_loc, inv float32 [batch]; rhs, y, q float64
    [batch]; d float32 [n_params]; stats float64 [4] = median, deviation, clamp bounds.  No part of the interface: the order is that of
    sr_step_layout (wf_train_sr.cpp), each part at the next multiple of 256 bytes, read here to check what the step computes on the way."""
    import torch
    ws, B, at, out = st["ws"], int(batch), 0, {}
    for name, count, dtype in (("x", B * model.D, torch.float32), ("hpsi", B, torch.float32), ("psi", B, torch.float32), ("e_loc", B, torch.float32),
                               ("inv", B, torch.float32), ("rhs", B, torch.float64), ("y", B, torch.float64), ("q", B, torch.float64),
                               ("d", model.n_params, torch.float32), ("stats", 4, torch.float64)):
        nbytes = count * (4 if dtype == torch.float32 else 8)
        out[name] = ws[at:at + nbytes].view(dtype)
        at += (nbytes + 255) // 256 * 256
    return out


def _snapshot(xs, st, names=NAMES + ("phi", "eff_ring")):
    import torch
    torch.cuda.synchronize()
    out = {k: st[k].clone() for k in names}
    out["x"] = xs.clone()
    return out


def _same(a, b, names=None):
    import torch
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in (names or a))


def _capture(model, step, restore):
    """`step` captured once, the way ModelTrainer does it: a side stream, one call outside the capture, `restore()` to undo it, then the capture."""
    import torch
    side = torch.cuda.Stream(device=model.device)
    side.wait_stream(torch.cuda.current_stream(model.device))
    with torch.cuda.stream(side):
        step()
        restore()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream(model.device).wait_stream(side)
    return graph


def _off_is_the_old_step(case, tag):
    import torch
    params, psi, h_fn, x, flat0 = case
    model, B = psi.model, int(x.shape[0])
    xo, so = _fresh_state(model, flat0, batch=B, old=True)
    model.sr_step(so, SEED, B, h_fn.protons, walkers=x)
    old = _snapshot(xo, so, NAMES)
    xs, st = _fresh_state(model, flat0, batch=B)
    model.spring_step(st, SEED, B, h_fn.protons, walkers=x, momentum=0.0, norm_constraint=0.0, clip=0.0)
    new = _snapshot(xs, st)
    d = _views(model, st, B)["d"]
    print(f"[spring off vs sr step, {tag}] B {B}: |d|^2 {float(new['norm_ring'][FIRST]):.9e}, status {new['status'].tolist()}, eff {float(new['eff_ring'][FIRST])!r}")
    assert not torch.equal(new["x"], flat0) and new["status"].tolist() == [0, 0]
    assert _same(old, new, NAMES + ("x",))
    assert torch.equal(new["phi"].view(torch.int32), d.view(torch.int32)) and bool(new["phi"].any())
    assert float(new["eff_ring"][FIRST]) == float(np.float32(LR))


def test_step_with_everything_off_is_the_sr_step_he(he_flat):
    _off_is_the_old_step(_he(he_flat), "He")


def test_step_with_everything_off_is_the_sr_step_three_particles():
    _off_is_the_old_step(_three(), "D = 3")


def _against_the_eager_step(case, tag, mu=0.9):
    """mu = 0.9, clip 5, a previous direction that is not zero and a cap that binds (a tenth of lr^2 |d|^2 of the uncapped step).
    -> a function that runs the device step again from the same start and returns its snapshot."""
    import torch
    from waveflow_amd import core, vqmc
    params, psi, h_fn, x, flat0 = case
    model, B, P = psi.model, int(x.shape[0]), psi.model.n_params
    clip = 5.0
    phi0 = torch.as_tensor((np.random.default_rng(17).normal(size=P) * 1e-2).astype(np.float32)).cuda()
    dp = core.DeviceParams(params, flat0.clone(), 0)
    d_eager, _ = vqmc.spring_direction(dp, psi, h_fn, x, phi0, mu, clip=clip)
    norm2 = float((d_eager.double() ** 2).sum())
    cap = 0.1 * LR * LR * norm2
    new_dp, d2, loss_eager = vqmc.train_step_spring(1, psi, h_fn, dp, x, LR, phi0, mu, cap, clip)
    eff = vqmc.spring_step_size(LR, d_eager, cap)
    assert torch.equal(d2, d_eager) and torch.equal(dp.flat, flat0) and eff < float(np.float32(LR))
    xs, st = _fresh_state(model, flat0, batch=B, phi=phi0)
    model.spring_step(st, SEED, B, h_fn.protons, walkers=x, momentum=mu, norm_constraint=cap, clip=clip)
    torch.cuda.synchronize()
    th_s, th_e, d = xs.double().cpu().numpy(), new_dp.flat.double().cpu().numpy(), d_eager.double().cpu().numpy()
    bound = 2.0 ** -23 * np.abs(th_e) + 2.0 ** -22 * eff * np.abs(d)
    diff = np.abs(th_s - th_e)
    n_diff = int((diff != 0).sum())
    worst = float((diff / np.maximum(bound, 1e-300)).max())
    ring, norm, status = st["ring"].cpu().numpy(), st["norm_ring"].cpu().numpy(), st["status"].cpu().tolist()
    eff_dev = float(st["eff_ring"][FIRST])
    phi_diff = int((st["phi"] != d_eager).sum())
    print(f"[spring step vs eager, {tag}] B {B} P {P}: {n_diff} entries differ (cap {P // 100}), worst |diff| / bound {worst:.3f}; loss {ring[FIRST, 0] / B:.12f} vs "
          f"{loss_eager:.12f}; |d|^2 {norm[FIRST]:.9e} vs {norm2:.9e}; eff {eff_dev!r} vs {eff!r} (lr {LR}); phi differs in {phi_diff}; status {status}")
    assert np.isfinite(th_s).all() and not np.array_equal(th_s, flat0.double().cpu().numpy())
    assert (diff <= bound).all()
    assert n_diff <= P // 100
    assert abs(ring[FIRST, 0] / B - loss_eager) <= 1e-12 * max(1.0, abs(loss_eager)) and ring[FIRST, 2] == B     # the unclipped energies
    assert status == [0, 0]
    assert abs(norm[FIRST] - norm2) <= 2.0 ** -20 * norm2
    assert abs(eff_dev - eff) <= 2.0 ** -22 * eff
    assert phi_diff <= P // 100 and bool(torch.isfinite(st["phi"]).all())
    first = _snapshot(xs, st)

    def again(shifted=False):
        xs2, st2 = _fresh_state(model, flat0, batch=B, phi=phi0, shifted=shifted)
        model.spring_step(st2, SEED, B, h_fn.protons, walkers=x, momentum=mu, norm_constraint=cap, clip=clip)
        return first, _snapshot(xs2, st2)
    return again


def test_step_is_the_eager_step_he(he_flat):
    _against_the_eager_step(_he(he_flat), "He")


def test_step_is_the_eager_step_three_particles():
    _against_the_eager_step(_three(), "D = 3")


def test_step_without_momentum_with_clip_and_cap_is_the_eager_step_and_repeatable_he(he_flat):
    """Momentum 0 with clip 5 and a binding cap: the right-hand side is computed ahead of the rows, with the clamp on (no q to wait for).  Against
    the eager step under the same bound, and bitwise the same when the step runs again, the workspace at another address."""
    first, second = _against_the_eager_step(_he(he_flat), "He, momentum 0", mu=0.0)(shifted=True)
    assert _same(first, second)
    assert 0.0 < float(first["eff_ring"][FIRST]) < float(np.float32(LR))      # the cap bound


@pytest.mark.parametrize("B", RHS_BS)
@pytest.mark.parametrize("k", RHS_KS)
def test_right_hand_side_inside_the_step_he(he_flat, B, k):
    """One step on He with momentum 0.9 and clip k: numpy on the device's own e_loc and q (read from the head of the workspace) gives the median,
    the deviation, the clamp bounds (exact) and rhs.  (B = 1 with a relative shift only is a refused solve; its right-hand side is there.)"""
    import torch
    from waveflow_amd import sr
    params, psi, h_fn, _, flat0 = _he(he_flat)
    model, P = psi.model, psi.model.n_params
    x = torch.as_tensor(sorted_walkers(B, 2, 8.0, 5)).cuda()
    phi0 = torch.as_tensor((np.random.default_rng(17).normal(size=P) * 1e-2).astype(np.float32)).cuda()
    xs, st = _fresh_state(model, flat0, lr=0.0, phi=phi0, batch=B)      # (rate 0: the parameters, and with them the rows, stay as they are)
    model.spring_step(st, SEED, B, h_fn.protons, walkers=x, momentum=0.9, clip=k)
    torch.cuda.synchronize()
    v = _views(model, st, B)
    e32, q = v["e_loc"].cpu().numpy(), v["q"].cpu().numpy()
    rows = model.psi_jacobian(x, w_psi=v["inv"].clone())
    assert torch.equal(sr.matvec(rows, phi0), v["q"])
    (c, w, lo, hi), r, ref = _rhs_reference(e32, q, 0.9, k)
    got_c, got_w, got_lo, got_hi = v["stats"].cpu().tolist()
    n_cut = int(((e32 < lo) | (e32 > hi)).sum()) if k > 0 else 0
    got = v["rhs"].cpu().numpy()
    bound = 4 * B * EPS * np.abs(r).max()
    print(f"[rhs in the step, He] B {B} k {k}: median {got_c!r}, w {got_w!r} vs {w!r}, bounds [{got_lo!r}, {got_hi!r}], {n_cut} walkers clamped; "
          f"max |rhs err| {np.abs(got - ref).max():.3e} (bound {bound:.3e})")
    assert got_c == c and got_w == w and got_lo == lo and got_hi == hi      # exact
    assert np.abs(got - ref).max() <= bound
    if k == 1.0 and B >= 15:   # some |e_b - c| exceeds their mean unless all are equal
        assert n_cut > 0


def test_three_steps_are_bitwise_repeatable_direct_shifted_and_replayed(he_flat):
    import torch
    params, psi, h_fn, x, flat0 = _he(he_flat)
    model = psi.model
    out = {}
    for mode in ("direct", "shifted", "graph"):
        xs, st = _fresh_state(model, flat0, shifted=mode == "shifted")

        def step():
            model.spring_step(st, SEED, B_HE, h_fn.protons, momentum=0.9, norm_constraint=1e-3, clip=5.0)

        def restore():
            xs.copy_(flat0)
            model.set_params_device(xs)
            st["counter"].fill_(FIRST)
            for name in ("ring", "norm_ring", "eff_ring", "status", "phi"):
                st[name].zero_()
        run = _capture(model, step, restore).replay if mode == "graph" else step
        for _ in range(3):
            run()
        out[mode] = _snapshot(xs, st)
    a = out["direct"]
    assert int(a["counter"].item()) == FIRST + 3 and a["status"].tolist() == [0, 0]
    assert bool((a["ring"][FIRST:FIRST + 3, 2] == B_HE).all()) and bool((a["norm_ring"][FIRST:FIRST + 3] > 0).all())
    assert bool((a["eff_ring"][FIRST:FIRST + 3] > 0).all()) and bool(a["phi"].any())
    assert not torch.equal(a["x"], flat0)
    assert _same(a, out["shifted"])
    assert _same(a, out["graph"])


def test_a_refused_solve_leaves_theta_and_phi_and_is_counted(he_flat):
    """batch = 1, relative damping only: the centred 1 x 1 matrix and its shift are exactly 0 -- info = 1, a status, no fault."""
    import torch
    params, psi, h_fn, x, flat0 = _he(he_flat)
    model = psi.model
    phi0 = torch.as_tensor((np.random.default_rng(17).normal(size=model.n_params) * 1e-2).astype(np.float32)).cuda()
    xs, st = _fresh_state(model, flat0, phi=phi0)
    st["eff_ring"].fill_(7.0)
    model.spring_step(st, SEED, 1, h_fn.protons, damping=0.0, relative_damping=1e-3, momentum=0.9, norm_constraint=1e-3, clip=5.0)
    s = _snapshot(xs, st)
    assert torch.equal(s["x"].view(torch.int32), flat0.view(torch.int32)) and torch.equal(s["phi"].view(torch.int32), phi0.view(torch.int32))
    assert s["status"].tolist() == [1, 1] and float(s["eff_ring"][FIRST]) == 0.0
    assert int(s["counter"].item()) == FIRST + 1 and float(s["ring"][FIRST, 2]) == 1.0 and bool(torch.isfinite(s["ring"][FIRST]).all())
    model.spring_step(st, SEED, B_HE, h_fn.protons, momentum=0.9, norm_constraint=1e-3, clip=5.0)
    s2 = _snapshot(xs, st)
    assert s2["status"].tolist() == [0, 1] and not torch.equal(s2["x"], flat0) and not torch.equal(s2["phi"], phi0)
    assert bool(torch.isfinite(s2["x"]).all()) and float(s2["eff_ring"][FIRST + 1]) > 0.0


def test_applied_step_size_follows_the_rate_and_the_cap_at_every_replay(he_flat):
    """One capture, the learning rate rewritten between two replays; the cap lies between the two rates times |d|: it binds on the second."""
    import torch
    params, psi, h_fn, x, flat0 = _he(he_flat)
    model = psi.model
    xs, st = _fresh_state(model, flat0, lr=0.0)
    model.spring_step(st, SEED, B_HE, h_fn.protons, walkers=x, momentum=0.0, clip=5.0)      # lr 0: only |d|^2 is of interest
    torch.cuda.synchronize()
    norm2 = float(st["norm_ring"][FIRST])
    small, large = 1e-3, 1e-1
    cap = (1e-2 ** 2) * norm2                       # sqrt(cap / |d|^2) = 1e-2 on these walkers
    xs, st = _fresh_state(model, flat0, lr=0.0)

    def restore():
        st["counter"].fill_(FIRST)
        for name in ("ring", "norm_ring", "eff_ring", "status", "phi"):
            st[name].zero_()
    graph = _capture(model, lambda: model.spring_step(st, SEED, B_HE, h_fn.protons, walkers=x, momentum=0.0, norm_constraint=cap, clip=5.0), restore)
    st["step_size"].fill_(small)
    graph.replay()
    st["step_size"].fill_(large)
    graph.replay()
    torch.cuda.synchronize()
    eff, norms = st["eff_ring"].cpu().numpy(), st["norm_ring"].cpu().numpy()
    want = np.sqrt(cap / norms[FIRST + 1])
    print(f"[eff] {eff[FIRST]!r} (lr {small}), {eff[FIRST + 1]!r} (lr {large}, cap gives {want!r})")
    assert eff[FIRST] == float(np.float32(small))
    assert abs(eff[FIRST + 1] - want) <= 2.0 ** -23 * want and want < large
    assert st["status"].cpu().tolist() == [0, 0]


def test_refusals_of_the_c_entry_with_a_model(he_flat):
    import ctypes
    import torch
    from waveflow_amd import sr
    params, psi, h_fn, x, flat0 = _he(he_flat)
    model = psi.model
    xs, st = _fresh_state(model, flat0)
    L = sr.lib()
    pr, n_pr = model._protons(h_fn.protons)
    ws, n = st["ws"].data_ptr(), st["ws"].numel()
    assert n == L.wf_vqmc_spring_step_workspace_bytes(model._h, B_HE) > L.wf_vqmc_sr_step_workspace_bytes(model._h, B_HE)
    assert L.wf_vqmc_spring_step_workspace_bytes(model._h, 4097) == -2
    c = ctypes.byref(st["c"])
    assert L.wf_vqmc_spring_step(model._h, c, SEED, 4097, pr, n_pr, 0.0, 1e-3, 0.9, 1e-3, 5.0, 0, None, 1, ws, 1 << 40, None) == -2
    assert L.wf_vqmc_spring_step(model._h, c, SEED, B_HE, pr, n_pr, 0.0, 1e-3, 0.9, 1e-3, 5.0, 0, None, 1, ws, n - 1, None) == -1
    assert L.wf_vqmc_spring_step(model._h, c, SEED, B_HE, pr, n_pr, 0.0, 1e-3, 1.0, 1e-3, 5.0, 0, None, 1, ws, n, None) == -1
    s = _snapshot(xs, st)   # nothing was launched
    assert torch.equal(s["x"], flat0) and int(s["counter"].item()) == FIRST and not bool(s["ring"].any()) and s["status"].tolist() == [0, 0]


def test_model_trainer_with_spring_eager_device_and_restart(tmp_path, monkeypatch):
    import os
    import torch
    from waveflow_amd import vqmc

    def trainer(name, on_device, epochs=3):
        t = vqmc.ModelTrainer(system_name="He", learning_rate=1e-2, box_length=10, num_epochs=epochs, batch_size=64, log_every=2)
        t.save_dir = str(tmp_path / name)
        t.optimizer = 'spring'
        t.sr_on_device = on_device
        return t

    for on_device in (False, True):
        t = trainer(f"a{int(on_device)}", on_device)
        _, loss = t.start_training(verbose=False)
        assert len(loss[1:]) == 3 and np.isfinite(np.asarray(loss[1:], dtype=np.float64)).all()
        assert os.path.exists(os.path.join(t.save_dir, "spring_state.npz")) and not os.path.exists(os.path.join(t.save_dir, "optimizer_state.npz"))
        assert t.spring_skipped_steps == 0 and 0 <= t.spring_capped_steps <= 3
        with np.load(os.path.join(t.save_dir, "spring_state.npz")) as z:
            assert int(z["epoch"]) == 2 and z["phi"].shape == (t.psi.model.n_params,) and z["phi"].any()     # the direction of epoch 1
        assert bool(torch.isfinite(t.params.flat).all())
    # a restart hands the saved direction to the step: bitwise what the checkpoint saved, and the step uses it
    import warnings
    from waveflow_amd import core
    with np.load(os.path.join(str(tmp_path / "a1"), "spring_state.npz")) as z:
        saved = z["phi"].copy()
    states = []
    make = core.DeviceModel.make_spring_train_state

    def spy(self, *a, **k):
        st = make(self, *a, **k)
        states.append((st, st["phi"].clone()))
        return st
    monkeypatch.setattr(core.DeviceModel, "make_spring_train_state", spy)
    t2 = trainer("a1", True, epochs=1)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*spring_state.*")      # "momentum restarts from zero": the saved direction was not found
        _, loss2 = t2.start_training(restart=True, verbose=False)
    assert np.isfinite(np.asarray(loss2[1:], dtype=np.float64)).all()
    os.remove(os.path.join(str(tmp_path / "a1"), "spring_state.npz"))
    t3 = trainer("a1", True, epochs=1)
    with pytest.warns(UserWarning, match="momentum restarts from zero"):
        t3.start_training(restart=True, verbose=False)
    (st2, phi2), (st3, phi3) = states
    assert np.array_equal(phi2.cpu().numpy().view(np.int32), saved.view(np.int32)) and saved.any() and not bool(phi3.any())
    slot = int(st2["counter"].item() - 1) % st2["ring_len"]
    n2, n3 = float(st2["norm_ring"][slot]), float(st3["norm_ring"][slot])
    print(f"[spring restart] |d|^2 of the first step with the saved direction {n2:.9e}, from zero {n3:.9e}")
    assert int(st2["counter"].item()) == int(st3["counter"].item()) and n2 > 0 and n3 > 0 and n2 != n3   # the same step, but for the direction it starts from
    assert not torch.equal(st2["phi"], st3["phi"])


def test_spring_trains_he_from_a_fresh_initialisation(tmp_path):
    """He, box 10, exact sampler, batch 512, N steps on the device path from a fresh initialisation; the energy on 4 x 2^15 independent |psi|^2
    walkers as test_trained_energy_respects_the_variational_bound evaluates it; Adam (the unchanged trainer, lr 5e-4) with the same batch, N and
    seed as the yardstick."""
    from waveflow_amd import vqmc
    N = SPRING_TRAIN_STEPS

    def run(name, optimizer):
        t = vqmc.ModelTrainer(system_name="He", learning_rate=SPRING_TRAIN_LR if optimizer == 'spring' else 5e-4, box_length=10, num_epochs=N, batch_size=512,
                              log_every=10 ** 9)
        t.save_dir = str(tmp_path / name)
        t.exact_sampler = True
        t.optimizer = optimizer
        t.sr_on_device = True
        params, _ = t.start_training(verbose=False)
        m = t.psi.model
        m.ensure_params(params)
        es = []
        for seed in range(4):
            x = m.sample(500 + seed, 1 << 15, exact=True)
            h, ps = m.hamiltonian(x, t.h_fn.protons, return_psi=True)
            es.append((h / (ps + 1e-8)).double().cpu().numpy())
        return t, params, np.concatenate(es)

    t, params, e = run("spring", 'spring')
    _, _, e_adam = run("adam", 'adam')
    mean, sem = e.mean(), e.std() / np.sqrt(e.size)
    print(f"[spring trains He] N {N}: mean {mean:.5f} +- {sem:.5f}, median {np.median(e):.5f}; Adam median {np.median(e_adam):.5f}, mean {e_adam.mean():.5f}; "
          f"skipped {t.spring_skipped_steps}, capped {t.spring_capped_steps}")
    assert t.spring_skipped_steps == 0
    assert bool(np.isfinite(params.flat.cpu().numpy()).all())
    assert mean > -1.8161 - 5 * sem, (mean, sem)
    assert np.median(e) < np.median(e_adam), (np.median(e), np.median(e_adam))
    assert SPRING_MEDIAN_WINDOW[0] < np.median(e) < SPRING_MEDIAN_WINDOW[1], np.median(e)


# N sized so that the test (two trainings, two evaluations) stays well under 10 s: 300 SPRING steps at 512 walkers are 0.55 s on the MI355X.
# The trainer's shipped settings (vqmc.SPRING_DEFAULTS: momentum 0.9, norm constraint 0.1, clip 5, relative damping 1e-2) at learning rate 0.1.
# Measured over the trainer seeds 2, 3, 4, 5: SPRING medians -1.8061, -1.7927, -1.8101, -1.8083 (Adam: 0.504, -0.589, -0.042, -0.575);
# the window is that spread, [-1.8101, -1.7927], widened by 3 x its width (0.0174) on either side.
SPRING_TRAIN_STEPS = 300
SPRING_TRAIN_LR = 0.1
SPRING_MEDIAN_WINDOW = (-1.8101 - 3 * 0.0174, -1.7927 + 3 * 0.0174)
