"""Observables on the device (include/waveflow_observe.h, waveflow_amd/observables.py, DeviceModel.observe_step).

The model-free kernel is held against numpy on the same fp32 inputs: per-walker values against an fp64 recomputation (bound: K 2^-24 M, K the
fp32 operations on the longest path, M the sum of the absolute values of a value's terms), the fp64 sums against numpy's sum of the device's
own per-walker values (bound: B 2^-52 sum |v|), histograms and counters exactly against the fp32 rule of the header.  The step is held
against the eager route (model.psi_derivatives, then observables.accumulate) bit for bit.

Skipped walkers and the fp64 sums.  The sums of a call are formed in an order that depends on B alone (lane = walker index modulo the grid,
shuffle tree, waves, blocks), so a batch from which the skipped walkers have been REMOVED has another B and another order: its sums agree
with the planted batch to the summation bound above, not bit for bit.  What is bitwise is stronger and is what the test asserts: the sums of
the planted batch equal an fp64 emulation on the host of exactly that order over the device's own values in which a skipped walker adds
nothing; histograms, counts[0] and the outside counters are integers and equal those of the batch without the planted walkers exactly.
"""
import ctypes

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
LO, HI = -10.0, 10.0
GRID_BLOCKS, BLOCK = 1024, 256                     # the capped grid of the accumulation kernel
B_TWO_PASSES = GRID_BLOCKS * BLOCK + 77            # the grid-stride loop runs twice
PROTONS = {0: [], 2: [-0.9, 0.9], 8: [-7.5, -3.0, -0.9, 0.0, 0.0, 0.9, 2.5, 6.0]}
# (B, D, protons, density bins, pair bins): every B, D, proton count and bin count of the issue at least once
CASES = [(1, 2, 0, 0, 0), (63, 3, 2, 1, 1), (64, 8, 8, 7, 1024), (65, 2, 2, 512, 0), (255, 3, 8, 7, 1), (256, 8, 0, 512, 1024),
         (257, 2, 8, 1, 1024), (4099, 3, 0, 512, 1024), (4099, 8, 2, 7, 1), (4099, 2, 2, 0, 1), (B_TWO_PASSES, 2, 2, 7, 1024)]
_cache = {}


# ---- inputs and numpy references

def _inputs(B, D, seed):
    """walkers in [-8, 8) sorted per row; psi, grad, hdiag random fp32 of unit scale with |psi| >= 0.05"""
    g = np.random.default_rng(seed + 1000)
    x = sorted_walkers(B, D, 8.0, seed)
    psi = g.normal(size=B).astype(f32)
    psi = np.where(np.abs(psi) < 0.05, np.copysign(f32(0.05), psi), psi).astype(f32)
    return x, psi, g.normal(size=(B, D)).astype(f32), g.normal(size=(B, D)).astype(f32)


def _reference64(x, psi, grad, hdiag, protons):
    """-> (values [B, 5], M [B, 5]) in fp64 from the fp32 inputs; M: the sum of the absolute values of each value's terms"""
    x, psi, grad, hdiag = (a.astype(f64) for a in (x, psi, grad, hdiag))
    D = x.shape[1]
    inv = 1.0 / (psi + f64(f32(1e-8)))
    lap = hdiag.sum(1)
    v_en = np.zeros_like(psi)
    for p in protons:
        v_en -= (1.0 / np.sqrt(1.0 + (f64(f32(p)) - x) ** 2)).sum(1)
    v_ee = np.zeros_like(psi)
    for i in range(D):
        for j in range(i):
            v_ee += 1.0 / np.sqrt(1.0 + (x[:, i] - x[:, j]) ** 2)
    t_lap = -0.5 * lap * inv
    t_grad = 0.5 * ((grad * inv[:, None]) ** 2).sum(1)
    e_loc = (-0.5 * lap + (v_en + v_ee) * psi) * inv
    M = np.stack([np.abs(0.5 * lap * inv) + (np.abs(v_en) + np.abs(v_ee)) * np.abs(psi * inv), (0.5 * np.abs(hdiag) * np.abs(inv)[:, None]).sum(1),
                  t_grad, np.abs(v_en), v_ee], axis=1)
    return np.stack([e_loc, t_lap, t_grad, v_en, v_ee], axis=1), M


def _hist_reference(x, nd, npair, lo=LO, hi=HI):
    """-> (density [D, nd], pair [npair], outside density, outside pair) by the header's fp32 rule (int64)"""
    B, D = x.shape
    width = f32(hi) - f32(lo)
    density, pair, out_d, out_p = np.zeros((D, nd), np.int64), np.zeros(npair, np.int64), 0, 0
    if nd > 0:
        scale = f32(nd) / width
        for d in range(D):
            t = ((x[:, d] - f32(lo)) * scale).astype(f32)
            inside = (t >= 0) & (t < f32(nd))
            density[d] = np.bincount(t[inside].astype(np.int32), minlength=nd)
            out_d += int((~inside).sum())
    if npair > 0:
        scale = f32(npair) / width
        for i in range(D):
            for j in range(i):
                t = (np.abs(x[:, i] - x[:, j]).astype(f32) * scale).astype(f32)
                inside = (t >= 0) & (t < f32(npair))
                pair += np.bincount(t[inside].astype(np.int32), minlength=npair)
                out_p += int((~inside).sum())
    return density, pair, out_d, out_p


def _dev(*arrays):
    import torch
    return [torch.as_tensor(a).cuda() for a in arrays]


def _acc(D, nd, npair, lo=LO, hi=HI):
    from waveflow_amd import observables as obs
    return obs.Accumulator(D, nd, npair, lo=lo, hi=hi, device="cuda")


def _bits(t):
    """The four arrays of a Totals as bytes"""
    return tuple(a.tobytes() for a in (t.sums, t.counts, t.density, t.pair))


def _run(case):
    """One device call per case (values and accumulator), shared by the tests below and left unchanged."""
    from waveflow_amd import observables as obs
    if case not in _cache:
        B, D, n_pr, nd, npair = case
        inputs = _inputs(B, D, 11 + B % 97 + D)
        acc = _acc(D, nd, npair)
        values = obs.accumulate(*_dev(*inputs), PROTONS[n_pr], acc=acc, return_values=True)
        _cache[case] = (inputs, values.cpu().numpy(), acc.totals())
    return _cache[case]


# ---- 1 .. 3: the model-free kernel against numpy

@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-D{}-p{}-bins{}x{}".format(*c))
def test_per_walker_values_against_fp64(case):
    B, D, n_pr, nd, npair = case
    inputs, values, _ = _run(case)
    ref, M = _reference64(*inputs, PROTONS[n_pr])
    K = 8 + 4 * (n_pr * D + D * (D - 1) // 2)
    assert values.shape == (B, 5) and values.dtype == f32 and np.isfinite(values).all()
    err = np.abs(values.astype(f64) - ref)
    bound = K * 2.0 ** -24 * M
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err == 0, 0.0, np.inf))
    print(f"[observables values, B {B} D {D} protons {n_pr}] K {K}: worst |device - fp64| / (K 2^-24 M) per scalar "
          + " ".join(f"{n} {r:.3f}" for n, r in zip(("e_loc", "t_lap", "t_grad", "v_en", "v_ee"), ratio.max(0))))
    assert (err <= bound).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-D{}-p{}-bins{}x{}".format(*c))
def test_sums_against_numpy_of_the_device_values(case):
    from waveflow_amd._accum import ordered_sum   # the device's order of summation, restated in numpy
    B = case[0]
    _, values, tot = _run(case)
    v = values.astype(f64)
    worst = 0.0
    for k in range(5):
        for col, terms in ((0, v[:, k]), (1, v[:, k] * v[:, k])):
            bound = B * 2.0 ** -52 * np.abs(terms).sum()
            diff = abs(tot.sums[k, col] - terms.sum())
            worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
            assert diff <= bound, (k, col, diff, bound)
            assert tot.sums[k, col] == ordered_sum(terms), (k, col)       # and bit for bit the documented order
    print(f"[observables sums, B {B}] worst |device - numpy| / (B 2^-52 sum |v|) {worst:.3e}")
    assert tot.counts[0] == B and tot.counts[1] == 0


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-D{}-p{}-bins{}x{}".format(*c))
def test_histograms_and_counters_equal_the_fp32_rule(case):
    B, D, n_pr, nd, npair = case
    (x, *_), _, tot = _run(case)
    density, pair, out_d, out_p = _hist_reference(x, nd, npair)
    assert x.min() >= -8.0 and x.max() < 8.0 and out_d == 0 and out_p == 0      # nothing is outside [-10, 10), no distance outside [0, 20)
    assert np.array_equal(tot.density, density) and np.array_equal(tot.pair, pair)
    assert tot.counts.tolist() == [B, 0, 0, 0]
    if nd:
        assert tot.density.sum() + tot.counts[2] == D * tot.counts[0]
    if npair:
        assert tot.pair.sum() + tot.counts[3] == D * (D - 1) // 2 * tot.counts[0]


def _plain_call(x, nd, npair, lo, hi, seed=3):
    """accumulate on walkers x with random psi, grad, hdiag and no protons -> Totals"""
    from waveflow_amd import observables as obs
    B, D = x.shape
    _, psi, grad, hdiag = _inputs(B, D, seed)
    acc = _acc(D, nd, npair, lo, hi)
    obs.accumulate(*_dev(np.ascontiguousarray(x, dtype=f32), psi, grad, hdiag), [], acc=acc)
    return acc.totals()


@pytest.mark.parametrize("lo,hi", [(-10.0, 10.0), (-8.0, 8.0), (0.0, 3.0)])
@pytest.mark.parametrize("nb", [1, 7, 64, 512])
def test_lattice_points_land_in_their_bins(lo, hi, nb):
    """x = lo + (k + 0.5) (hi - lo) / n_bins in fp32: point k lands in bin k -- in both columns; every pair distance is 0, the pair bin 0."""
    lattice = (f32(lo) + (np.arange(nb, dtype=f32) + f32(0.5)) * ((f32(hi) - f32(lo)) / f32(nb))).astype(f32)
    x = np.stack([lattice, lattice], axis=1)
    want = _hist_reference(x, nb, 1, lo, hi)
    assert np.array_equal(want[0], np.ones((2, nb), np.int64)) and want[2] == 0          # the rule itself, in numpy
    tot = _plain_call(x, nb, 1, lo, hi)
    assert np.array_equal(tot.density, want[0]) and tot.pair.tolist() == [nb] and tot.counts.tolist() == [nb, 0, 0, 0]


@pytest.mark.parametrize("lo,hi,nb", [(-10.0, 10.0, 200), (-10.0, 10.0, 512), (-8.0, 8.0, 7), (0.0, 3.0, 64)])
def test_edge_walkers_are_counted_outside_and_enter_no_bin(lo, hi, nb):
    """x = hi, x = nextafter(hi, lo) (fp32 rounding puts it at t == n_bins: the rule) and x < lo: counts[2], never a bin.  One walker inside
    shows that the histogram is alive; conservation holds."""
    edge = [f32(hi), np.nextafter(f32(hi), f32(lo)), np.nextafter(f32(lo), f32(lo - 1)), f32(lo - 5)]
    inside = f32(lo) + f32(0.25) * (f32(hi) - f32(lo))
    x = np.array([[e, e] for e in edge] + [[inside, inside]], dtype=f32)
    want = _hist_reference(x, nb, nb, lo, hi)
    tot = _plain_call(x, nb, nb, lo, hi)
    assert np.array_equal(tot.density, want[0]) and np.array_equal(tot.pair, want[1])
    assert tot.counts.tolist() == [5, 0, want[2], want[3]]
    if (lo, hi, nb) == (-10.0, 10.0, 200):
        assert want[2] == 8 and tot.density.sum() == 2       # all four edge walkers, both columns: outside
    assert tot.counts[2] >= 6 and tot.density.sum() + tot.counts[2] == 2 * 5 and tot.pair.sum() + tot.counts[3] == 5
    assert tot.density.sum(1).max() <= 2


# ---- 4: skipped walkers

def test_skipped_walkers_are_counted_and_add_nothing():
    from waveflow_amd import observables as obs
    from waveflow_amd._accum import ordered_sum
    B, D, nd, npair = 600, 3, 64, 128
    x, psi, grad, hdiag = _inputs(B, D, 21)
    plant = {63: "x", 64: "psi", 255: "grad", 256: "hdiag", 300: "inv"}     # both sides of a wave edge and of a block edge, and one more
    x[63, 1] = np.nan
    psi[64] = np.inf
    grad[255, 2] = np.nan
    hdiag[256, 0] = -np.inf
    psi[300] = -f32(1e-8)                                                    # psi + 1e-8f == 0: inv is infinite
    keep = np.ones(B, bool)
    keep[list(plant)] = False
    acc = _acc(D, nd, npair)
    values = obs.accumulate(*_dev(x, psi, grad, hdiag), PROTONS[2], acc=acc, return_values=True).cpu().numpy()
    tot = acc.totals()
    acc2 = _acc(D, nd, npair)
    obs.accumulate(*_dev(x[keep], psi[keep], grad[keep], hdiag[keep]), PROTONS[2], acc=acc2)
    clean = acc2.totals()
    assert tot.counts[1] == len(plant) and tot.counts[0] == B - len(plant) == clean.counts[0] and clean.counts[1] == 0
    assert np.array_equal(tot.density, clean.density) and np.array_equal(tot.pair, clean.pair) and np.array_equal(tot.counts[2:], clean.counts[2:])
    assert tot.density.sum() + tot.counts[2] == D * tot.counts[0] and tot.pair.sum() + tot.counts[3] == 3 * tot.counts[0]
    # values of the skipped walkers, as computed
    col = {n: i for i, n in enumerate(obs.SCALARS)}
    assert np.isfinite(values[keep]).all()
    for b in plant:
        assert not np.isfinite(values[b]).all(), (b, values[b])
    assert np.isnan(values[63, col["v_ee"]]) and np.isnan(values[63, col["v_en"]]) and np.isnan(values[63, col["e_loc"]]) and np.isfinite(values[63, col["t_lap"]])
    assert np.isnan(values[64, col["e_loc"]]) and values[64, col["t_lap"]] == 0 and values[64, col["t_grad"]] == 0
    assert np.isnan(values[255, col["t_grad"]]) and np.isfinite(values[255, [col["e_loc"], col["t_lap"]]]).all()
    assert np.isinf(values[256, col["t_lap"]]) and np.isinf(values[256, col["e_loc"]]) and np.isfinite(values[256, col["t_grad"]])
    assert np.isinf(values[300, col["t_lap"]]) and np.isinf(values[300, col["t_grad"]]) and not np.isfinite(values[300, col["e_loc"]])
    # the sums: bit for bit the device's order with the skipped walkers adding nothing; against the batch without them, the summation bound
    v = np.where(keep[:, None], values.astype(f64), 0.0)
    for k in range(5):
        for c, terms in ((0, v[:, k]), (1, v[:, k] * v[:, k])):
            assert tot.sums[k, c] == ordered_sum(terms), (k, c)
            assert abs(tot.sums[k, c] - clean.sums[k, c]) <= B * 2.0 ** -52 * np.abs(terms).sum(), (k, c)


# ---- 5: reproducibility and additivity

def test_same_call_twice_halves_values_only_and_workspaces_give_the_same_bits():
    import torch
    from waveflow_amd import observables as obs
    B, D, nd, npair = 4099, 3, 64, 128
    dev = _dev(*_inputs(B, D, 31))
    pr = PROTONS[2]

    def call(ws=None):
        acc = _acc(D, nd, npair)
        vals = obs.accumulate(*dev, pr, acc=acc, return_values=True, workspace=ws)
        return acc.totals(), vals
    a, va = call()
    b, vb = call()
    assert _bits(a) == _bits(b) and torch.equal(va.view(torch.int32), vb.view(torch.int32)) and a.counts[0] == B
    # two halves into one accumulator == two halves into two accumulators, merged
    h = 2049
    first, second = [t[:h].contiguous() for t in dev], [t[h:].contiguous() for t in dev]
    one = _acc(D, nd, npair)
    obs.accumulate(*first, pr, acc=one)
    obs.accumulate(*second, pr, acc=one)
    p, q = _acc(D, nd, npair), _acc(D, nd, npair)
    obs.accumulate(*first, pr, acc=p)
    obs.accumulate(*second, pr, acc=q)
    assert _bits(one.totals()) == _bits(p.totals().merge(q.totals()))
    assert np.array_equal(one.totals().density, a.density) and np.array_equal(one.totals().pair, a.pair) and one.totals().counts[0] == B
    # values only
    only = obs.accumulate(*dev, pr, return_values=True)
    assert torch.equal(only.view(torch.int32), va.view(torch.int32))
    # a poisoned workspace, and one 256 bytes into a larger allocation
    n = obs.lib().wf_observe_workspace_bytes(B)
    assert n == 256 * -(-(-(-B // 256) * 14 * 8) // 256)
    buf = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for ws in (buf[:n], buf[256:]):
        c, vc = call(ws)
        assert _bits(c) == _bits(a) and torch.equal(vc.view(torch.int32), va.view(torch.int32))


# ---- 6 .. 9: the step

SEED, FIRST = 20240611, 5


def _waveflow(D, k, knots, layers, box, kind="mean", seed=7):
    from waveflow_amd import model_factory
    init = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                            i_spline_reg=0.05, n_flow_layers=layers, box_size=box, xu_coord_type=kind)
    return init(seed, D)


def _he(he_flat):
    """(model, protons, x [67, 2] on the device, flat parameters on the device): the He model and walkers of tests/test_gpu_sr_step.py"""
    import torch
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        _, psi, _, _ = _waveflow(2, 6, 23, 3, 10.0)
        flat = torch.as_tensor(np.asarray(he_flat, dtype=np.float32)).cuda()
        psi.model.set_params_device(flat)
        protons, _ = physics.system_catalogue[1]["He"]
        _cache["he"] = (psi.model, protons, torch.as_tensor(sorted_walkers(67, 2, 8.0, 5)).cuda(), flat)
    return _cache["he"]


def _three():
    """D = 3 (degree 6, 23 knots, 2 layers, box 10) at its initial parameters, 16 sorted walkers, two protons"""
    import torch
    from waveflow_amd import core
    from waveflow_amd.utils import physics
    if "three" not in _cache:
        params, psi, _, _ = _waveflow(3, 6, 23, 2, 10.0)
        flat = torch.as_tensor(core.flatten_params(params).astype(np.float32)).cuda()
        psi.model.set_params_device(flat)
        protons, _ = physics.system_catalogue[1]["H2"]
        _cache["three"] = (psi.model, protons, torch.as_tensor(sorted_walkers(16, 3, 8.0, 5)).cuda(), flat)
    return _cache["three"]


def _counter(first=FIRST):
    import torch
    return torch.tensor([first], dtype=torch.int64, device="cuda")


def _eager(model, protons, x, acc=None):
    """The eager route: model.psi_derivatives, then observables.accumulate -> values [B, 5]"""
    from waveflow_amd import observables as obs
    grad, hdiag, psi = model.psi_derivatives(x, hessian_diag=True, return_psi=True)
    return obs.accumulate(x, psi, grad, hdiag, protons, acc=acc, return_values=True)


def _step_against_the_eager_route(case, tag):
    import torch
    model, protons, x, flat = case
    B, D = int(x.shape[0]), model.D
    probe = torch.as_tensor(sorted_walkers(64, D, 8.0, 9)).cuda()
    flat_before, logp_before = flat.clone(), model.log_pdf(probe).clone()
    # draw = 0: values and accumulators are those of the eager route, the counter advanced by one
    acc, counter = _acc(D, 200, 200), _counter()
    values = torch.full((B, 5), float("nan"), device="cuda")
    model.observe_step(acc, counter, SEED, B, protons, walkers=x, values=values)
    ref_acc = _acc(D, 200, 200)
    ref = _eager(model, protons, x, ref_acc)
    assert torch.equal(values.view(torch.int32), ref.view(torch.int32)) and bool(torch.isfinite(values).all())
    assert _bits(acc.totals()) == _bits(ref_acc.totals()) and acc.totals().counts[0] == B
    assert int(counter.item()) == FIRST + 1
    # draw = 1: the walkers it returns reproduce its accumulators through the eager route
    acc1, w5 = _acc(D, 200, 200), torch.full((B, D), float("nan"), device="cuda")
    model.observe_step(acc1, counter.fill_(FIRST), SEED, B, protons, exact_sampler=True, out_walkers=w5)
    ref1 = _acc(D, 200, 200)
    _eager(model, protons, w5, ref1)
    t1 = acc1.totals()
    assert _bits(t1) == _bits(ref1.totals()) and t1.counts[0] + t1.counts[1] == B and t1.counts[0] > 0
    assert int(counter.item()) == FIRST + 1
    w5b, w6 = torch.full_like(w5, float("nan")), torch.full_like(w5, float("nan"))
    model.observe_step(_acc(D, 0, 0), counter.fill_(FIRST), SEED, B, protons, exact_sampler=True, out_walkers=w5b)     # the same counter
    model.observe_step(_acc(D, 0, 0), counter, SEED, B, protons, exact_sampler=True, out_walkers=w6)                   # the next one
    assert torch.equal(w5.view(torch.int32), w5b.view(torch.int32)) and not torch.equal(w5, w6) and int(counter.item()) == FIRST + 2
    ok = torch.isfinite(w5).all(1)
    assert bool((w5[ok][:, 1:] >= w5[ok][:, :-1]).all()) and float(w5[ok].abs().max()) <= 10.0
    # nothing of the model moved
    assert torch.equal(flat.view(torch.int32), flat_before.view(torch.int32))
    assert torch.equal(model.log_pdf(probe).view(torch.int32), logp_before.view(torch.int32))
    print(f"[observe step vs eager, {tag}] B {B}: values, accumulators and counter equal; drawn walkers: {int(t1.counts[1])} skipped")


def test_step_is_the_eager_route_he(he_flat):
    _step_against_the_eager_route(_he(he_flat), "He")


def test_step_is_the_eager_route_three_particles():
    _step_against_the_eager_route(_three(), "D = 3")


def test_step_at_16384_walkers_staged_sampler_and_matrix_core_derivatives(he_flat):
    import torch
    model, protons, _, _ = _he(he_flat)
    B = 16384
    acc, counter = _acc(2, 200, 200), _counter()
    values, w = torch.full((B, 5), float("nan"), device="cuda"), torch.full((B, 2), float("nan"), device="cuda")
    model.observe_step(acc, counter, SEED, B, protons, exact_sampler=True, out_walkers=w, values=values)
    ref_acc = _acc(2, 200, 200)
    ref = _eager(model, protons, w, ref_acc)
    assert torch.equal(values.view(torch.int32), ref.view(torch.int32))
    t = acc.totals()
    assert _bits(t) == _bits(ref_acc.totals()) and int(counter.item()) == FIRST + 1
    assert t.counts[0] + t.counts[1] == B and t.counts[0] > 0
    r = t.result()
    print(f"[observe step, He, B {B}] e_loc {r['e_loc']:.4f} +- {r['e_loc_stderr']:.4f}, t_lap {r['t_lap']:.4f}, t_grad {r['t_grad']:.4f}, "
          f"v_en {r['v_en']:.4f}, v_ee {r['v_ee']:.4f}; skipped {r['n_skipped']}, outside {r['outside_density']} / {r['outside_pair']}")
    # E_L = T_lap + V_en + V_ee per walker up to fp32 rounding (~1e-7 of the terms) and the 1e-8 in the denominator (V 1e-8 / psi, psi ~ 0.1 where
    # |psi|^2 puts walkers): three orders of magnitude below this bound, which a wrong sign or a missing term exceeds by four
    assert abs(r["e_loc"] - (r["t_lap"] + r["v_en"] + r["v_ee"])) <= 1e-4 * (abs(r["t_lap"]) + abs(r["v_en"]) + abs(r["v_ee"]))


def _capture(model, step, restore):
    """`step` captured once, the recipe of tests/test_gpu_sr_step.py: a side stream, one call outside the capture, `restore()`, then the capture."""
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


def test_five_replays_equal_five_eager_calls(he_flat):
    import torch
    model, protons, _, _ = _he(he_flat)
    B = 67
    out = {}
    for mode in ("direct", "graph"):
        acc, counter = _acc(2, 200, 200), _counter()
        acc.st["ws"] = model._workspace(model.observe_step_workspace_bytes(B), acc.device).fill_(0xFF)

        def step():
            model.observe_step(acc, counter, SEED, B, protons, exact_sampler=True)

        def restore():
            acc.reset()
            counter.fill_(FIRST)
        run = _capture(model, step, restore).replay if mode == "graph" else step
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        out[mode] = (acc.totals(), int(counter.item()))
    (a, ca), (g, cg) = out["direct"], out["graph"]
    assert ca == cg == FIRST + 5 and a.counts[0] + a.counts[1] == 5 * B
    assert _bits(a) == _bits(g)


def test_measure_equals_its_steps_by_hand(he_flat):
    import torch
    from waveflow_amd import distributed, observables as obs
    model, protons, _, _ = _he(he_flat)
    n_walkers, batch = 1000, 256
    by_graph = obs.measure(model, protons, n_walkers, batch, SEED, use_graph=True)
    by_calls = obs.measure(model, protons, n_walkers, batch, SEED, use_graph=False)
    acc, counter = _acc(2, 200, 200), _counter(0)
    values = torch.empty(4, batch, 5, device="cuda")
    for s in range(4):
        model.observe_step(acc, counter, SEED, batch, protons, exact_sampler=True, values=values[s])
    hand = acc.totals()
    assert hand.geometry() == by_graph.geometry() == (2, 200, 200, -10.0, 10.0)
    assert _bits(by_graph) == _bits(hand) == _bits(by_calls) and int(counter.item()) == 4
    r = by_graph.result()
    assert r["n"] + r["n_skipped"] == 1024
    e = values[:, :, 0].reshape(-1)
    e = e[torch.isfinite(values.reshape(-1, 5)).all(1)].contiguous()
    assert e.numel() == r["n"]
    mean, var, stderr = distributed.ShardedDensity(model).expectation(e)
    print(f"[measure, He] n {r['n']} skipped {r['n_skipped']}: e_loc {r['e_loc']:.12f} vs block sums {mean:.12f}; stderr {r['e_loc_stderr']:.3e} vs {stderr:.3e}")
    assert abs(r["e_loc"] - mean) <= 1e-12 * abs(mean)       # fp64 summation order only


def test_error_paths_with_a_model(he_flat):
    import torch
    from waveflow_amd import observables as obs
    L = obs.lib()
    model, protons, x, _ = _he(he_flat)
    B = int(x.shape[0])
    pr, n_pr = model._protons(protons)
    grad, hdiag, psi = model.psi_derivatives(x, hessian_diag=True, return_psi=True)
    acc = _acc(2, 200, 200)
    n = L.wf_observe_workspace_bytes(B)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")

    def accumulate(c, ws_bytes=n):
        return L.wf_observe_accumulate(x.data_ptr(), psi.data_ptr(), grad.data_ptr(), hdiag.data_ptr(), B, 2, pr, n_pr, ctypes.byref(c), None,
                                       ws.data_ptr(), ws_bytes, None)

    def variant(**kw):
        fields = {name: getattr(acc.c, name) for name, _ in obs.ObserveAcc._fields_}
        fields.update(kw)
        return obs.ObserveAcc(**fields)
    assert accumulate(variant(n_density_bins=513)) == -2 and accumulate(variant(n_pair_bins=1025)) == -2
    assert accumulate(acc.c, n - 1) == -1
    assert accumulate(variant(lo=3.0, hi=3.0)) == -1
    # the step: a workspace one byte short, and batches without a sampler
    counter = _counter()
    need = L.wf_vqmc_observe_step_workspace_bytes(model._h, B)
    assert need == model.observe_step_workspace_bytes(B) and need > 3 * B * 2 * 4
    sws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def step(m, c, batch, nbytes):
        return L.wf_vqmc_observe_step(m, ctypes.byref(c), counter.data_ptr(), SEED, batch, pr, n_pr, 1, None, 1, None, sws.data_ptr(), nbytes, None)
    assert step(model._h, acc.c, B, need - 1) == -1
    assert step(model._h, variant(n_density_bins=513), B, need) == -2
    assert L.wf_vqmc_observe_step_workspace_bytes(model._h, 131072) > 0 and L.wf_vqmc_observe_step_workspace_bytes(model._h, 131073) > 0   # staged sampler
    three, protons3, _, _ = _three()
    assert L.wf_vqmc_observe_step_workspace_bytes(three._h, 131072) > 0
    assert L.wf_vqmc_observe_step_workspace_bytes(three._h, 131073) == -2        # D = 3: the wave sampler only, up to its limit
    acc3 = _acc(3, 8, 8)
    assert step(three._h, acc3.c, 131073, 1 << 40) == -2
    with pytest.raises(Exception, match="status -2"):
        three.observe_step_workspace_bytes(131073)
    torch.cuda.synchronize()
    t = acc.totals()                                                             # nothing was launched
    assert not t.sums.any() and not t.counts.any() and not t.density.any() and int(counter.item()) == FIRST and not acc3.totals().counts.any()


def test_all_reduce_under_rccl():
    """Totals.all_reduce with the backend the example script initialises ("nccl": RCCL reduces device tensors only), in a process of its own
    with the one rank a single GPU gives: the reduced totals equal the rank's own, dtype for dtype.  (World 2 on the host: the gloo test of
    tests/test_observables_host.py.)"""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_observables_nccl_rank.py"), str(port)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "__ALL_REDUCE_OK__ rank 0 of 1, backend nccl" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
