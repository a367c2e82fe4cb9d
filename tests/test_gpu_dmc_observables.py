"""Forward walking behind the DMC comb on the device (include/waveflow_dmc_observe.h, waveflow_amd/dmc_observables.py).

Model-free, at B in {1, 63, 64, 65, 1025, 4099}, D in {2, 3, 8} and four (n_slots, stride): after every call the genealogy, the snapshots, the
tags, every integer accumulator and the distinct-ancestor column equal dmc_observables.reference_update exactly, the fp64 sums agree with the
fp64 sum of the fp32 per-configuration values of wf_observe_accumulate to 1e-12, and a second run leaves the same bits.  One case at 2^20
walkers.  The pair histogram against the V_ee it was filled next to.  With a model: the state after dmc_fw_step is the state after dmc_step bit
for bit and the tracker is the one `update` builds by hand from dmc.reconfigure's src; five graph replays against five eager calls; the size
query against the carving, every refusal; dmc.run with a tracker, replayed and eager.  Known answer: <V_en> and <V_ee> of the exact antisymmetric ground state of 1-D He
(scratch/he1d_exact_parts.py) from the walk of tests/test_gpu_dmc.py::test_analytic_guide_reaches_the_exact_energy.
"""
import ctypes

import numpy as np
import pytest

from conftest import sorted_walkers
from test_gpu_dmc import ORDER_BS, SEED, TAU, BOX, _bits, _capture, _dev, _guide, _he, _three, _waveflow, _a256

pytestmark = pytest.mark.gpu

PROTONS = [-0.7, 0.4]
BS, DS = [1, 63, 64, 65, 1025, 4099], [2, 3, 8]
SHAPES = [(1, 1), (3, 2), (16, 1), (4, 5)]                       # (n_slots, stride)
CASES = [(B, D, S, stride) for B in BS for D in DS for S, stride in SHAPES]
IDS = [f"B{B}-D{D}-slots{S}-stride{stride}" for B, D, S, stride in CASES]
# lowest antisymmetric state of 1-D soft-Coulomb He in the box of 10, finite differences at n = 400 (scratch/he1d_exact_parts.py); n = 300
# gives -2.59431 and 0.40466: the two grids differ by 1.6e-4 and 4e-5, below the 1e-3 at which the difference would enter the tolerance
V_EN_EXACT, V_EE_EXACT = -2.59415, 0.40462


def _values(cfg, protons):
    """V_en and V_ee of configurations [n, D] as wf_observe_accumulate forms them (psi = 1, no derivatives: the potentials need none) ->
    two float64 arrays over the finite configurations."""
    import torch
    from waveflow_amd import observables as obs
    x = torch.as_tensor(np.ascontiguousarray(cfg)).cuda()
    zero = torch.zeros_like(x)
    v = obs.accumulate(x, torch.ones(x.shape[0], device="cuda"), zero, zero, protons, return_values=True).cpu().numpy()
    fin = np.isfinite(cfg).all(axis=1)
    return v[fin, 3].astype(np.float64), v[fin, 4].astype(np.float64)


def _compare(fw, ref, tag):
    """Everything that is an integer, exactly; tag as Python integers."""
    have = {"anc": fw.anc, "snap": fw.snap, "counts": fw.counts, "density": fw.density, "pair": fw.pair}
    tags = [int(t) & 0xFFFFFFFFFFFFFFFF for t in fw.tag.cpu().numpy()]
    assert tags == list(ref.tag), (tag, tags, ref.tag)
    live = [s for s, t in enumerate(ref.tag) if t != 0xFFFFFFFFFFFFFFFF]      # an empty slot's anc and snap are not defined
    for name, t in have.items():
        a, b = t.cpu().numpy(), getattr(ref, name)
        if name in ("anc", "snap"):
            a, b = a[live], b[live]
        assert np.array_equal(_bits(a) if name == "snap" else a, _bits(b) if name == "snap" else b), (tag, name)
    assert int(fw.measurements.item()) == ref.measurements, tag
    series = fw.series.cpu().numpy()
    assert np.array_equal(series[:, :, 2:], ref.series[:, :, 2:]), (tag, "counted and distinct columns of the series")
    return series


def _drive(B, D, S, stride, check):
    """3 S stride + 2 calls of update on walkers that are gathered through src and jittered, next to reference_update -> the bits of every
    tensor of the tracker at the end."""
    import torch
    from waveflow_amd import dmc_observables as fwo
    rng = np.random.default_rng(7 * B + 13 * D + S + stride)
    geometry = (B, D, S, stride, 37, 53, -6.0, 6.0, 5)                            # bins that divide nothing; walkers reach beyond the range
    fw = fwo.ForwardWalk(*geometry, device="cuda")
    ref = fwo.Reference(*geometry) if check else None
    sums = np.zeros((S + 1, 2, 2))
    x = sorted_walkers(B, D, 7.0, B + D)
    gen = torch.zeros(1, dtype=torch.int64, device="cuda")
    n_calls = 3 * S * stride + 2
    for g in range(1, n_calls + 1):
        kind = g % 5
        src = None if kind == 0 else rng.integers(0, B, size=B).astype(np.int32)   # with repeats, not monotone; every fifth call the identity
        if g == 3:
            src[rng.integers(0, B, size=min(B, 3))] = [B + 5, -2, 1 << 30][:min(B, 3)]   # out of range: clamped
        x = ((x if src is None else x[np.clip(src, 0, B - 1)]) + np.float32(0.05) * rng.normal(size=(B, D)).astype(np.float32)).astype(np.float32)
        if g == 2 or (B > 1 and g > 2):
            x[B // 2, D - 1] = np.nan                                             # one walker; it is snapshotted, inherited and skipped
        xd = torch.as_tensor(x).cuda()
        sd = None if src is None else torch.as_tensor(src).cuda()
        gen += 1
        fwo.update(xd, sd, PROTONS, fw, gen if g % 2 else g)                      # the generation on the device, or as a number
        if not check:
            continue
        measured = fwo.reference_update(ref, x, src, PROTONS, g)
        series = _compare(fw, ref, (B, D, S, stride, g))
        assert (len(measured) > 0) == (g % stride == 0)
        if measured:
            row = series[(ref.measurements - 1) % 5]
            for lag, cfg in measured:
                v_en, v_ee = _values(cfg, PROTONS)
                add = np.array([[v_en.sum(), (v_en * v_en).sum()], [v_ee.sum(), (v_ee * v_ee).sum()]])
                sums[lag] += add
                assert (np.abs(row[lag, :2] - add[:, 0]) <= 1e-12 * np.abs(add[:, 0])).all(), (g, lag)
                assert row[lag, 2] == v_en.size
            assert not row[[j for j in range(S + 1) if j not in dict(measured)]].any()   # a lag no slot serves: zeros
            have = fw.sums.cpu().numpy()
            assert (np.abs(have - sums) <= 1e-12 * np.abs(sums)).all(), (g, np.abs(have - sums).max())
    if check:
        total = ref.counts[:, 0] + ref.counts[:, 1]
        assert ref.measurements == n_calls // stride and total[0] == B * ref.measurements and total[S] >= 2 * B   # every lag was served
        # the NaN walker was skipped; walkers beyond the range were counted as such (at the lags only where an ancestor out there survived:
        # uniformly random parents coalesce within about B generations)
        assert ref.counts[0, 1] > 0 and (B < 63 or ref.counts[0, 2] > 0)
    torch.cuda.synchronize()
    return [_bits(t) for t in fw.tensors()]


@pytest.mark.parametrize("B,D,S,stride", CASES, ids=IDS)
def test_update_equals_the_integer_reference(B, D, S, stride):
    first = _drive(B, D, S, stride, check=True)
    again = _drive(B, D, S, stride, check=False)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)                                               # bitwise the same a second time, the fp64 sums included


@pytest.mark.parametrize("B", ORDER_BS)
def test_lag_0_sums_are_the_ordered_sum_of_the_potentials(B):
    """After one update at generation 0 the sums of lag 0 equal, bit for bit, the sums of V_en, V_en^2, V_ee and V_ee^2 in the one order of
    the device's fp64 sums (_accum.ordered_sum) over the per-walker potentials of wf_observe_accumulate (psi = 1, no derivatives: the same
    local_values); a walker that is not finite enters as 0."""
    import torch
    from waveflow_amd import dmc_observables as fwo
    from waveflow_amd import observables as obs
    from waveflow_amd._accum import ordered_sum
    D = 2
    x = sorted_walkers(B, D, 7.0, B + 3)
    x[3::7, 1] = np.nan
    x[5::11, 0] = np.inf
    fin = np.isfinite(x).all(axis=1)
    fw = fwo.ForwardWalk(B, D, 1, 1, 37, 53, -6.0, 6.0, 2, device="cuda")
    xd = torch.as_tensor(x).cuda()
    fwo.update(xd, None, PROTONS, fw, 0)
    zero = torch.zeros_like(xd)
    v = obs.accumulate(xd, torch.ones(B, device="cuda"), zero, zero, PROTONS, return_values=True).cpu().numpy().astype(np.float64)
    sums, counts = fw.sums.cpu().numpy()[0].reshape(-1), fw.counts.cpu().numpy()[0]
    assert list(counts[:2]) == [fin.sum(), (~fin).sum()] and (B < 65 or not fin.all())
    with np.errstate(all="ignore"):
        terms = [v[:, 3], v[:, 3] * v[:, 3], v[:, 4], v[:, 4] * v[:, 4]]
    for k in range(4):
        want = ordered_sum(np.where(fin, terms[k], 0.0))
        assert np.isfinite(sums[k]) and sums[k].tobytes() == want.tobytes(), (k, sums[k], want)


def test_update_at_2_pow_20_walkers():
    """2^20 walkers, 16 slots, the largest histograms: three calls, every integer equal to the reference."""
    import torch
    from waveflow_amd import dmc_observables as fwo
    B, D, S = 1 << 20, 2, 16
    geometry = (B, D, S, 1, 512, 1024, -8.0, 8.0, 2)
    fw, ref = fwo.ForwardWalk(*geometry, device="cuda"), fwo.Reference(*geometry)
    rng = np.random.default_rng(20)
    x = sorted_walkers(B, D, 8.5, 20)
    for g in (1, 2, 3):
        src = np.sort(rng.integers(0, B, size=B)).astype(np.int32) if g < 3 else rng.integers(0, B, size=B).astype(np.int32)
        x = x[src] + np.float32(0.01) * rng.normal(size=(B, D)).astype(np.float32)
        fwo.update(torch.as_tensor(x).cuda(), torch.as_tensor(src).cuda(), PROTONS, fw, g)
        fwo.reference_update(ref, x, src, PROTONS, g)
        _compare(fw, ref, g)
    assert list(ref.counts[:4, 0]) == [3 * B, 2 * B, B, 0] and ref.counts[0, 2] > 0 and ref.series[0, 2, 3] < ref.series[0, 1, 3] < B
    have, want = fw.sums.cpu().numpy(), ref.sums
    assert (np.abs(have - want) <= 1e-12 * np.abs(want)).all()                    # (numpy's pairwise sums of the same fp32 values)


def test_pair_histogram_and_v_ee_agree():
    """V_ee recomputed from the pair histogram at bin centres, 1024 bins over [0, 20), is within 0.385 w / 2 (w = 20 / 1024) of sum V_ee / n:
    0.385 = max |d/dr (1 + r^2)^(-1/2)| (at r = 1 / sqrt 2), times half a bin.  Walkers inside the range: no pair is dropped.  Lag 0 and lag 1."""
    import torch
    from waveflow_amd import dmc_observables as fwo
    B, D = 4099, 2
    fw = fwo.ForwardWalk(B, D, 1, 1, 64, 1024, -10.0, 10.0, 4, device="cuda")
    rng = np.random.default_rng(1)
    for g in (1, 2, 3):
        x = torch.as_tensor(sorted_walkers(B, D, 9.9, g)).cuda()
        fwo.update(x, torch.as_tensor(rng.integers(0, B, size=B).astype(np.int32)).cuda(), PROTONS, fw, g)
    r = fwo.result(fw, n_blocks=2)
    w = 20.0 / 1024
    assert list(r["outside_pair"]) == [0, 0] and list(r["n"]) == [3 * B, 2 * B] and list(r["n_skipped"]) == [0, 0]
    pair = fw.pair.cpu().numpy()
    assert (pair.sum(axis=1) == r["n"]).all()
    centres = (np.arange(1024) + 0.5) * w
    from_hist = (pair * (1.0 / np.sqrt(1.0 + centres ** 2))).sum(axis=1) / r["n"]
    print(f"[pair histogram] V_ee from the bins {from_hist}, from the sums {r['v_ee']} (bound {0.385 * w / 2:.2e})")
    assert (np.abs(from_hist - r["v_ee"]) <= 0.385 * w / 2).all()
    assert np.allclose(r["pair"].sum(axis=1) * w, 1.0) and np.allclose(r["density"].sum(axis=1) * (20.0 / 64), 2.0)


# ---- with a model

def _fw_step_against_the_plain_step(model, protons, B, tag):
    """Six generations with n_slots = 2, stride = 2 (measurements at 2, 4, 6; retags; lag 2 from generation 6 on... lag 1 at 4, lag 2 at 6):
    dmc_fw_step next to dmc_step from the same start, and next to the route by hand with `update` fed by dmc.reconfigure's src."""
    import torch
    from waveflow_amd import dmc, dmc_observables as fwo
    box = float(model.desc.box_size)
    plain, walked = model.make_dmc_state(B, ring_len=3), model.make_dmc_state(B, ring_len=3)
    model.dmc_init(plain, SEED, protons, exact_sampler=True)
    model.dmc_init(walked, SEED, protons, exact_sampler=True)
    fw, by_hand = (model.make_forward_walk(B, 2, 2, n_density_bins=50, n_pair_bins=70, series_len=2) for _ in range(2))
    torch.cuda.synchronize()
    x, psi, grad, e_loc = (t.clone() for t in (plain.x, plain.psi, plain.grad, plain.e_loc))
    e_trial = float(plain.e_trial.item())
    for g in range(6):
        tau, e_cut = (TAU, 0.0005)[g % 2], 1.0                                    # (both branches of the acceptance: tests/test_gpu_dmc.py)
        xn, flag = dmc.propose(x, psi, grad, box, tau, SEED, g)
        grn, hdn, psn = model.psi_derivatives(xn, hessian_diag=True, return_psi=True)
        w, record = dmc.accept(x, psi, grad, e_loc, xn, psn, grn, hdn, flag, protons, tau, e_trial, SEED, g, e_cut=e_cut)
        src, _ = dmc.reconfigure(x, psi, grad, e_loc, w, SEED, g)
        fwo.update(x, src, protons, by_hand, g + 1)
        record = record.cpu().numpy()
        e_trial = float(record[1] / record[0])
        model.dmc_step(plain, SEED, protons, tau, e_cut=e_cut)
        model.dmc_fw_step(walked, fw, SEED, protons, tau, e_cut=e_cut)
        torch.cuda.synchronize()
        for a, b in zip(plain.tensors(), walked.tensors()):
            assert np.array_equal(_bits(a), _bits(b)), (tag, g)                   # the DMC state: bit for bit that of dmc_step
        assert np.array_equal(_bits(walked.x), _bits(x)) and int(walked.counter.item()) == g + 1
        for name, a, b in zip(("snap", "anc", "tag", "counts", "density", "pair", "sums", "measurements", "series"), fw.tensors(), by_hand.tensors()):
            assert np.array_equal(_bits(a), _bits(b)), (tag, g, name)             # the tracker: that of update by hand
    assert int(fw.measurements.item()) == 3 and [int(t) for t in fw.tag.cpu().numpy()] == [4, 6]
    counts = fw.counts.cpu().numpy()
    assert list(counts[:, 0] + counts[:, 1]) == [3 * B, 2 * B, B]                 # lag 0 at 2, 4, 6; lag 1 at 4 and 6; lag 2 at 6
    series = fw.series.cpu().numpy()
    assert series[0, 0, 3] == B and 0 < series[0, 2, 3] <= series[0, 1, 3] <= B   # row 0 holds the third measurement (series_len 2)
    print(f"[dmc_fw_step vs dmc_step, {tag}] B {B}: 6 generations equal; distinct ancestors at lag 1, 2: {series[0, 1, 3]:.0f}, {series[0, 2, 3]:.0f}")


def test_fw_step_leaves_the_state_of_the_plain_step_he_128(he_flat):
    _fw_step_against_the_plain_step(*_he(he_flat), 128, "He")


def test_fw_step_leaves_the_state_of_the_plain_step_he_16384_staged_sampler_matrix_cores(he_flat):
    _fw_step_against_the_plain_step(*_he(he_flat), 16384, "He")


def test_fw_step_leaves_the_state_of_the_plain_step_three_particles_67():
    _fw_step_against_the_plain_step(*_three(), 67, "D = 3")


def test_five_replays_equal_five_eager_calls_tracker_included(he_flat):
    import torch
    model, protons = _he(he_flat)
    B = 128
    out = {}
    for mode in ("direct", "graph"):
        state = model.make_dmc_state(B, ring_len=8)
        fw = model.make_forward_walk(B, 2, 2, series_len=4)
        state.st["ws"] = model._workspace(model.dmc_fw_workspace_bytes(B, 2), state.device).fill_(0xFF)
        model.dmc_init(state, SEED, protons)
        held = state.tensors() + fw.tensors()
        kept = [t.clone() for t in held]

        def step():
            model.dmc_fw_step(state, fw, SEED, protons, TAU, limit_drift=True, e_cut=2.0)

        def restore():
            for t, k in zip(held, kept):
                t.copy_(k)
        run = _capture(model, step, restore).replay if mode == "graph" else step
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        out[mode] = [_bits(t) for t in held]
        assert int(state.counter.item()) == 5 and int(fw.measurements.item()) == 2 and [int(t) for t in fw.tag.cpu().numpy()] == [4, 2]
    for a, g in zip(out["direct"], out["graph"]):
        assert np.array_equal(a, g)


def test_size_query_equals_the_carving_and_the_refusals_of_the_plain_step(he_flat):
    import torch
    from waveflow_amd import core, dmc, dmc_observables as fwo
    L = fwo.lib()
    he, protons = _he(he_flat)
    three, _ = _three()

    def update_bytes(B, S):
        blocks = min(-(-B // 256), 1024)
        return _a256(4 * S * B) + _a256(S * B) + _a256((S + 1) * blocks * 64) + _a256(17 * 8)
    for model, D, B, S in ((he, 2, 128, 2), (three, 3, 67, 5), (he, 2, 16384, 16), (he, 2, 1 << 20, 1)):
        assert L.wf_dmc_fw_workspace_bytes(B, D, S) == update_bytes(B, S), (B, D, S)
        assert model.dmc_fw_workspace_bytes(B, S) == model.dmc_workspace_bytes(B) + _a256(4 * B) + update_bytes(B, S), (B, D, S)
    # the refusals of wf_vqmc_dmc_step, from the size query too
    top = dmc.MAX_WALKERS
    q = L.wf_vqmc_dmc_fw_workspace_bytes
    assert q(he._h, top, 16) > 0 and q(he._h, top + 1, 2) == -2 and q(three._h, 131072, 2) > 0 and q(three._h, 131073, 2) == -2
    assert q(he._h, 128, 0) == -1 and q(he._h, 128, 17) == -1 and q(None, 128, 2) == -1 and q(he._h, 0, 2) == -1
    params, psi, _, _ = _waveflow(2, 6, 23, 1, 10.0, kind="first")
    first = psi.model
    first.set_params_device(torch.as_tensor(core.flatten_params(params).astype(np.float32)).cuda())
    assert q(first._h, 128, 2) == -2
    B = 128
    need = he.dmc_fw_workspace_bytes(B, 2)
    state = he.make_dmc_state(B, ring_len=2)
    fw = he.make_forward_walk(B, 2, 1)
    he.dmc_init(state, SEED, protons)
    before = [t.clone() for t in state.tensors() + fw.tensors()]
    pr, n_pr = he._protons(protons)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    one, big = ctypes.c_void_p(256), 1 << 40

    def step(m=he, B=B, tau=TAU, fwc=fw.c, w=ws.data_ptr(), nbytes=need):
        return L.wf_vqmc_dmc_fw_step(m._h, ctypes.byref(state.c), ctypes.byref(fwc), SEED, B, pr, n_pr, tau, 0, 0.0, w, nbytes, None)
    assert step(nbytes=need - 1) == -1                                            # one byte less
    assert step(m=first, w=one, nbytes=big) == -2 and step(m=three, B=131073, w=one, nbytes=big) == -2
    assert step(B=top + 1, w=one, nbytes=big) == -2 and step(tau=-TAU) == -1 and step(w=None, nbytes=big) == -1
    bad = fwo.DmcFw.from_buffer_copy(fw.c)
    bad.n_slots = 17
    assert step(fwc=bad) == -1
    bad.n_slots, bad.n_pair_bins = 2, 1025
    assert step(fwc=bad) == -2
    with pytest.raises(ValueError, match="ForwardWalk"):
        he.dmc_fw_step(state, he.make_forward_walk(64, 2, 1), SEED, protons, TAU)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state.tensors() + fw.tensors()))   # nothing was launched
    assert step() == 0
    torch.cuda.synchronize()
    assert int(state.counter.item()) == 1 and int(fw.measurements.item()) == 1 and int(fw.tag[1].item()) == 1


def test_run_with_a_forward_walk_replayed_equals_eager_and_the_plain_run(he_flat):
    """dmc.run(..., forward_walk=): the captured step and the eager one leave the same ring and the same tracker; the ring is that of a run
    without forward walking; the accumulators hold the measured generations only (zeroed behind the equilibration, tags kept: every lag is
    served from the first measured generation on).  Both warnings are drawn: 1 a.u. of equilibration, a longest lag of 0.5 a.u."""
    from waveflow_amd import dmc
    model, protons = _he(he_flat)
    B, kw = 128, dict(tau=TAU, n_steps=40, n_equil=20, seed=SEED, limit_drift=True, e_cut=1.0, n_blocks=4)
    out = {}
    for mode in ("graph", "eager", "plain"):
        fw = model.make_forward_walk(B, 2, 5, n_density_bins=40, n_pair_bins=40, series_len=16) if mode != "plain" else None
        with pytest.warns(RuntimeWarning) as caught:
            out[mode] = dmc.run(model, protons, B, use_graph=mode == "graph", forward_walk=fw, **kw)
        texts = " | ".join(str(w.message) for w in caught)
        assert "tau * n_equil" in texts and ("n_slots * stride * tau" in texts) == (fw is not None)
        if fw is not None:
            out[mode]["tracker"] = [_bits(t) for t in fw.tensors()]
    for a, b in zip(out["graph"]["tracker"], out["eager"]["tracker"]):
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(out["graph"]["ring"]), _bits(out["eager"]["ring"])) and np.array_equal(_bits(out["graph"]["ring"]), _bits(out["plain"]["ring"]))
    assert "forward_walk" not in out["plain"]
    r = out["graph"]["forward_walk"]
    assert r["measurements"] == 8 and list(r["lag"]) == [0, 5, 10] and list(r["n_measurements"]) == [8, 8, 8]     # generations 25, 30, ..., 60
    assert list(r["n"] + r["n_skipped"]) == [8 * B] * 3 and np.isfinite(r["v_en"]).all() and (r["v_ee_stderr"] > 0).all()
    assert r["distinct_fraction"][0] == 1.0 and 0 < r["distinct_fraction"][2] <= r["distinct_fraction"][1] <= 1.0


# ---- known answer

def test_forward_walking_reaches_the_exact_potential_energies():
    """The walk of test_analytic_guide_reaches_the_exact_energy (alpha = 0.6, 1024 walkers, tau = 0.05, 600 + 2000 generations through
    dmc.propose / accept / reconfigure) with `update` behind every comb: n_slots = 8, stride = 25, the accumulators zeroed behind the
    equilibration -- 80 measurements in 10 blocks.  At lag 8 (200 generations, 10 a.u.) V_en and V_ee must be the exact expectation values of
    the antisymmetric ground state within 5 blocked standard errors of their series; at lag 0 (the mixed estimator) both must be more than 10
    of theirs away; and more than 0.3 of the tagged walkers must still have descendants at lag 8.  (The fp64 CPU prototype of this walk, three
    seeds: mixed V_en -2.512 / -2.518 / -2.508 +- 0.003, V_ee 0.385 / 0.386 / 0.383 +- 0.001; lag 8 V_en -2.593 / -2.596 / -2.586 +- 0.005,
    V_ee 0.405 / 0.405 / 0.402 +- 0.0015; surviving share 0.56 - 0.58.)"""
    import torch
    from waveflow_amd import dmc, dmc_observables as fwo, observables as obs
    from waveflow_amd.utils import physics
    protons = physics.system_catalogue[1]["He"][0]
    B, tau, n_equil, n_steps = 1024, 0.05, 600, 2000
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.sort(torch.randn(B, 2, device="cuda", generator=g) * 1.5, dim=1).values.float().contiguous()
    psi, grad, hdiag = _guide(x)
    e_loc = obs.accumulate(x, psi, grad, hdiag, protons, return_values=True)[:, 0].contiguous()
    et = torch.tensor([-1.8], dtype=torch.float64, device="cuda")
    fw = fwo.ForwardWalk(B, 2, 8, 25, 200, 200, -BOX, BOX, 128, device="cuda")
    ws = torch.empty(fwo.lib().wf_dmc_fw_workspace_bytes(B, 2, 8), dtype=torch.uint8, device="cuda")
    gen = torch.zeros(1, dtype=torch.int64, device="cuda")

    def generation(step, comb):
        xn, flag = dmc.propose(x, psi, grad, BOX, tau, SEED, step)
        psn, grn, hdn = _guide(xn)
        w, record = dmc.accept(x, psi, grad, e_loc, xn, psn, grn, hdn, flag, protons, tau, et, SEED, step)
        if comb:
            src, _ = dmc.reconfigure(x, psi, grad, e_loc, w, SEED, step)
            gen.add_(1)
            fwo.update(x, src, protons, fw, gen, workspace=ws)
        return record
    for s in range(300):                                                         # to |psi_T|^2 first: the 300 steps of the energy test
        generation(1 << 30 | s, comb=False)
    for s in range(n_equil + n_steps):
        if s == n_equil:
            fw.zero_accumulators()
        generation(s, comb=True)
    r = fwo.result(fw, n_blocks=10)
    for j in range(9):
        print(f"[forward walking] lag {r['lag'][j]:3d} generations: V_en {r['v_en'][j]:.4f} +- {r['v_en_stderr'][j]:.4f}, V_ee {r['v_ee'][j]:.4f} +- "
              f"{r['v_ee_stderr'][j]:.4f}, surviving ancestors {r['distinct_fraction'][j]:.3f}, {r['n_measurements'][j]} measurements "
              f"(exact {V_EN_EXACT}, {V_EE_EXACT})")
    assert r["measurements"] == 80 and list(r["n_measurements"]) == [80] * 9 and not r["n_skipped"].any()
    assert abs(r["v_en"][8] - V_EN_EXACT) <= 5 * r["v_en_stderr"][8], (r["v_en"][8], r["v_en_stderr"][8])
    assert abs(r["v_ee"][8] - V_EE_EXACT) <= 5 * r["v_ee_stderr"][8], (r["v_ee"][8], r["v_ee_stderr"][8])
    assert abs(r["v_en"][0] - V_EN_EXACT) > 10 * r["v_en_stderr"][0], (r["v_en"][0], r["v_en_stderr"][0])
    assert abs(r["v_ee"][0] - V_EE_EXACT) > 10 * r["v_ee_stderr"][0], (r["v_ee"][0], r["v_ee_stderr"][0])
    assert r["distinct_fraction"][8] > 0.3
