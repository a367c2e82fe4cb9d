"""Fixed-node diffusion Monte Carlo on the device (include/waveflow_dmc.h, waveflow_amd/dmc.py).

Model-free, at B in {1, 63, 64, 65, 257, 4099} and D in {2, 3, 8}: the proposal bit for bit against numpy fp64 of the header's formula (from the
device's own chi), the statistics and the stream layout of chi; the acceptance (E_L' bit for bit against wf_observe_accumulate, logA and w to
1e-12, the decisions, the record); the comb bit for bit against dmc.comb_reference (numpy uint64 prefix sums, searchsorted, Python integers).
With a model: the step against the by-hand route bit for bit, five graph replays against five eager calls, the size query against the
carving, every refusal.  Known answers: the fixed-node energy of 1-D He is the exact eigenvalue -1.8161 (scratch/he1d_exact.py) -- with an
analytic guide through the three model-free entries, and with the trained model through dmc.run.
"""
import ctypes
import warnings

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

SEED = 20250117
BOX, TAU = 10.0, 0.05
BS, DS = [1, 63, 64, 65, 257, 4099], [2, 3, 8]
CASES = [(B, D) for B in BS for D in DS]
IDS = [f"B{B}-D{D}" for B, D in CASES]
PROTONS = [-0.7, 0.4]
E_EXACT = -1.8161           # lowest antisymmetric eigenvalue of 1-D soft-Coulomb He in the box of 10 (scratch/he1d_exact.py: -1.81613 at n = 400)
_cache = {}


def _dev(*arrays):
    import torch
    return tuple(torch.as_tensor(a).cuda().contiguous() for a in arrays)


def _bits(t):
    """float32 / float64 tensor or array -> its bit patterns as a numpy integer array (NaN compares equal to itself)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _inputs(B, D, seed, special=True):
    """Old walkers: x sorted in (-8, 8), psi of either sign away from zero, a drift of order 1, e_loc around -1.8.  With `special`, every eighth
    walker each: pushed through the wall by its drift, with two coordinates 1e-6 apart (the noise makes them cross), or not finite (x, psi or
    grad in turn)."""
    g = np.random.default_rng(seed)
    x = sorted_walkers(B, D, 8.0, seed)
    psi = (g.uniform(0.05, 1.0, size=B) * np.where(g.uniform(size=B) < 0.3, -1.0, 1.0)).astype(np.float32)
    grad = (g.normal(size=(B, D)) * np.abs(psi)[:, None]).astype(np.float32)
    e_loc = (-1.8 + 0.3 * g.normal(size=B)).astype(np.float32)
    if special:
        for b in range(B):
            kind = b % 8
            if kind == 1:
                x[b, -1] = 9.99
                grad[b, -1] = 50.0 * psi[b]
            elif kind == 2:
                x[b, 1] = x[b, 0] + np.float32(1e-6)                  # (still ascending: above one ulp of |x| < 8)
                grad[b, 0], grad[b, 1] = 3.0 * psi[b], -3.0 * psi[b]  # the drift pushes the pair through each other as well
            elif kind == 3:
                which = (b // 8) % 3
                if which == 0:
                    x[b, D - 1] = np.nan
                elif which == 1:
                    psi[b] = np.nan
                else:
                    grad[b, 0] = np.inf
    return x, psi, grad, e_loc


def _seq_sum(a):
    """sum over the last axis, d ascending, one fp64 rounding per addition"""
    acc = np.zeros(a.shape[0], dtype=np.float64)
    for d in range(a.shape[1]):
        acc = acc + a[:, d]
    return acc


def _vbar(psi, grad, tau, limit):
    """The drift of the header: fp32 inv and v (numpy float32 arithmetic rounds every operation), then fp64.  -> (v fp32, vbar fp64)"""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / (psi + np.float32(1e-8))
        v = grad * inv[:, None]
        v64 = v.astype(np.float64)
        if not limit:
            return v, v64
        a = _seq_sum(v64 * v64) * tau
        f = np.where(a == 0.0, 1.0, (-1.0 + np.sqrt(1.0 + 2.0 * a)) / np.where(a == 0.0, 1.0, a))
        return v, v64 * f[:, None]


def _propose_reference(x, psi, grad, chi, tau, limit, box=BOX):
    with np.errstate(all="ignore"):
        v, vb = _vbar(psi, grad, tau, limit)
        xp = ((x.astype(np.float64) + tau * vb) + np.sqrt(tau) * chi.astype(np.float64)).astype(np.float32)
        fin = np.isfinite(x).all(1) & np.isfinite(psi) & np.isfinite(grad).all(1) & np.isfinite(v).all(1)
        ok = fin & np.isfinite(xp).all(1) & (np.abs(xp) < np.float32(box)).all(1) & (xp[:, 1:] > xp[:, :-1]).all(1)
    return np.where(ok[:, None], xp, x), (~ok).astype(np.int32)


# ---- propose

@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limited"])
@pytest.mark.parametrize("B,D", CASES, ids=IDS)
def test_proposal_is_the_fp64_formula_bit_for_bit(B, D, limit):
    from waveflow_amd import dmc
    x, psi, grad, _ = _inputs(B, D, 11 * B + D)
    if B >= 64:
        grad[40] = 0.0          # |v|^2 tau == 0: the limiter's factor is 1
    xd, pd, gd = _dev(x, psi, grad)
    xn, flag, chi = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 7, limit_drift=limit, return_chi=True)
    want_x, want_flag = _propose_reference(x, psi, grad, chi.cpu().numpy(), TAU, limit)
    flag = flag.cpu().numpy()
    assert np.array_equal(flag, want_flag)
    assert np.array_equal(_bits(xn), _bits(want_x))
    assert np.array_equal(_bits(xn)[flag == 1], _bits(x)[flag == 1])            # a flagged walker keeps its x, bit for bit (NaN included)
    moved = xn.cpu().numpy()[flag == 0]
    assert (np.abs(moved) < BOX).all() and (moved[:, 1:] > moved[:, :-1]).all()
    assert np.array_equal(_bits(xd), _bits(x))                                  # inputs untouched
    if B >= 64:
        kinds = np.arange(B) % 8
        # not finite: always; the wall: always with the plain drift (2.5 beyond it against a noise of 0.22), the limiter caps the step at
        # sqrt(2 tau) = 0.32; crossings: most of eight or more walkers
        assert flag[kinds == 3].all() and flag[kinds == 2].any() and (flag[kinds == 1].any() if limit else flag[kinds == 1].all())
        assert not flag[kinds == 0].all()


@pytest.mark.parametrize("D", DS)
def test_chi_is_standard_normal(D):
    """2^16 x D numbers: |mean| <= 5 / sqrt(n), the variance within 5 sqrt(2 / n) of 1 (five standard errors of either estimator), and
    Kolmogorov-Smirnov against the normal at p > 1e-4."""
    import torch
    from scipy import stats
    from waveflow_amd import dmc
    B = 1 << 16
    x = torch.zeros(B, D, device="cuda") + torch.arange(D, device="cuda", dtype=torch.float32)
    _, _, chi = dmc.propose(x, torch.ones(B, device="cuda"), torch.zeros(B, D, device="cuda"), BOX, TAU, SEED, 3, return_chi=True)
    c = chi.double().cpu().numpy()
    n = c.size
    p = stats.kstest(c.reshape(-1), "norm").pvalue
    print(f"[chi, D {D}] n {n}: mean {c.mean():+.2e} (bound {5 / np.sqrt(n):.2e}), var - 1 {c.var() - 1:+.2e} (bound {5 * np.sqrt(2 / n):.2e}), KS p {p:.3f}")
    assert abs(c.mean()) <= 5 / np.sqrt(n)
    assert abs(c.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert p > 1e-4
    for d in range(D):                                                           # every column on its own: cosine and sine branches alike
        assert abs(c[:, d].mean()) <= 5 / np.sqrt(B) and abs(c[:, d].var() - 1.0) <= 5 * np.sqrt(2.0 / B), d
    assert abs(np.corrcoef(c[:, 0], c[:, 1])[0, 1]) <= 5 / np.sqrt(B)


@pytest.mark.parametrize("D", DS)
def test_chi_depends_on_seed_step_and_slot_alone(D):
    from waveflow_amd import dmc
    x, psi, grad, _ = _inputs(4099, D, 5, special=False)
    xd, pd, gd = _dev(x, psi, grad)
    big = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 4, return_chi=True)
    small = dmc.propose(xd[:64].contiguous(), pd[:64].contiguous(), gd[:64].contiguous(), BOX, TAU, SEED, 4, return_chi=True)
    assert np.array_equal(_bits(big[2])[:64], _bits(small[2])) and np.array_equal(_bits(big[0])[:64], _bits(small[0]))
    again = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 4, return_chi=True)
    assert np.array_equal(_bits(big[2]), _bits(again[2])) and np.array_equal(_bits(big[0]), _bits(again[0]))
    other_step = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 5, return_chi=True)[2]
    other_seed = dmc.propose(xd, pd, gd, BOX, TAU, SEED + 1, 4, return_chi=True)[2]
    wrapped = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 4 + (1 << 40), return_chi=True)[2]
    assert (_bits(big[2]) != _bits(other_step)).mean() > 0.99 and (_bits(big[2]) != _bits(other_seed)).mean() > 0.99
    assert np.array_equal(_bits(big[2]), _bits(wrapped))                         # the step enters modulo 2^40, as the header says


# ---- accept

def _accept_case(B, D, limit, e_cut=0.0, seed=0):
    """Old walkers, proposals from the device's own propose, and invented values at the proposals: psi' near psi (every eleventh of the other
    sign), a drift, a Hessian diagonal (every thirteenth NaN); every seventeenth old e_loc NaN."""
    from waveflow_amd import dmc
    g = np.random.default_rng(1000 + 17 * B + D + seed)
    x, psi, grad, e_loc = _inputs(B, D, 3 * B + D + seed)
    e_loc[np.arange(B) % 17 == 16] = np.nan
    xd, pd, gd, ed = _dev(x, psi, grad, e_loc)
    xn, flag = dmc.propose(xd, pd, gd, BOX, TAU, SEED, 9, limit_drift=limit)
    psn = (psi * (1.0 + 0.2 * g.normal(size=B)) * np.where(np.arange(B) % 11 == 10, -1.0, 1.0)).astype(np.float32)
    grn = (grad + 0.3 * g.normal(size=(B, D)) * np.abs(psi)[:, None]).astype(np.float32)
    hdn = (g.normal(size=(B, D)) * np.abs(psi)[:, None]).astype(np.float32)
    hdn[np.arange(B) % 13 == 12, D - 1] = np.nan
    psnd, grnd, hdnd = _dev(psn, grn, hdn)
    return dict(x=x, psi=psi, grad=grad, e_loc=e_loc, xn=xn.cpu().numpy(), psn=psn, grn=grn, hdn=hdn, flag=flag.cpu().numpy(), limit=limit, e_cut=e_cut,
                dev=(xd, pd, gd, ed, xn, psnd, grnd, hdnd, flag))


def _run_accept(c, e_trial=-1.75):
    from waveflow_amd import dmc
    xd, pd, gd, ed, xn, psn, grn, hdn, flag = c["dev"]
    state = [t.clone() for t in (xd, pd, gd, ed)]
    out = dmc.accept(*state, xn, psn, grn, hdn, flag, PROTONS, TAU, e_trial, SEED, 9, limit_drift=c["limit"], e_cut=c["e_cut"], details=True)
    return state, out


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limited"])
@pytest.mark.parametrize("B,D", CASES, ids=IDS)
def test_acceptance_against_fp64_numpy(B, D, limit):
    from waveflow_amd import observables as obs
    e_trial = -1.75
    c = _accept_case(B, D, limit, e_cut=0.08 if D == 3 else 0.0)
    state, raw = _run_accept(c, e_trial)
    w, record, logA, u, acc = raw
    xd, pd, gd, ed, xn, psn, grn, hdn, flag = c["dev"]
    acc, u, logA, w, record = acc.cpu().numpy().astype(bool), u.cpu().numpy(), logA.cpu().numpy(), w.cpu().numpy(), record.cpu().numpy()
    # E_L' of accepted walkers: the bits of wf_observe_accumulate's values[:, 0]; everything else of the state: x', psi', grad' or untouched
    e_new_rule = obs.accumulate(xn, psn, grn, hdn, PROTONS, return_values=True)[:, 0].cpu().numpy()
    got = [t.cpu().numpy() for t in state]
    for have, old, new in ((got[0], c["x"], c["xn"]), (got[1], c["psi"], c["psn"]), (got[2], c["grad"], c["grn"]), (got[3], c["e_loc"], e_new_rule)):
        sel = acc.reshape((-1,) + (1,) * (have.ndim - 1))
        assert np.array_equal(_bits(have), _bits(np.where(sel, new, old)))
    # logA: fp64 from the fp32 inputs; only log differs between the two sides
    with np.errstate(all="ignore"):
        _, vbo = _vbar(c["psi"], c["grad"], TAU, limit)
        _, vbn = _vbar(c["psn"], c["grn"], TAU, limit)
        d = c["xn"].astype(np.float64) - c["x"].astype(np.float64)
        qf, qr = _seq_sum((d - TAU * vbo) ** 2), _seq_sum((-d - TAU * vbn) ** 2)
        t_log, t_q = 2.0 * np.log(np.abs(c["psn"].astype(np.float64)) / np.abs(c["psi"].astype(np.float64))), (qf - qr) / (2.0 * TAU)
        want_logA = t_log + t_q
    fin = np.isfinite(want_logA)
    assert np.array_equal(np.isfinite(logA), fin) and fin.sum() >= B // 2
    assert (np.abs(logA[fin] - want_logA[fin]) <= 1e-12 * (np.abs(t_log[fin]) + np.abs(t_q[fin]))).all()
    # the decisions: u < exp(min(logA, 0)) from the device's own u and logA, on top of flag, sign and finiteness
    assert (u >= 0).all() and (u < 1).all()
    with np.errstate(all="ignore"):
        A = np.where(logA >= 0, 1.0, np.exp(logA))
        fin_new = (np.isfinite(c["xn"]).all(1) & np.isfinite(c["psn"]) & np.isfinite(c["grn"]).all(1) & np.isfinite(c["hdn"]).all(1)
                   & np.isfinite(e_new_rule))
        sign = c["psn"].astype(np.float64) * c["psi"].astype(np.float64)
        allowed = (c["flag"] == 0) & (sign > 0) & fin_new
        want_acc = allowed & (u.astype(np.float64) < A)
    differ = np.flatnonzero(acc != want_acc)
    assert differ.size <= 1 and (np.abs(u[differ] - A[differ]) <= 1e-12).all()
    # the weights
    with np.errstate(all="ignore"):
        fin_old = np.isfinite(c["x"]).all(1) & np.isfinite(c["psi"]) & np.isfinite(c["grad"]).all(1) & np.isfinite(c["e_loc"])
        e_new = np.where(acc, e_new_rule, c["e_loc"]).astype(np.float64)
        ebar = (e_new + c["e_loc"].astype(np.float64)) * 0.5
        if c["e_cut"] > 0:
            win = c["e_cut"] / np.sqrt(TAU)
            ebar = np.clip(ebar, e_trial - win, e_trial + win)
        want_w = np.where(fin_old, np.exp(-TAU * (ebar - e_trial)), 0.0)
    assert np.array_equal(w == 0, ~fin_old) and (np.abs(w - want_w) <= 1e-12 * want_w).all()
    if c["e_cut"] > 0:
        assert w.max() <= np.exp(TAU * win) * (1 + 1e-12) and w[fin_old].min() >= np.exp(-TAU * win) * (1 - 1e-12)
    # the record: sums over the device's own weights, counts exact
    live = w != 0
    sums = [w[live].sum(), (w[live] * e_new[live]).sum(), (w[live] * e_new[live] ** 2).sum()]
    left = ~acc & ((c["flag"] != 0) | (sign <= 0))
    counts = [acc.sum(), left.sum(), (~acc & ~left & ~fin_new).sum()]
    assert (np.abs(record[:3] - sums) <= 1e-12 * np.abs(sums)).all() and list(record[3:]) == counts
    if B >= 257:
        assert counts[0] > B // 10 and counts[1] > 0 and counts[2] > 0 and (~acc & allowed).any()
    # bitwise the same a second time: state, weights, record, logA, u, decisions
    state2, raw2 = _run_accept(c, e_trial)
    for a, b in zip(state + list(raw), state2 + list(raw2)):
        assert np.array_equal(_bits(a), _bits(b))


# one lane, across a wave, across a block, 258 blocks (the reduce stages its rows twice), one walker beyond 1024 x 256 (the grid-stride loop
# runs twice): the smallest sizes at which each stage of the order of summation can go wrong
ORDER_BS = [1, 65, 257, 65793, 262145]


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("B", ORDER_BS)
def test_record_sums_are_the_ordered_sum_of_the_device_terms(B, D):
    """record[0 .. 2] equal, bit for bit, the sums of w, w e and (w e) e in the one order of the device's fp64 sums (_accum.ordered_sum), the
    terms formed in fp64 from the device's own weights, decisions and local energies; a walker of weight 0 (not finite) enters as 0."""
    from waveflow_amd._accum import ordered_sum
    c = _accept_case(B, D, False)
    state, (w, record, _, _, acc) = _run_accept(c)
    w, record, acc = w.cpu().numpy(), record.cpu().numpy(), acc.cpu().numpy().astype(bool)
    e = np.where(acc, state[3].cpu().numpy(), c["e_loc"]).astype(np.float64)
    live = w != 0
    assert B < 65 or (~live).any()
    with np.errstate(all="ignore"):
        terms = [np.where(live, w, 0.0), np.where(live, w * e, 0.0), np.where(live, (w * e) * e, 0.0)]
    for k in range(3):
        assert np.isfinite(record[k]) and record[k].tobytes() == ordered_sum(terms[k]).tobytes(), (k, record[k], ordered_sum(terms[k]))


def test_sign_flag_and_not_finite_each_reject_and_are_counted():
    """Proposals that would all be accepted (zero drift on both sides and psi' = psi: logA == 0, A == 1 > u), but for walker 3 (psi' of the
    other sign), walker 5 (flagged) and walker 7 (a Hessian diagonal that is not finite)."""
    import torch
    from waveflow_amd import dmc
    B, D = 64, 3
    x, psi, _, e_loc = _inputs(B, D, 77, special=False)
    grad = np.zeros((B, D), dtype=np.float32)
    xn = np.sort(x + np.float32(1e-3) * np.random.default_rng(1).normal(size=(B, D)).astype(np.float32), axis=1)
    psn, hdn, flag = psi.copy(), np.ones((B, D), dtype=np.float32), np.zeros(B, dtype=np.int32)
    psn[3] = -psi[3]
    flag[5] = 1
    hdn[7, 1] = np.inf
    xd, pd, gd, ed, xnd, psnd, hdnd, flagd = _dev(x, psi, grad, e_loc, xn, psn, hdn, flag)
    w, record, logA, u, acc = dmc.accept(xd, pd, gd, ed, xnd, psnd, gd.clone(), hdnd, flagd, PROTONS, TAU, -1.8, SEED, 0, details=True)
    acc = acc.cpu().numpy().astype(bool)
    rejected = np.isin(np.arange(B), [3, 5, 7])
    assert np.array_equal(acc, ~rejected) and logA.cpu().numpy()[~rejected].max() == 0.0
    assert list(record.cpu().numpy()[3:]) == [B - 3, 2, 1]                        # accepted; left the domain (sign, flag); not finite
    got = xd.cpu().numpy()
    assert np.array_equal(_bits(got[rejected]), _bits(x[rejected])) and np.array_equal(_bits(got[~rejected]), _bits(xn[~rejected]))
    assert bool((w > 0).all()) and bool(torch.isfinite(w).all())                  # a rejected move keeps its walker alive


# ---- reconfigure

def _weight_sets(B, seed):
    g = np.random.default_rng(seed)
    sets = {"equal": np.full(B, 0.83), "one": np.full(B, 1e-30), "bad": np.exp(0.5 * g.normal(size=B)), "zero": np.zeros(B),
            "lognormal": np.exp(g.normal(size=B))}
    sets["one"][(2 * B) // 3] = 1.0
    if B >= 8:
        sets["bad"][[0, 2, 3, B - 1]] = [np.nan, np.inf, 0.0, -1.0]
    return sets


def _check_comb(B, D, name, w, step):
    import torch
    from waveflow_amd import dmc
    x, psi, grad, e_loc = _inputs(B, D, B + D, special=False)
    xd, pd, gd, ed, wd = _dev(x, psi, grad, e_loc, w)
    status = torch.zeros(1, dtype=torch.int64, device="cuda")
    src, stats = dmc.reconfigure(xd, pd, gd, ed, wd, SEED, step, status=status)
    src, stats = src.cpu().numpy(), stats.cpu().numpy()
    want_src, want_stats, ok = dmc.comb_reference(w, dmc.comb_rand64(SEED, step))
    assert np.array_equal(src, want_src), name
    assert float(stats[:1].view(np.float64)[0]) == want_stats[0] and [int(v) for v in stats[1:]] == list(want_stats[1:]), (name, stats, want_stats)
    assert int(status.item()) == (0 if ok else 1)
    for have, old in ((xd, x), (pd, psi), (gd, grad), (ed, e_loc)):
        assert np.array_equal(_bits(have), _bits(old[want_src])), name
    assert bool((wd == 1.0).all())
    return src


@pytest.mark.parametrize("B,D", CASES, ids=IDS)
def test_comb_equals_the_integer_reference(B, D):
    for i, (name, w) in enumerate(_weight_sets(B, 31 * B + D).items()):
        src = _check_comb(B, D, name, w, step=100 + i)
        k = np.arange(B)
        if name in ("equal", "zero"):
            assert np.array_equal(src, k)
        if name == "one":
            assert (src == (2 * B) // 3).all()
        if name == "bad" and B >= 8:
            assert not np.isin(src, [0, 2, 3, B - 1]).any()
        if name == "lognormal" and B >= 63:
            assert (src < k).any() and (src > k).any()                           # the gather reads slots on both sides of the one it writes


def test_comb_at_2_pow_20_walkers():
    """The scan over 1024 blocks and both levels of the search."""
    B = 1 << 20
    w = np.exp(np.random.default_rng(5).normal(size=B))
    w[::1000] = 0.0
    src = _check_comb(B, 2, "2^20", w, step=3)
    assert src[0] >= 0 and src[-1] <= B - 1 and (np.diff(src) >= 0).all() and not np.isin(src, np.arange(0, B, 1000)).any()


# ---- with a model

def _waveflow(D, k, knots, layers, box, kind="mean", seed=7):
    from waveflow_amd import model_factory
    init = model_factory.get_waveflow_model(D, base_spline_degree=k, i_spline_degree=k, n_prior_internal_knots=knots, n_i_internal_knots=knots,
                                            i_spline_reg=0.05, n_flow_layers=layers, box_size=box, xu_coord_type=kind)
    return init(seed, D)


def _he(he_flat):
    """(model, protons): the He model of tests/test_gpu_observables.py at the shipped checkpoint"""
    import torch
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        _, psi, _, _ = _waveflow(2, 6, 23, 3, 10.0)
        psi.model.set_params_device(torch.as_tensor(np.asarray(he_flat, dtype=np.float32)).cuda())
        _cache["he"] = (psi.model, physics.system_catalogue[1]["He"][0])
    return _cache["he"]


def _three():
    """D = 3 (degree 6, 23 knots, 2 layers, box 10) at its initial parameters, two protons: the model of tests/test_gpu_observables.py"""
    import torch
    from waveflow_amd import core
    from waveflow_amd.utils import physics
    if "three" not in _cache:
        params, psi, _, _ = _waveflow(3, 6, 23, 2, 10.0)
        psi.model.set_params_device(torch.as_tensor(core.flatten_params(params).astype(np.float32)).cuda())
        _cache["three"] = (psi.model, physics.system_catalogue[1]["H2"][0])
    return _cache["three"]


def _step_against_the_route_by_hand(model, protons, B, generations, tag):
    import torch
    from waveflow_amd import dmc
    D = model.D
    box = float(model.desc.box_size)
    state = model.make_dmc_state(B, ring_len=3)                                  # shorter than the run: the ring wraps
    model.dmc_init(state, SEED, protons, exact_sampler=True)
    torch.cuda.synchronize()
    x, psi, grad, e_loc = (t.clone() for t in (state.x, state.psi, state.grad, state.e_loc))
    xs = x.cpu().numpy()
    assert np.isfinite(xs).all() and (np.abs(xs) < box).all() and (xs[:, 1:] > xs[:, :-1]).all()
    assert int(state.counter.item()) == 0 and int(state.status.item()) == 0 and not state.ring.any()
    e_trial = float(state.e_trial.item())
    assert np.isfinite(e_trial) and bool(torch.isfinite(e_loc).all())
    accepted = 0
    for g in range(generations):
        # the fixtures are no ground states (the shipped He checkpoint has <E_L> = 248): at tau = 0.05 nearly every move is
        # rejected, at 0.0005 most are accepted.  Alternating the two exercises both branches; e_cut keeps exp() in range for such energies.
        tau, e_cut = (TAU, 0.0005)[g % 2], 1.0
        xn, flag = dmc.propose(x, psi, grad, box, tau, SEED, g)
        grn, hdn, psn = model.psi_derivatives(xn, hessian_diag=True, return_psi=True)
        w, record = dmc.accept(x, psi, grad, e_loc, xn, psn, grn, hdn, flag, protons, tau, e_trial, SEED, g, e_cut=e_cut)
        dmc.reconfigure(x, psi, grad, e_loc, w, SEED, g)
        model.dmc_step(state, SEED, protons, tau, e_cut=e_cut)
        torch.cuda.synchronize()
        record = record.cpu().numpy()
        row = state.ring.cpu().numpy()[g % 3]
        for have, want in ((state.x, x), (state.psi, psi), (state.grad, grad), (state.e_loc, e_loc)):
            assert np.array_equal(_bits(have), _bits(want)), (tag, g)
        assert np.array_equal(_bits(row[:6]), _bits(record)) and row[7] == e_trial
        growth = e_trial - np.log(record[0] / B) / tau
        assert abs(row[6] - growth) <= 1e-12 * abs(growth)
        e_trial = float(record[1] / record[0])                                   # one fp64 division: the same bits on either side
        assert float(state.e_trial.item()) == e_trial and int(state.counter.item()) == g + 1
        accepted += int(record[3])
    assert int(state.status.item()) == 0 and 0 < accepted < generations * B      # both branches of the acceptance were taken
    print(f"[dmc step vs by hand, {tag}] B {B}: {generations} generations equal; acceptance {accepted / (generations * B):.3f}, E_T {e_trial:.4f}")


def test_step_is_the_route_by_hand_he_128_wave_kernels(he_flat):
    _step_against_the_route_by_hand(*_he(he_flat), 128, 4, "He")


def test_step_is_the_route_by_hand_he_16384_staged_sampler_matrix_cores(he_flat):
    _step_against_the_route_by_hand(*_he(he_flat), 16384, 2, "He")


def test_step_is_the_route_by_hand_three_particles_67():
    _step_against_the_route_by_hand(*_three(), 67, 4, "D = 3")


def test_init_from_given_walkers_replaces_the_ones_that_are_not_finite(he_flat):
    import torch
    model, protons = _he(he_flat)
    B = 96
    x = torch.as_tensor(sorted_walkers(B, 2, 6.0, 3)).cuda()
    x[5, 0] = float("nan")
    x[70, 1] = float("inf")
    state = model.make_dmc_state(B, ring_len=2)
    model.dmc_init(state, SEED, protons, walkers=x)
    xs = state.x.cpu().numpy()
    assert np.isfinite(xs).all() and bool(torch.isfinite(state.psi).all()) and bool(torch.isfinite(state.e_loc).all())
    good = x[torch.isfinite(x).all(1)].cpu().numpy()
    assert all((row == good).all(1).any() for row in xs)                         # every walker is one of the finite ones given
    assert int(state.status.item()) == 0 and int(state.counter.item()) == 0 and np.isfinite(state.e_trial.item())
    # walkers that are all finite: equal weights, so the comb is the identity and E_T the plain mean (up to the order of the fp64 sum)
    given = torch.as_tensor(good).cuda().contiguous()
    state = model.make_dmc_state(B - 2, ring_len=2)
    model.dmc_init(state, SEED, protons, walkers=given)
    assert np.array_equal(_bits(state.x), _bits(given))
    grad, hdiag, psi = model.psi_derivatives(given, hessian_diag=True, return_psi=True)
    from waveflow_amd import observables as obs
    e_loc = obs.accumulate(given, psi, grad, hdiag, protons, return_values=True)[:, 0]
    for have, want in ((state.psi, psi), (state.grad, grad), (state.e_loc, e_loc)):
        assert np.array_equal(_bits(have), _bits(want))
    e_trial = float(state.e_trial.item())
    assert abs(e_trial - float(e_loc.double().mean())) <= 1e-12 * abs(e_trial)


def _capture(model, step, restore):
    """`step` captured once, the recipe of tests/test_gpu_observables.py: a side stream, one call outside the capture, `restore()`, then the capture."""
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
    model, protons = _he(he_flat)
    B = 128
    out = {}
    for mode in ("direct", "graph"):
        state = model.make_dmc_state(B, ring_len=8)
        state.st["ws"] = model._workspace(model.dmc_workspace_bytes(B), state.device).fill_(0xFF)
        model.dmc_init(state, SEED, protons)
        kept = [t.clone() for t in state.tensors()]

        def step():
            model.dmc_step(state, SEED, protons, TAU, limit_drift=True, e_cut=2.0)

        def restore():
            for t, k in zip(state.tensors(), kept):
                t.copy_(k)
        run = _capture(model, step, restore).replay if mode == "graph" else step
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        out[mode] = [_bits(t) for t in state.tensors()]
    assert int(out["graph"][4][0]) == 5 and out["graph"][7][:5, 3].view(np.float64).min() > 0
    for a, g in zip(out["direct"], out["graph"]):
        assert np.array_equal(a, g)


def _a256(n):
    return (n + 255) // 256 * 256


def _carved(B, D):
    """The step's workspace without the sampler's pass: the parts of dmc_step_layout and of the comb's layout, each at a multiple of 256 bytes."""
    blocks = min(-(-B // 256), 1024)
    comb = 2 * 8192 + _a256(8 * B) + _a256(4 * B) + 2 * _a256(4 * B * D) + 2 * _a256(4 * B)
    return 3 * _a256(4 * B * D) + _a256(4 * B) + _a256(4 * B) + _a256(8 * B) + _a256(blocks * 48) + 256 + comb


def test_size_query_equals_the_carving_and_one_byte_less_is_refused(he_flat):
    import torch
    from waveflow_amd import dmc, observables as obs
    L = dmc.lib()
    he, protons = _he(he_flat)
    three, _ = _three()
    assert L.wf_dmc_reconfigure_workspace_bytes(128, 2) == 2 * 8192 + _a256(8 * 128) + _a256(4 * 128) + 2 * _a256(8 * 128) + 2 * _a256(4 * 128)
    # the staged sampler's pass is what the measurement step's query holds beyond its own four arrays and block partials (0 where the wave
    # sampler draws)
    for model, D, B in ((he, 2, 128), (three, 3, 67), (he, 2, 16384), (he, 2, 1 << 20)):
        pass_bytes = model.observe_step_workspace_bytes(B) - (3 * _a256(4 * B * D) + _a256(4 * B) + _a256(min(-(-B // 256), 1024) * 14 * 8))
        assert pass_bytes >= 0 and (pass_bytes > 0 or B < 16384) and model.dmc_workspace_bytes(B) == _carved(B, D) + pass_bytes, (D, B)
    B = 128
    need = he.dmc_workspace_bytes(B)
    state = he.make_dmc_state(B, ring_len=2)
    he.dmc_init(state, SEED, protons)
    before = [t.clone() for t in state.tensors()]
    pr, n_pr = he._protons(protons)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.wf_vqmc_dmc_step(he._h, ctypes.byref(state.c), SEED, B, pr, n_pr, TAU, 0, 0.0, ws.data_ptr(), need - 1, None) == -1
    assert L.wf_vqmc_dmc_init(he._h, ctypes.byref(state.c), SEED, B, pr, n_pr, 1, None, 1, ws.data_ptr(), need - 1, None) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state.tensors()))      # nothing was launched
    assert L.wf_vqmc_dmc_step(he._h, ctypes.byref(state.c), SEED, B, pr, n_pr, TAU, 0, 0.0, ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert int(state.counter.item()) == 1


def test_refusals_with_a_model(he_flat):
    import torch
    from waveflow_amd import core, dmc
    L = dmc.lib()
    he, protons = _he(he_flat)
    three, _ = _three()
    top = dmc.MAX_WALKERS
    assert L.wf_vqmc_dmc_workspace_bytes(he._h, top) > 0 and L.wf_vqmc_dmc_workspace_bytes(he._h, top + 1) == -2       # the comb's limit
    assert L.wf_vqmc_dmc_workspace_bytes(three._h, 131072) > 0 and L.wf_vqmc_dmc_workspace_bytes(three._h, 131073) == -2   # no sampler beyond
    with pytest.raises(Exception, match="status -2"):
        three.dmc_workspace_bytes(131073)
    # a 'first'-type box: walkers are not confined to |x| < L in every coordinate the same way; not covered
    params, psi, _, _ = _waveflow(2, 6, 23, 1, 10.0, kind="first")
    first = psi.model
    first.set_params_device(torch.as_tensor(core.flatten_params(params).astype(np.float32)).cuda())
    assert L.wf_vqmc_dmc_workspace_bytes(first._h, 128) == -2
    state = he.make_dmc_state(64, ring_len=2)
    before = [t.clone() for t in state.tensors()]
    pr, n_pr = he._protons(protons)
    big = 1 << 40
    one = ctypes.c_void_p(256)
    assert L.wf_vqmc_dmc_init(first._h, ctypes.byref(state.c), SEED, 64, pr, n_pr, 1, None, 1, one, big, None) == -2
    assert L.wf_vqmc_dmc_step(first._h, ctypes.byref(state.c), SEED, 64, pr, n_pr, TAU, 0, 0.0, one, big, None) == -2
    assert L.wf_vqmc_dmc_step(three._h, ctypes.byref(state.c), SEED, 131073, pr, n_pr, TAU, 0, 0.0, one, big, None) == -2
    assert L.wf_vqmc_dmc_step(he._h, ctypes.byref(state.c), SEED, top + 1, pr, n_pr, TAU, 0, 0.0, one, big, None) == -2
    assert L.wf_vqmc_dmc_step(he._h, ctypes.byref(state.c), SEED, 64, pr, n_pr, -TAU, 0, 0.0, one, big, None) == -1
    assert L.wf_vqmc_dmc_step(he._h, ctypes.byref(state.c), SEED, 64, pr, n_pr, TAU, 0, 0.0, None, big, None) == -1
    with pytest.raises(ValueError, match="columns"):
        three.dmc_step(state, SEED, protons, TAU)
    with pytest.raises(ValueError, match="walkers"):
        he.dmc_init(state, SEED, protons, walkers=torch.zeros(63, 2, device="cuda"))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state.tensors()))      # nothing was launched


# ---- known answers

def _guide(x, alpha=0.6, L=10.0):
    """psi_T = (x2 - x1) exp(-alpha (sqrt(1 + x1^2) + sqrt(1 + x2^2))) cos(pi x1 / 2L) cos(pi x2 / 2L), with its gradient and Hessian diagonal
    by torch autograd in fp64 -> float32 (psi [B], grad [B, 2], hdiag [B, 2])."""
    import torch
    xx = x.double().detach().requires_grad_(True)
    psi = ((xx[:, 1] - xx[:, 0]) * torch.exp(-alpha * torch.sqrt(1.0 + xx * xx).sum(1)) * torch.cos(np.pi * xx / (2.0 * L)).prod(1))
    grad, = torch.autograd.grad(psi.sum(), xx, create_graph=True)
    hdiag = torch.stack([torch.autograd.grad(grad[:, d].sum(), xx, retain_graph=True)[0][:, d] for d in range(2)], dim=1)
    return psi.detach().float(), grad.detach().float().contiguous(), hdiag.detach().float().contiguous()


def test_analytic_guide_reaches_the_exact_energy():
    """1024 walkers, tau = 0.05, 600 + 2000 generations through wf_dmc_propose / accept / reconfigure with the analytic guide (alpha = 0.6): the
    fixed-node energy must be the exact eigenvalue within 5 blocked standard errors (20 blocks), and lie 10 of them below the guide's own
    variational energy.  (The fp64 CPU prototype of this walk gave -1.8146 +- 0.0009 against E_VMC -1.7707, acceptance 0.996.)  The walkers
    start from |psi_T|^2: the same entries without the comb are a drift-diffusion Metropolis sampler of it, which also measures E_VMC."""
    import torch
    from waveflow_amd import dmc, observables as obs
    from waveflow_amd.utils import physics
    protons = physics.system_catalogue[1]["He"][0]
    B, tau, n_equil, n_steps = 1024, 0.05, 600, 2000
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.sort(torch.randn(B, 2, device="cuda", generator=g) * 1.5, dim=1).values.float().contiguous()
    psi, grad, hdiag = _guide(x)
    e_loc = obs.accumulate(x, psi, grad, hdiag, protons, return_values=True)[:, 0].contiguous()
    et = torch.tensor([-1.8], dtype=torch.float64, device="cuda")

    def generation(step, comb):
        xn, flag = dmc.propose(x, psi, grad, BOX, tau, SEED, step)
        psn, grn, hdn = _guide(xn)
        w, record = dmc.accept(x, psi, grad, e_loc, xn, psn, grn, hdn, flag, protons, tau, et, SEED, step)
        if comb:
            dmc.reconfigure(x, psi, grad, e_loc, w, SEED, step)
        return record
    vmc = []
    for s in range(300):                                                         # 100 to reach |psi_T|^2, 200 measured
        generation(1 << 30 | s, comb=False)
        if s >= 100:
            vmc.append(e_loc.double().mean())
    e_vmc = float(torch.stack(vmc).mean())
    records = torch.stack([generation(s, comb=True) for s in range(n_equil + n_steps)]).cpu().numpy()[n_equil:]
    e_dmc, sem = dmc.blocked_mean(records[:, 1] / records[:, 0], 20)
    acceptance = records[:, 3].sum() / (B * n_steps)
    print(f"[analytic guide] E_VMC {e_vmc:.4f}, E_DMC {e_dmc:.4f} +- {sem:.4f} (exact {E_EXACT}), acceptance {acceptance:.4f}, "
          f"left the domain {int(records[:, 4].sum())}, not finite {int(records[:, 5].sum())}")
    assert np.isfinite(records).all() and records[:, 5].sum() == 0
    assert abs(e_dmc - E_EXACT) <= 5 * sem, (e_dmc, sem)
    assert e_dmc < e_vmc - 10 * sem, (e_dmc, e_vmc, sem)


def test_trained_model_lands_between_the_exact_and_the_variational_energy(tmp_path):
    """He trained as in test_trained_energy_respects_the_variational_bound, then dmc.run with 2048 walkers, tau = 0.05, 600 + 1500 generations:
    -1.8161 - 5 SEM <= E_DMC <= E_VMC + 3 sqrt(SEM^2 + SEM_VMC^2), status zero, every ring entry finite.  (psi's signed prior may have nodes
    of its own inside the ordered domain, so equality with -1.8161 is not asserted.)"""
    from waveflow_amd import dmc, vqmc
    t = vqmc.ModelTrainer(system_name="He", learning_rate=5e-4, box_length=10, num_epochs=20000, batch_size=512, log_every=10 ** 9)
    t.save_dir = str(tmp_path / "run")
    t.exact_sampler = True
    params, _ = t.start_training(verbose=False)
    m = t.psi.model
    m.ensure_params(params)
    es = []
    for seed in range(4):
        x = m.sample(500 + seed, 1 << 15, exact=True)
        h, ps = m.hamiltonian(x, t.h_fn.protons, return_psi=True)
        es.append((h / (ps + 1e-8)).double().cpu().numpy())
    e = np.concatenate(es)
    e = e[np.isfinite(e)]
    e_vmc, sem_vmc = e.mean(), e.std() / np.sqrt(e.size)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                           # 0.05 * 600 = 30 a.u.: no equilibration warning
        r = dmc.run(m, t.h_fn.protons, 2048, 0.05, 1500, 600, SEED)
    print(f"[trained He] E_VMC {e_vmc:.4f} +- {sem_vmc:.4f}, E_DMC {r['e_dmc']:.4f} +- {r['e_dmc_stderr']:.4f} (growth {r['e_growth_mean']:.4f} +- "
          f"{r['e_growth_stderr']:.4f}; exact {E_EXACT}), acceptance {r['acceptance']:.4f}, left the domain {r['left_domain']}, "
          f"not finite {r['not_finite']}, status {r['status']}")
    sem = r["e_dmc_stderr"]
    assert r["status"] == 0 and r["generations"] == 2100 and np.isfinite(r["ring"]).all()
    assert E_EXACT - 5 * sem <= r["e_dmc"] <= e_vmc + 3 * np.sqrt(sem ** 2 + sem_vmc ** 2), (r["e_dmc"], sem, e_vmc, sem_vmc)
