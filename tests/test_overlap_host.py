"""Overlaps on the device, host side (no GPU needed): include/waveflow_overlap.h against overlap.PROTOTYPES, overlap.OverlapAcc and the built
library; the numpy restatements of the two kernels against a brute-force loop; what the entries, the Python surface and the trainer refuse
before any launch; the host-side Totals; and the normalisation convention the GPU tests rely on (2 int_{x1 < x2} psi^2 = 1), by quadrature of
the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from waveflow_amd import _lib, core, dmc, observables as obs, overlap as ov, sr, vqmc
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_overlap.h")
NAMES = ["wf_overlap_workspace_bytes", "wf_overlap_accumulate", "wf_overlap_penalise", "wf_vqmc_overlap_step_workspace_bytes", "wf_vqmc_overlap_step"]
f32, f64 = np.float32, np.float64


def test_prototype_table_matches_the_header_and_the_library():
    """overlap.PROTOTYPES against include/waveflow_overlap.h, by the method of tests/test_observables_host.py: the same functions in the same
    order, per position the same argument class; every symbol exported; overlap.lib() applies the table; nothing of it is in an existing table,
    and those keep their sizes; ABI version 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(ov.PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = ov.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = ov.PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert declared["wf_vqmc_overlap_step"][1][5] == "u64" and declared["wf_overlap_accumulate"][1][2:4] == ["i64", "i64"]
    assert ov.PROTOTYPES["wf_overlap_accumulate"][1][5] is ctypes.POINTER(ov.OverlapAcc)
    assert ov.PROTOTYPES["wf_overlap_penalise"][1][6] is ctypes.POINTER(ov.OverlapAcc)
    assert ov.PROTOTYPES["wf_vqmc_overlap_step"][1][3] is ctypes.POINTER(ov.OverlapAcc)
    for table in (_lib.PROTOTYPES, sr.PROTOTYPES, sr.STEP_PROTOTYPES, sr.SPRING_PROTOTYPES, sr.CG_PROTOTYPES, obs.PROTOTYPES, dmc.PROTOTYPES):
        assert not set(declared) & set(table)
    assert len(_lib.PROTOTYPES) == 55 and len(obs.PROTOTYPES) == 4 and len(dmc.PROTOTYPES) == 8
    hdr = open(HEADER).read()
    assert '#include "waveflow_hip.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    assert re.search(r"#define\s+WF_OVERLAP_MAX_REFS\s+8\b", hdr) and ov.MAX_REFS == 8
    assert L.wf_abi_version() == 2


def test_accumulator_struct_matches_the_header():
    body = re.search(r"typedef\s+struct\s+wf_overlap_acc\s*\{(.*?)\}\s*wf_overlap_acc\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, name = decl.replace("*", " * ").rsplit(None, 1)
            fields.append((name, c_class(kind)))
    assert fields == [("sums_dev", "pointer"), ("counts_dev", "pointer")]
    assert [(n, ctypes_class(t)) for n, t in ov.OverlapAcc._fields_] == fields
    assert [getattr(ov.OverlapAcc, n).offset for n, _ in fields] == [0, 8] and ctypes.sizeof(ov.OverlapAcc) == 16


def test_c_entries_refuse_bad_arguments_on_the_host():
    """What the five entries decide before they look at a model or touch a device."""
    L = ov.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    big = 1 << 30
    good = ov.OverlapAcc(256, 256)
    ws = L.wf_overlap_workspace_bytes
    assert ws(-1, 1) == -1 and ws(8, 0) == -1 and ws(8, 9) == -2 and ws(0, 3) == 0
    # the block partials: 2 K + 2 words of 8 bytes per block, 256 walkers per block, at most 1024 blocks, rounded up to 256 bytes
    assert ws(1, 1) == 256 and ws(257, 1) == 256 and ws(257, 8) == 512 and ws(1 << 18, 8) == ws(1 << 30, 8) == 1024 * 18 * 8
    assert ws(1 << 18, 3) == 1024 * 8 * 8

    def accumulate(acc=good, B=8, K=2, ld=8, psi=one, ref=one, ratios=None, w=one, w_bytes=big):
        return L.wf_overlap_accumulate(psi, ref, ld, B, K, ctypes.byref(acc) if acc is not None else None, ratios, w, w_bytes, None)
    assert accumulate(B=0, ld=0) == 0 and accumulate(acc=None, B=0, ld=0) == 0        # an empty batch: nothing is touched
    assert accumulate(B=-1) == -1 and accumulate(K=0) == -1 and accumulate(K=9) == -2
    assert accumulate(ld=7) == -1                                                       # rows that overlap
    assert accumulate(acc=None) == -1                                                   # neither an accumulator nor ratios
    assert accumulate(psi=None) == -1 and accumulate(ref=None) == -1
    assert accumulate(acc=ov.OverlapAcc(None, 256)) == -1 and accumulate(acc=ov.OverlapAcc(256, None)) == -1
    assert accumulate(w=None) == -1 and accumulate(B=257, ld=257, K=8, w_bytes=511) == -1

    def penalise(acc=good, B=8, K=2, ld=8, e=one, ratios=one, lam=(0.5, 0.25), out=one, no_lambda=False):
        arr = (ctypes.c_float * 8)(*lam)
        return L.wf_overlap_penalise(e, ratios, ld, B, K, None if no_lambda else ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(acc) if acc is not None else None,
                                     out, None)
    assert penalise(B=0, ld=0) == 0
    assert penalise(B=-1) == -1 and penalise(K=0) == -1 and penalise(K=9) == -2 and penalise(ld=7) == -1
    assert penalise(no_lambda=True) == -1 and penalise(acc=None) == -1 and penalise(acc=ov.OverlapAcc(None, 256)) == -1
    for lam in ((-0.5, 0.0), (0.0, -1e-30), (float("nan"), 0.0), (0.0, float("inf"))):
        assert penalise(lam=lam) == -1, lam
    assert penalise(e=None) == -1 and penalise(ratios=None) == -1 and penalise(out=None) == -1

    wsb = L.wf_vqmc_overlap_step_workspace_bytes
    assert wsb(None, 128, 1) == -1 and wsb(one, 0, 1) == -1 and wsb(one, 128, 0) == -1 and wsb(one, 128, 9) == -2
    refs = (ctypes.c_void_p * 8)(*([256] * 8))

    def step(m=one, refs=refs, K=2, acc=good, counter=one, batch=8, x=None, draw=1, ratios=None):
        return L.wf_vqmc_overlap_step(m, refs, K, ctypes.byref(acc) if acc is not None else None, counter, 1, batch, 1, x, draw, ratios, one, big, None)
    assert step(m=None) == -1 and step(refs=None) == -1 and step(batch=0) == -1 and step(K=0) == -1 and step(counter=None) == -1
    assert step(K=9) == -2
    assert step(acc=None) == -1                                                         # neither an accumulator nor ratios
    assert step(draw=0) == -1                                                           # draw = 0 without walkers
    assert step(acc=ov.OverlapAcc(None, 256)) == -1
    assert step(refs=(ctypes.c_void_p * 8)()) == -1                                     # a missing reference (looked at first: nothing is dereferenced)


# ---- the restatements against a brute-force loop

def _brute_accumulate(psi, refs):
    """One walker at a time: fp32 scalars for the ratio, python floats (fp64) summed in walker order."""
    K, B = refs.shape
    ratios = np.zeros((K, B), f32)
    sums, absum, counts = np.zeros((K, 2)), np.zeros((K, 2)), [0, 0]
    with np.errstate(all="ignore"):
        for b in range(B):
            inv = f32(1.0) / f32(psi[b] + f32(1e-8))
            ok = bool(np.isfinite(psi[b]))
            for k in range(K):
                ratios[k, b] = f32(refs[k, b] * inv)
                ok = ok and bool(np.isfinite(refs[k, b])) and bool(np.isfinite(ratios[k, b]))
            counts[0 if ok else 1] += 1
            if ok:
                for k in range(K):
                    r = float(ratios[k, b])
                    sums[k] += (r, r * r)
                    absum[k] += (abs(r), r * r)
    return ratios, sums, absum, counts


def _planted(B, K, seed):
    g = np.random.default_rng(seed)
    psi = g.normal(size=B).astype(f32)
    refs = g.normal(size=(K, B)).astype(f32)
    if B >= 8:
        psi[1] = -f32(1e-8)            # psi + 1e-8 == 0: inv = inf, the walker is skipped
        psi[2] = f32(1e-30)            # tiny but fine: inv ~ 1e8
        psi[3] = np.nan
        refs[0, 4] = np.nan
        refs[K - 1, 5] = np.inf
        refs[K - 1, 6] = -np.inf
        psi[7], refs[0, 7] = f32(3e-38), f32(3e38)   # finite inputs, but the ratio overflows for this walker only when ref / psi does
    return psi, refs


@pytest.mark.parametrize("B,K", [(1, 1), (8, 1), (37, 3), (300, 8), (64, 8)])
def test_reference_accumulate_against_a_brute_force_loop(B, K):
    psi, refs = _planted(B, K, 100 * B + K)
    ratios, sums, counts = ov.reference_accumulate(psi, refs)
    want_r, want_s, absum, want_c = _brute_accumulate(psi, refs)
    assert ratios.dtype == f32 and np.array_equal(ratios.view(np.int32), want_r.view(np.int32))
    assert counts.tolist() == want_c and counts.dtype == np.int64
    if B >= 8:
        assert want_c[1] >= 5 and not np.isfinite(ratios[0, 1])
    bound = B * 2.0 ** -53 * absum
    assert (np.abs(sums - want_s) <= bound).all(), (np.abs(sums - want_s) / np.maximum(bound, 1e-300)).max()
    # calls add: a second batch into the same sums and counts
    r2, s2, c2 = ov.reference_accumulate(psi[::-1].copy(), refs[:, ::-1].copy(), sums=sums, counts=counts)
    assert c2.tolist() == [2 * want_c[0], 2 * want_c[1]] and (np.abs(s2 - 2 * want_s) <= 4 * bound).all()
    assert np.array_equal(sums, ov.reference_accumulate(psi, refs)[1])      # the inputs were left as they were


def test_reference_accumulate_with_an_empty_count():
    psi = np.array([np.nan, -1e-8, np.inf], f32)
    refs = np.ones((2, 3), f32)
    ratios, sums, counts = ov.reference_accumulate(psi, refs)
    assert counts.tolist() == [0, 3] and not sums.any() and ratios.shape == (2, 3)
    ratios, sums, counts = ov.reference_accumulate(np.zeros(0, f32), np.zeros((2, 0), f32))
    assert counts.tolist() == [0, 0] and not sums.any() and ratios.shape == (2, 0)
    with pytest.raises(ValueError, match="shape"):
        ov.reference_accumulate(np.zeros(3, f32), np.zeros((2, 4), f32))
    with pytest.raises(ValueError, match="1 .. 8"):
        ov.reference_accumulate(np.zeros(3, f32), np.zeros((9, 3), f32))


@pytest.mark.parametrize("B,K", [(8, 1), (37, 3), (300, 8)])
def test_reference_penalise_against_a_brute_force_loop(B, K):
    psi, refs = _planted(B, K, 7 * B + K)
    ratios, sums, counts = ov.reference_accumulate(psi, refs)
    e = np.random.default_rng(B).normal(size=B).astype(f32) - f32(1.8)
    lam = np.linspace(0.25, 2.0, K)
    got = ov.reference_penalise(e, ratios, sums, counts, lam)
    n = int(counts[0])
    want = np.zeros(B, f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            s = float(e[b])
            for k in range(K):
                a = float(sums[k, 0]) / float(n)
                s = s + (float(f32(lam[k])) * a) * (float(ratios[k, b]) - a)
            want[b] = f32(s) if np.isfinite(ratios[:, b]).all() else e[b]
    assert got.dtype == f32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    passed = ~np.isfinite(ratios).all(0)
    assert passed.sum() >= 5 and np.array_equal(got[passed], e[passed]) and (got[~passed] != e[~passed]).any()
    # one number for every state; lambda = 0 changes nothing that is finite; an empty count passes everything through
    assert np.array_equal(ov.reference_penalise(e, ratios, sums, counts, 0.5), ov.reference_penalise(e, ratios, sums, counts, [0.5] * K))
    assert np.array_equal(ov.reference_penalise(e, ratios, sums, counts, 0.0), e)
    assert np.array_equal(ov.reference_penalise(e, ratios, np.zeros((K, 2)), [0, B], lam), e)
    for bad in (-1.0, [0.5] * (K + 1), float("nan")):
        with pytest.raises(ValueError, match="overlap_penalty"):
            ov.reference_penalise(e, ratios, sums, counts, bad)


def test_the_penalty_gradient_is_the_gradient_of_the_penalty():
    """sum_b (e~_b - e_b) O_b / B with O = d ln psi: for a one-parameter family psi_t = cos t psi + sin t chi (both normalised, <chi|psi> = 0)
    on a grid, the derivative of lambda S(t)^2 is twice that mean of (e~ - e) (O - mean O) -- the statement the optimisers rely on."""
    x = np.linspace(-6, 6, 4001)
    w = x[1] - x[0]
    g0 = np.exp(-x * x / 2)
    g0 /= np.sqrt((g0 * g0).sum() * w)
    g1 = x * g0
    g1 /= np.sqrt((g1 * g1).sum() * w)
    ref = (g0 + 0.5 * g1) / np.sqrt(1.25)
    lam, t = 0.7, 0.3
    psi, dpsi = np.cos(t) * g0 + np.sin(t) * g1, -np.sin(t) * g0 + np.cos(t) * g1
    p = psi * psi * w                                   # the law of the walkers
    r, O = ref / psi, dpsi / psi
    a = (p * r).sum()
    e_shift = lam * a * (r - a)                          # e~ - e
    grad = 2 * (p * e_shift * (O - (p * O).sum())).sum()
    S = lambda s: ((np.cos(s) * g0 + np.sin(s) * g1) * ref).sum() * w
    h = 1e-5
    assert abs(grad - lam * (S(t + h) ** 2 - S(t - h) ** 2) / (2 * h)) < 1e-7


# ---- the Python surface

def _bare_model(D=2):
    """A DeviceModel that owns nothing (no GPU here): overlap_step must refuse its arguments before it needs more than the walker width."""
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = D, 0, None
    return m


def test_python_surface_refuses_before_any_launch():
    import torch
    m, other = _bare_model(), _bare_model(3)
    acc, counter = object(), object()   # never looked at
    with pytest.raises(ValueError, match="1 .. 8"):
        m.overlap_step([], acc, counter, 1, 8)
    with pytest.raises(ValueError, match="1 .. 8"):
        m.overlap_step([m] * 9, acc, counter, 1, 8)
    with pytest.raises(ValueError, match="at least 1"):
        m.overlap_step([m], acc, counter, 1, 0)
    for bad in (torch.zeros(8, 3), torch.zeros(7, 2), torch.zeros(16)):
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.overlap_step([m], acc, counter, 1, 8, walkers=bad)
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.overlap_step([m], acc, counter, 1, 8, out_walkers=bad)
    with pytest.raises(ValueError, match=r"shape \[3, 8\]"):
        m.overlap_step([m] * 3, acc, counter, 1, 8, ratios=torch.zeros(8, 3))
    with pytest.raises(ValueError, match="float32"):
        m.overlap_step([m], acc, counter, 1, 8, walkers=torch.zeros(8, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        m.overlap_step([m, m], acc, counter, 1, 8, ratios=torch.zeros(8, 2).t())         # not contiguous
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.overlap_step([m], acc, counter, 1, 8, walkers=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.overlap_step([m], acc, counter, 1, 8, ratios=torch.zeros(1, 8))
    with pytest.raises(ValueError, match="exclude"):
        m.overlap_step([m], acc, counter, 1, 8, walkers=torch.zeros(8, 2), out_walkers=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="every reference"):
        m.overlap_step([m, other], acc, counter, 1, 8)                                   # another n_dim
    with pytest.raises(ValueError, match="every reference"):
        m.overlap_step([object()], acc, counter, 1, 8)
    elsewhere = _bare_model()
    elsewhere.device = 1
    with pytest.raises(ValueError, match="every reference"):
        m.overlap_step([elsewhere], acc, counter, 1, 8)                                  # another device
    with pytest.raises(ValueError, match="nothing to do"):
        m.overlap_step([m], None, counter, 1, 8)
    with pytest.raises(ValueError, match="overlap.Accumulator"):
        m.overlap_step([m], acc, counter, 1, 8)
    # the model-free bindings and the accumulator
    psi, refs = torch.zeros(8), torch.zeros(2, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ov.accumulate(psi, refs)
    with pytest.raises(ValueError, match=r"psi must be a torch tensor of shape \[B\]"):
        ov.accumulate(torch.zeros(8, 1), refs)
    with pytest.raises(ValueError, match="1 .. 8"):
        ov.accumulate(psi, torch.zeros(9, 8))
    with pytest.raises(ValueError, match=r"shape \[2, 8\]"):
        ov.accumulate(psi, torch.zeros(2, 7))
    with pytest.raises(ValueError, match="2-d"):
        ov.accumulate(psi, torch.zeros(8))
    with pytest.raises(ValueError, match="float32"):
        ov.accumulate(psi, torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous rows"):
        ov.accumulate(psi, torch.zeros(8, 2).t())
    with pytest.raises(ValueError, match="no CPU fallback"):
        ov.penalise(psi, refs, acc, 0.5)
    with pytest.raises(ValueError, match="2-d"):
        ov.penalise(psi, psi, acc, 0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ov.Accumulator(2, device="cpu")
    with pytest.raises(ValueError, match="1 .. 8"):
        ov.Accumulator(0, device="cpu")
    with pytest.raises(ValueError, match="1 .. 8"):
        ov.Accumulator(9, device="cpu")
    with pytest.raises(ValueError, match=">= 1"):
        ov.measure(m, [m], 0, 8, 1)
    with pytest.raises(ValueError, match="1 .. 8"):
        ov.measure(m, [], 8, 8, 1)
    with pytest.raises(ValueError, match="2 .. 8"):
        ov.overlap_matrix([m], 8, 8, 1)
    for bad, K in ((-0.1, 1), ([0.1, 0.2], 3), (float("inf"), 1), ([0.1, float("nan")], 2)):
        with pytest.raises(ValueError, match="overlap_penalty"):
            ov._check_penalty(bad, K)
    assert ov._check_penalty(0.5, 3).tolist() == [0.5] * 3 and ov._check_penalty([1, 2], 2).dtype == f32


def test_training_functions_refuse_bad_lower_states_before_any_launch():
    """The four functions of vqmc.py check lower_states and overlap_penalty before they touch the model (which is a fake here)."""
    class Fake:
        model = object()
    psi, bad_psi = Fake(), object()
    calls = {"sr_natural_gradient": lambda **k: vqmc.sr_natural_gradient(None, psi, None, None, **k),
             "spring_direction": lambda **k: vqmc.spring_direction(None, psi, None, None, None, 0.9, **k),
             "train_step_sr": lambda **k: vqmc.train_step_sr(1, psi, None, None, None, 0.1, **k),
             "train_step_spring": lambda **k: vqmc.train_step_spring(1, psi, None, None, None, 0.1, None, 0.9, 0.1, 5.0, **k)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="overlap_penalty"):
            call(lower_states=[(psi, None)], overlap_penalty=-1.0)
        with pytest.raises(ValueError, match="overlap_penalty"):
            call(lower_states=[(psi, None)], overlap_penalty=[0.1, 0.2])
        with pytest.raises(ValueError, match="lower_states must be a list"):
            call(lower_states=[(bad_psi, None)], overlap_penalty=0.5)
        with pytest.raises(ValueError, match="lower_states must be a list"):
            call(lower_states=[psi], overlap_penalty=0.5)
        with pytest.raises(ValueError, match="1 .. 8"):
            call(lower_states=[(psi, None)] * 9, overlap_penalty=0.5)
    import inspect
    for f in (vqmc.sr_natural_gradient, vqmc.spring_direction, vqmc.train_step_sr, vqmc.train_step_spring):
        p = inspect.signature(f).parameters
        assert p["lower_states"].kind is inspect.Parameter.KEYWORD_ONLY and p["lower_states"].default is None, f.__name__
        assert p["overlap_penalty"].kind is inspect.Parameter.KEYWORD_ONLY and p["overlap_penalty"].default == 0.0, f.__name__
    assert vqmc._overlap_args(None, 0.5, None) == {} and vqmc._overlap_args([], 0.5, None) == {}


def test_trainer_refuses_lower_states_where_no_step_honours_them(tmp_path):
    def trainer(**attrs):
        t = vqmc.ModelTrainer(system_name="He", learning_rate=1e-2, box_length=10, num_epochs=1, batch_size=8)
        t.save_dir = str(tmp_path / "run")
        for k, v in attrs.items():
            setattr(t, k, v)
        return t
    t0 = trainer()
    assert t0.lower_states == [] and t0.overlap_penalty == 0.0
    lower = [np.zeros(4, f32)]
    with pytest.raises(ValueError, match="lower_states.*optimizer='adam'"):
        trainer(lower_states=lower).start_training(verbose=False)
    for opt in ("sr", "spring"):
        with pytest.raises(ValueError, match="lower_states.*sr_on_device"):
            trainer(lower_states=lower, optimizer=opt, sr_on_device=True).start_training(verbose=False)
        with pytest.raises(ValueError, match="overlap_penalty"):
            trainer(lower_states=lower, optimizer=opt, overlap_penalty=-0.5).start_training(verbose=False)
        with pytest.raises(ValueError, match="overlap_penalty"):
            trainer(lower_states=lower, optimizer=opt, overlap_penalty=[0.1, 0.2]).start_training(verbose=False)
        with pytest.raises(ValueError, match="lower_states.*1 .. 8"):
            trainer(lower_states=lower * 9, optimizer=opt).start_training(verbose=False)
    # the existing refusal stays, with or without lower states
    with pytest.raises(ValueError, match="sr_solver='cg' with sr_on_device=True"):
        trainer(optimizer="sr", sr_solver="cg", sr_on_device=True).start_training(verbose=False)
    with pytest.raises(ValueError, match="sr_solver='cg' with sr_on_device=True"):
        trainer(lower_states=lower, optimizer="sr", sr_solver="cg", sr_on_device=True).start_training(verbose=False)
    assert t0._check_lower_state_settings("adam") is None and trainer(lower_states=None)._check_lower_state_settings("adam") is None
    assert trainer(lower_states=lower, overlap_penalty=0.4)._check_lower_state_settings("spring").tolist() == [f32(0.4)]


def test_an_excited_state_must_not_start_on_the_state_it_avoids():
    g = np.random.default_rng(3)
    a = g.normal(size=50).astype(f32)
    b = a.copy()
    with pytest.raises(ValueError, match=r"lower_states\[2\] equals this trainer's initial parameters bit for bit"):
        vqmc._check_distinct_start(a, b, 2)
    b[17] = np.nextafter(b[17], f32(np.inf))
    vqmc._check_distinct_start(a, b, 0)          # one ulp apart: another point
    vqmc._check_distinct_start(a, a[:49], 0)     # another size is the size check's business
    z = np.zeros(4, f32)
    vqmc._check_distinct_start(z, -z, 0)         # -0.0 is not +0.0 bit for bit


def test_totals_merge_result_and_shapes():
    g = np.random.default_rng(5)
    r = g.normal(size=(3, 1000)) * 0.3 + np.array([[0.6], [0.0], [-0.2]])
    t = ov.Totals(3, sums=np.stack([r.sum(1), (r * r).sum(1)], axis=1), counts=[1000, 4])
    res = t.result()
    assert res["n"] == 1000 and res["n_skipped"] == 4
    assert np.allclose(res["overlap"], r.mean(1), rtol=0, atol=1e-15)
    assert np.allclose(res["stderr"], np.sqrt(r.var(1) / 1000), rtol=1e-12, atol=0)
    u = ov.Totals(3, sums=np.ones((3, 2)), counts=[2, 1])
    want_s, want_c = t.sums + u.sums, t.counts + u.counts
    assert t.merge(u) is t and np.array_equal(t.sums, want_s) and np.array_equal(t.counts, want_c) and t.counts.dtype == np.int64
    with pytest.raises(ValueError, match="cannot merge"):
        t.merge(ov.Totals(2))
    with pytest.raises(ValueError, match="shape"):
        ov.Totals(3, sums=np.zeros((2, 2)))
    empty = ov.Totals(2).result()
    assert empty["n"] == 0 and np.isnan(empty["overlap"]).all() and np.isnan(empty["stderr"]).all()


# ---- the normalisation convention

def test_waveflow_psi_is_normalised_and_the_quadrature_overlap():
    """The oracle's He model at the shipped checkpoint (pa) and at pb = pa + 0.05 N(0, 1): midpoint quadrature over x1 < x2 on a 300 x 300
    grid of [-10, 10]^2 in fp64.  2 int psi_a^2 and 2 int psi_b^2 are 1 within 2e-3 (measured 1.00097, 1.00103) and 2 int psi_a psi_b is
    0.60735 within 1e-4 (measured 0.607354; 0.607346 at 600^2 and 1200^2): S = E_{|psi|^2}[psi_k / psi] needs no norm estimate."""
    import oracle
    pa = np.load(os.path.join(ROOT, "tests", "golden", "he_checkpoint.npz"))["flat"].astype(f32)
    pb = (pa + 0.05 * np.random.default_rng(0).standard_normal(pa.shape)).astype(f32)
    n = 300
    h = 20.0 / n
    mid = -10.0 + (np.arange(n) + 0.5) * h
    i, j = np.triu_indices(n, 1)                     # cells whose midpoint has x1 < x2
    x = np.stack([mid[i], mid[j]], axis=1)
    m = oracle.he_model(10.0)
    a = m.psi(pa, x, threads=4, f64=True).astype(f64)
    b = m.psi(pb, x, threads=4, f64=True).astype(f64)
    naa, nbb, sab = 2 * (a * a).sum() * h * h, 2 * (b * b).sum() * h * h, 2 * (a * b).sum() * h * h
    print(f"[normalisation] 2 int psi_a^2 = {naa:.6f}, 2 int psi_b^2 = {nbb:.6f}, 2 int psi_a psi_b = {sab:.6f}")
    assert abs(naa - 1) < 2e-3 and abs(nbb - 1) < 2e-3
    assert abs(sab - 0.60735) < 1e-4
