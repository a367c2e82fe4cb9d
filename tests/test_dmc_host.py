"""Fixed-node DMC, host side (no GPU needed): include/waveflow_dmc.h against dmc.PROTOTYPES, dmc.DmcState and the built library; the host's
restatement of the random streams and of the comb (dmc.philox_block, dmc.comb_reference) against a plain-integer comb; what the entries and
dmc.run refuse before any launch."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from waveflow_amd import _lib, core, dmc, observables as obs, sr
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_dmc.h")
NAMES = ["wf_dmc_propose", "wf_dmc_accept_workspace_bytes", "wf_dmc_accept", "wf_dmc_reconfigure_workspace_bytes", "wf_dmc_reconfigure",
         "wf_vqmc_dmc_workspace_bytes", "wf_vqmc_dmc_init", "wf_vqmc_dmc_step"]


def test_prototype_table_matches_the_header_and_the_library():
    """dmc.PROTOTYPES against include/waveflow_dmc.h, by the method of tests/test_observables_host.py: the same functions in the same order,
    per position the same argument class; every symbol exported; dmc.lib() applies the table; nothing of it is in the existing tables, which
    keep their sizes; ABI version 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(dmc.PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = dmc.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = dmc.PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert declared["wf_dmc_propose"][1][5:10] == ["f32", "f64", "i32", "u64", "u64"]
    assert dmc.PROTOTYPES["wf_vqmc_dmc_step"][1][1] is ctypes.POINTER(dmc.DmcState)
    assert dmc.PROTOTYPES["wf_vqmc_dmc_init"][1][1] is ctypes.POINTER(dmc.DmcState)
    for table in (_lib.PROTOTYPES, sr.PROTOTYPES, sr.STEP_PROTOTYPES, sr.SPRING_PROTOTYPES, obs.PROTOTYPES):
        assert not set(declared) & set(table)
    assert len(_lib.PROTOTYPES) == 55 and len(obs.PROTOTYPES) == 4
    hdr = open(HEADER).read()
    assert '#include "waveflow_hip.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    for name, value in (("WF_DMC_RECORD", len(dmc.RECORD)), ("WF_DMC_RING_RECORD", len(dmc.RING_RECORD)), ("WF_DMC_STATS", len(dmc.STATS)),
                        ("WF_DMC_MAX_WALKERS", dmc.MAX_WALKERS)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr), name
    assert L.wf_abi_version() == 2


def test_state_struct_matches_the_header():
    """wf_dmc_state field by field: eight pointers, two int32 -- names, order, kinds, offsets and size of dmc.DmcState."""
    body = re.search(r"typedef\s+struct\s+wf_dmc_state\s*\{(.*?)\}\s*wf_dmc_state\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, name = decl.replace("*", " * ").rsplit(None, 1)
            fields.append((name, c_class(kind)))
    assert fields == [("x_dev", "pointer"), ("psi_dev", "pointer"), ("grad_dev", "pointer"), ("e_loc_dev", "pointer"), ("counter_dev", "pointer"),
                      ("e_trial_dev", "pointer"), ("ring_dev", "pointer"), ("status_dev", "pointer"), ("ring_len", "i32"), ("reserved", "i32")]
    assert [(n, ctypes_class(t)) for n, t in dmc.DmcState._fields_] == fields
    assert [getattr(dmc.DmcState, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]
    assert ctypes.sizeof(dmc.DmcState) == 72


def test_philox_and_stream_ids():
    """Philox4x32-10 at the all-zero key and counter (the known-answer vector of the Random123 distribution), and the stream ids of the header:
    bit 63 set, the purpose, step and slot fields disjoint, the step taken modulo 2^40."""
    assert dmc.philox_block(0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert dmc.philox_block(1, 0, 0) != dmc.philox_block(0, 0, 0) != dmc.philox_block(0, 1, 0) != dmc.philox_block(0, 0, 1)
    ids = {dmc.stream_id(p, s, b) for p in (0, 1, 2, 3) for s in (0, 1, (1 << 40) - 1) for b in (0, 1, (1 << 20) - 1)}
    assert len(ids) == 36 and all(i >> 63 == 1 and i < 1 << 64 for i in ids)
    assert dmc.stream_id(1, 5, 7) == (1 << 63) | (1 << 60) | (5 << 20) | 7
    assert dmc.stream_id(0, (1 << 40) + 3, 2) == dmc.stream_id(0, 3, 2)
    assert dmc.comb_rand64(9, 4) == (dmc.philox_block(9, dmc.stream_id(2, 4))[0] << 32) | dmc.philox_block(9, dmc.stream_id(2, 4))[1]
    assert dmc.comb_rand64(9, 4, purpose=3) == dmc.comb_rand64(9, 0, purpose=3) != dmc.comb_rand64(9, 0)


def _plain_comb(w, rand64):
    """The comb of the header in Python integers and loops: nothing shared with dmc.comb_reference but the quantisation's fp64 product."""
    B = len(w)
    good = [bool(np.isfinite(v) and v > 0) for v in w]
    if not any(good):
        return list(range(B)), None
    w_max = max(float(v) for v, g in zip(w, good) if g)
    scale = np.float64(4294967296.0) / np.float64(w_max)
    q = [min(int(np.float64(v) * scale), 1 << 33) if g else 0 for v, g in zip(w, good)]
    C, run = [], 0
    for v in q:
        run += v
        C.append(run)
    W = C[-1]
    S = W // B
    r = (rand64 * S) >> 64
    src = []
    for k in range(B):
        tooth = k * S + r
        src.append(next(j for j in range(B) if C[j] > tooth))
    return src, (w_max, W, S, r, max(src.count(j) for j in set(src)))


@pytest.mark.parametrize("B", [1, 5, 64, 257])
def test_comb_reference_against_plain_integers(B):
    g = np.random.default_rng(B)
    sets = {"equal": np.full(B, 0.7), "lognormal": np.exp(g.normal(size=B)), "one": np.full(B, 1e-30), "zero": np.zeros(B),
            "bad": np.exp(g.normal(size=B))}
    sets["one"][B // 2] = 1.0
    if B >= 5:
        sets["bad"][[0, 1, 2, 3]] = [np.nan, np.inf, 0.0, -1.0]
    for name, w in sets.items():
        for rand64 in (0, (1 << 64) - 1, int(g.integers(0, 1 << 63)) * 2 + 1):
            src, stats, ok = dmc.comb_reference(w, rand64)
            want, want_stats = _plain_comb(list(w), rand64)
            assert src.dtype == np.int32 and list(src) == want, (name, rand64)
            assert ok == (want_stats is not None)
            if ok:
                assert stats == want_stats, (name, rand64)
                assert stats[2] >= 4096 and 0 <= stats[3] < stats[2] and (B - 1) * stats[2] + stats[3] < stats[1] <= B << 33
            else:
                assert stats == (0.0, 0, 0, 0, 1)
            if name == "equal":
                assert list(src) == list(range(B))
            if name == "one":
                assert set(src) == {B // 2}
            if name == "bad" and B >= 5:
                assert not set(src) & {0, 1, 2, 3}
            if name == "zero":
                assert not ok and list(src) == list(range(B))


def test_comb_is_unbiased_over_its_offset():
    """Over a sweep of the offset r the number of copies of slot j averages to B w_j / sum w: the property the comb exists for."""
    w = np.array([0.2, 1.0, 0.5, 0.05, 1.7, 0.55])
    counts = np.zeros(w.size)
    n = 4096
    for i in range(n):
        src, _, _ = dmc.comb_reference(w, (i << 52) + (1 << 51))
        counts += np.bincount(src, minlength=w.size)
    assert np.abs(counts / n - w.size * w / w.sum()).max() <= 2e-3


def test_blocked_mean():
    v = np.arange(43, dtype=np.float64)
    mean, err = dmc.blocked_mean(v, 20)
    blocks = v[3:].reshape(20, 2).mean(1)
    assert mean == v.mean() and abs(err - blocks.std(ddof=1) / np.sqrt(20)) <= 1e-15
    with pytest.raises(ValueError, match="blocks"):
        dmc.blocked_mean(v[:19], 20)


def test_c_entries_refuse_bad_arguments_on_the_host():
    """What the entries decide before they look at a model or touch a device."""
    L = dmc.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    big = 1 << 40
    top = dmc.MAX_WALKERS
    assert L.wf_dmc_accept_workspace_bytes(-1) == -1 and L.wf_dmc_accept_workspace_bytes(0) == 0
    assert L.wf_dmc_accept_workspace_bytes(1) == 256 and L.wf_dmc_accept_workspace_bytes(top) == 1024 * 6 * 8
    assert L.wf_dmc_accept_workspace_bytes(top + 1) == -2
    assert L.wf_dmc_reconfigure_workspace_bytes(-1, 2) == -1 and L.wf_dmc_reconfigure_workspace_bytes(0, 2) == 0
    assert L.wf_dmc_reconfigure_workspace_bytes(8, 1) == -1 and L.wf_dmc_reconfigure_workspace_bytes(8, 9) == -1
    assert L.wf_dmc_reconfigure_workspace_bytes(top + 1, 2) == -2
    # block maxima and block sums (1024 words each), then per walker: a prefix sum, a source, one copy of x, psi, grad, e_loc
    assert L.wf_dmc_reconfigure_workspace_bytes(64, 3) == 2 * 8192 + 512 + 256 + 768 + 256 + 768 + 256

    def propose(B=8, D=2, box=10.0, tau=0.05, x=one, psi=one, grad=one, xn=one, flag=one):
        return L.wf_dmc_propose(x, psi, grad, B, D, box, tau, 0, 1, 0, xn, flag, None, None)
    assert propose(B=0) == 0 and propose(B=-1) == -1 and propose(B=top + 1) == -2
    for D in (0, 1, 9):
        assert propose(D=D) == -1, D
    for tau in (0.0, -0.1, float("nan"), float("inf")):
        assert propose(tau=tau) == -1, tau
    for box in (0.0, -1.0, float("nan"), float("inf")):
        assert propose(box=box) == -1, box
    for missing in ("x", "psi", "grad", "xn", "flag"):
        assert propose(**{missing: None}) == -1, missing

    def accept(B=8, D=2, n_pr=0, pr=None, tau=0.05, e_cut=0.0, ws=one, ws_bytes=big, **ptrs):
        p = dict.fromkeys(("x", "psi", "grad", "e", "xn", "psn", "grn", "hdn", "flag", "et", "w", "rec"), one)
        p.update(ptrs)
        return L.wf_dmc_accept(p["x"], p["psi"], p["grad"], p["e"], p["xn"], p["psn"], p["grn"], p["hdn"], p["flag"], B, D, pr, n_pr, tau, 0, e_cut,
                               p["et"], 1, 0, p["w"], p["rec"], None, None, None, ws, ws_bytes, None)
    assert accept(B=0) == 0 and accept(B=-1) == -1 and accept(B=top + 1) == -2
    assert accept(n_pr=9, pr=one) == -1 and accept(n_pr=2) == -1
    assert accept(tau=0.0) == -1 and accept(e_cut=-1.0) == -1 and accept(e_cut=float("nan")) == -1
    for missing in ("x", "psi", "grad", "e", "xn", "psn", "grn", "hdn", "flag", "et", "w", "rec"):
        assert accept(**{missing: None}) == -1, missing
    assert accept(ws=None) == -1 and accept(B=257, ws_bytes=255) == -1

    def reconfigure(B=8, D=2, ws=one, ws_bytes=big, **ptrs):
        p = dict.fromkeys(("x", "psi", "grad", "e", "w"), one)
        p.update(ptrs)
        return L.wf_dmc_reconfigure(p["x"], p["psi"], p["grad"], p["e"], p["w"], B, D, 1, 0, None, None, None, ws, ws_bytes, None)
    assert reconfigure(B=0) == 0 and reconfigure(B=-1) == -1 and reconfigure(B=top + 1) == -2 and reconfigure(D=9) == -1
    for missing in ("x", "psi", "grad", "e", "w"):
        assert reconfigure(**{missing: None}) == -1, missing
    assert reconfigure(ws=None) == -1
    assert reconfigure(B=64, D=3, ws_bytes=L.wf_dmc_reconfigure_workspace_bytes(64, 3) - 1) == -1

    assert L.wf_vqmc_dmc_workspace_bytes(None, 128) == -1 and L.wf_vqmc_dmc_workspace_bytes(one, 0) == -1
    st = dmc.DmcState(256, 256, 256, 256, 256, 256, 256, 256, 4, 0)

    def step(m=one, s=st, batch=8, pr=None, n_pr=0, tau=0.05, e_cut=0.0):
        return L.wf_vqmc_dmc_step(m, ctypes.byref(s) if s is not None else None, 1, batch, pr, n_pr, tau, 0, e_cut, one, big, None)
    assert step(m=None) == -1 and step(s=None) == -1 and step(batch=0) == -1 and step(n_pr=9, pr=one) == -1
    assert step(tau=0.0) == -1 and step(tau=float("nan")) == -1 and step(e_cut=-1.0) == -1
    assert step(s=dmc.DmcState(256, 256, 256, 256, 256, 256, 256, 256, 0, 0)) == -1             # a ring of no rows
    assert step(s=dmc.DmcState(256, 256, 256, 256, None, 256, 256, 256, 4, 0)) == -1            # no counter

    def init(m=one, s=st, batch=8, x=None, draw=1):
        return L.wf_vqmc_dmc_init(m, ctypes.byref(s) if s is not None else None, 1, batch, None, 0, 1, x, draw, one, big, None)
    assert init(m=None) == -1 and init(s=None) == -1 and init(batch=0) == -1 and init(draw=0) == -1


def _bare_model(D=2):
    """A DeviceModel that owns nothing (no GPU here): dmc.run must refuse its arguments before it needs the model."""
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = D, 0, None
    return m


def test_run_checks_its_arguments_before_it_needs_the_model():
    m = _bare_model()
    ok = dict(n_walkers=64, tau=0.05, n_steps=40, n_equil=600, seed=1)

    def run(**kw):
        a = dict(ok)
        a.update(kw)
        return dmc.run(m, [0.0], **a)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # none of these gets as far as the equilibration warning, or it is long enough
        for bad, match in ((dict(n_walkers=0), "walkers"), (dict(n_walkers=dmc.MAX_WALKERS + 1), "walkers"), (dict(tau=0.0), "tau"),
                           (dict(tau=float("nan")), "tau"), (dict(tau=-0.1), "tau"), (dict(e_cut=-1.0), "e_cut"), (dict(e_cut=float("inf")), "e_cut"),
                           (dict(n_equil=-1), "n_equil"), (dict(n_steps=19), "blocks"), (dict(n_steps=40, n_blocks=1), "blocks")):
            with pytest.raises(ValueError, match=match):
                run(**bad)
        assert dmc._check_run(64, 0.05, 40, 600, 0.0, 20) == (64, 0.05, 40, 600, 0.0, 20)
    # too short an equilibration: a warning that names the decay time, not an error
    with pytest.warns(RuntimeWarning, match=r"5\.7 a\.u\."):
        assert dmc._check_run(64, 0.01, 40, 300, 0.0, 20)[3] == 300
    with pytest.warns(RuntimeWarning, match="tau \\* n_equil"):
        dmc._check_run(64, 0.05, 40, 599, 0.0, 20)
    # the model-free bindings and the state: the same style
    import torch
    x = torch.zeros(8, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dmc.propose(x, torch.zeros(8), x, 10.0, 0.05, 1, 0)
    with pytest.raises(ValueError, match="2 .. 8"):
        dmc.propose(torch.zeros(8, 9), torch.zeros(8), x, 10.0, 0.05, 1, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dmc.State(8, 2, 4, "cpu")
    with pytest.raises(ValueError, match="ring_len"):
        dmc.State(8, 2, 0, "cpu")
    with pytest.raises(ValueError, match="tau"):
        m.dmc_step(object(), 1, [0.0], 0.0)
