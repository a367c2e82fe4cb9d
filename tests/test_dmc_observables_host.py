"""Forward walking behind the DMC comb, host side (no GPU needed): include/waveflow_dmc_observe.h against dmc_observables.PROTOTYPES,
dmc_observables.DmcFw and the built library, by the method of tests/test_dmc_host.py; the host's restatement of the update rule
(dmc_observables.reference_update) against a brute-force genealogy that stores every generation's src and walks back; what the entries and the
bindings refuse before any launch."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from waveflow_amd import _lib, core, dmc, dmc_observables as fwo, observables as obs, sr
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_dmc_observe.h")
NAMES = ["wf_dmc_fw_workspace_bytes", "wf_dmc_fw_update", "wf_vqmc_dmc_fw_workspace_bytes", "wf_vqmc_dmc_fw_step"]
PROTONS = [-0.7, 0.4]


def test_prototype_table_matches_the_header_and_the_library():
    """dmc_observables.PROTOTYPES against the header: the same functions in the same order, per position the same argument class; every symbol
    exported; lib() applies the table; nothing of it is in an existing table, and those keep their sizes; ABI version 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(fwo.PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = fwo.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = fwo.PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert fwo.PROTOTYPES["wf_dmc_fw_update"][1][6] is ctypes.POINTER(fwo.DmcFw)
    assert fwo.PROTOTYPES["wf_vqmc_dmc_fw_step"][1][1] is ctypes.POINTER(dmc.DmcState)
    assert fwo.PROTOTYPES["wf_vqmc_dmc_fw_step"][1][2] is ctypes.POINTER(fwo.DmcFw)
    assert declared["wf_vqmc_dmc_fw_step"][1][3:10] == ["u64", "i64", "pointer", "i32", "f64", "i32", "f64"]
    for table in (_lib.PROTOTYPES, sr.PROTOTYPES, sr.STEP_PROTOTYPES, sr.SPRING_PROTOTYPES, obs.PROTOTYPES, dmc.PROTOTYPES):
        assert not set(declared) & set(table)
    assert len(_lib.PROTOTYPES) == 55 and len(obs.PROTOTYPES) == 4 and len(dmc.PROTOTYPES) == 8
    hdr = open(HEADER).read()
    assert '#include "waveflow_dmc.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    for name, value in (("WF_DMC_FW_MAX_SLOTS", fwo.MAX_SLOTS), ("WF_DMC_FW_COUNTS", len(fwo.COUNTS)), ("WF_DMC_FW_SERIES", len(fwo.SERIES))):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr), name
    assert re.search(r"#define\s+WF_DMC_FW_EMPTY\s+0x(F{16})ull", hdr) and fwo.EMPTY == 0xFFFFFFFFFFFFFFFF
    assert L.wf_abi_version() == 2


def test_tracker_struct_matches_the_header():
    """wf_dmc_fw field by field: nine pointers, then eight 4-byte fields -- names, order, kinds, offsets and size of dmc_observables.DmcFw."""
    body = re.search(r"typedef\s+struct\s+wf_dmc_fw\s*\{(.*?)\}\s*wf_dmc_fw\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, names = decl.replace("*", " * ").split(None, 1) if "*" not in decl else decl.replace("*", " * ").rsplit(None, 1)
            for name in names.split(","):                                   # (float lo, hi;)
                fields.append((name.strip(), c_class(kind)))
    want = [(n, "pointer") for n in ("snap_dev", "anc_dev", "tag_dev", "counts_dev", "density_dev", "pair_dev", "sums_dev", "measurements_dev",
                                     "series_dev")]
    want += [("n_slots", "i32"), ("stride", "i32"), ("series_len", "i32"), ("n_density_bins", "i32"), ("n_pair_bins", "i32"), ("lo", "f32"),
             ("hi", "f32"), ("reserved", "i32")]
    assert fields == want
    assert [(n, ctypes_class(t)) for n, t in fwo.DmcFw._fields_] == want
    assert [getattr(fwo.DmcFw, n).offset for n, _ in want] == [8 * i for i in range(9)] + [72 + 4 * i for i in range(8)]
    assert ctypes.sizeof(fwo.DmcFw) == 104


# ---- the reference against a brute-force genealogy

def _brute_force_ancestor(history, B, g, tag):
    """The slot at tag time that every walker of generation g descends from: the stored src of generations g, g - 1, ..., tag + 1, walked back
    one walker at a time in Python integers."""
    out = []
    for k in range(B):
        at = k
        for gen in range(g, tag, -1):
            src = history[gen]
            at = at if src is None else min(max(int(src[at]), 0), B - 1)
        out.append(at)
    return out


@pytest.mark.parametrize("B,n_slots,stride", [(1, 1, 1), (5, 3, 2), (64, 16, 1)])
def test_reference_update_against_a_brute_force_genealogy(B, n_slots, stride):
    D = 2
    rng = np.random.default_rng(100 * B + n_slots)
    ref = fwo.Reference(B, D, n_slots, stride, 16, 16, -4.0, 4.0, 5)
    history, walkers = {}, {}
    x = np.sort(rng.normal(size=(B, D)), axis=1).astype(np.float32)
    n_gen = 3 * n_slots * stride + 2
    measured_at = []
    for g in range(1, n_gen + 1):
        kind = g % 4
        src = None if kind == 0 else rng.integers(0, B, size=B).astype(np.int32)      # random, with repeats, not monotone; or the identity
        if kind == 2:
            src[rng.integers(0, B)] = B + 7                                             # out of range: clamped
            src[rng.integers(0, B)] = -3
        x = (x if src is None else x[np.clip(src, 0, B - 1)]) + rng.normal(size=(B, D)).astype(np.float32) * np.float32(0.1)
        if g == 4 and B > 1:
            x[1, 0] = np.nan
        history[g], walkers[g] = src, x.copy()
        counts_before = ref.counts.copy()
        got = fwo.reference_update(ref, x, src, PROTONS, g)
        assert (got != []) == (g % stride == 0)
        if g % stride:
            assert np.array_equal(ref.counts, counts_before)
            tags_now = list(ref.tag)
        else:
            measured_at.append(g)
            # what was measured: lag 0 is x; lag j the walkers of generation g - j stride, each counted once per descendant
            lags = dict(got)
            assert np.array_equal(lags[0], x, equal_nan=True)
            for j in range(1, n_slots + 1):
                t = g - j * stride
                if t >= stride:                                                          # tagged generations: the multiples of the stride
                    want = walkers[t][_brute_force_ancestor(history, B, g, t)]
                    assert np.array_equal(lags[j], want, equal_nan=True), (g, j)
                    assert ref.series[(len(measured_at) - 1) % 5, j, 3] == len(set(_brute_force_ancestor(history, B, g, t)))
                else:
                    assert j not in lags
            assert ref.tag[(g // stride) % n_slots] == g
        # every tagged slot: anc is the brute-force ancestor, snap the walkers of the tag's generation
        for s, t in enumerate(ref.tag):
            if t == fwo.EMPTY:
                continue
            assert t % stride == 0 and (t // stride) % n_slots == s and g - t < n_slots * stride
            assert list(ref.anc[s]) == _brute_force_ancestor(history, B, g, t), (g, s)
            assert np.array_equal(ref.snap[s], walkers[t], equal_nan=True)
    assert ref.measurements == len(measured_at) == n_gen // stride
    # the accumulators: every measured configuration is counted or skipped; every counted one is in a bin or outside
    total = ref.counts[:, 0] + ref.counts[:, 1]
    assert total[0] == B * len(measured_at) and (total % B == 0).all() and total[n_slots] > 0
    assert (ref.density.sum(axis=(1, 2)) + ref.counts[:, 2] == D * ref.counts[:, 0]).all()
    assert (ref.pair.sum(axis=1) + ref.counts[:, 3] == ref.counts[:, 0]).all()
    if B > 1:
        assert ref.counts[:, 1].sum() > 0                                               # the NaN walker was skipped, at lag 0 and as an ancestor
    # zeroing the accumulators leaves the genealogy alone
    tags, anc = list(ref.tag), ref.anc.copy()
    ref.zero_accumulators()
    assert ref.measurements == 0 and not ref.counts.any() and not ref.series.any() and list(ref.tag) == tags and np.array_equal(ref.anc, anc)


def test_reference_bins_and_potentials():
    """The bin rule of waveflow_observe.h (nextafter(hi, lo) lands outside; lo lands in bin 0) and the potentials against fp64."""
    ref = fwo.Reference(4, 2, 1, 1, 8, 8, -2.0, 2.0, 1)
    x = np.array([[-2.0, 0.0], [np.nextafter(np.float32(2.0), np.float32(0.0)), 2.5], [-0.5, 0.5], [np.inf, 0.0]], dtype=np.float32)
    fwo.reference_update(ref, x, None, PROTONS, 1)
    assert list(ref.counts[0]) == [3, 1, 2, 0]                  # counted, skipped (inf), outside the density range: x = 2 - ulp and 2.5
    assert ref.density[0, 0, 0] == 1 and ref.density[0, 1, 4] == 1 and ref.density[0, 0, 3] == 1 and ref.density[0, 1, 5] == 1
    assert ref.pair[0, 4] == 1 and ref.pair[0, 1] == 1 and ref.pair[0, 2] == 1 and ref.pair[0].sum() == 3   # distances 2, 0.5 + ulp, 1
    v_en, v_ee = fwo.potentials(x[:3], PROTONS)
    x64, p64 = x[:3].astype(np.float64), np.array(PROTONS)
    want_en = -(1.0 / np.sqrt(1.0 + (p64[None, :, None] - x64[:, None, :]) ** 2)).sum(axis=(1, 2))
    want_ee = 1.0 / np.sqrt(1.0 + (x64[:, 1] - x64[:, 0]) ** 2)
    assert v_en.dtype == np.float32 and np.abs(v_en - want_en).max() <= 4 * 2.0 ** -23 * np.abs(want_en).max()
    assert np.abs(v_ee - want_ee).max() <= 4 * 2.0 ** -23
    assert np.allclose(ref.sums[0, :, 0], [v_en.astype(np.float64).sum(), v_ee.astype(np.float64).sum()], rtol=1e-15)


def test_result_and_extrapolated_on_the_host():
    B, S = 32, 2
    rng = np.random.default_rng(3)
    ref = fwo.Reference(B, 2, S, 1, 20, 20, -5.0, 5.0, 8)
    for g in range(1, 13):
        x = np.sort(rng.normal(size=(B, 2)), axis=1).astype(np.float32)
        fwo.reference_update(ref, x, rng.integers(0, B, size=B).astype(np.int32), PROTONS, g)
    r = fwo.result(ref, n_blocks=4)
    assert list(r["lag"]) == [0, 1, 2] and list(r["n"]) == [12 * B, 11 * B, 10 * B] and r["measurements"] == 12
    assert list(r["n_measurements"]) == [8, 8, 8]                                       # the series keeps the last 8
    assert np.allclose(r["v_en"], ref.sums[:, 0, 0] / r["n"]) and np.isfinite(r["v_en_stderr"]).all() and (r["v_ee_stderr"] > 0).all()
    assert r["distinct_fraction"][0] == 1.0 and 0 < r["distinct_fraction"][2] < r["distinct_fraction"][1] < 1
    w = 10.0 / 20
    assert np.allclose(r["density"].sum(axis=1) * w, 2.0) and np.allclose(r["pair"].sum(axis=1) * w, 1.0)
    assert np.isnan(fwo.result(ref, n_blocks=9)["v_en_stderr"]).all()                   # fewer measurements than blocks: no error bar
    vmc = obs.Totals(2, 20, 20, -5.0, 5.0, sums=np.array([[0, 0], [0, 0], [0, 0], [-20.0, 50.0], [4.0, 2.0]]), counts=[10, 0, 0, 0],
                     density=np.full((2, 20), 1), pair=np.full(20, 1))
    e = fwo.extrapolated(r, vmc)
    assert e["v_en"] == 2 * r["v_en"][0] + 2.0 and e["v_ee"] == 2 * r["v_ee"][0] - 0.4
    assert np.allclose(e["density"], 2 * r["density"][0] - vmc.result()["density"]) and e["pair"].shape == (20,)
    with pytest.raises(ValueError, match="binned differently"):
        fwo.extrapolated(r, obs.Totals(2, 10, 20, -5.0, 5.0, counts=[1, 0, 0, 0]))


# ---- refusals

def test_c_entries_refuse_bad_arguments_on_the_host():
    """What the entries decide before they look at a model or touch a device."""
    L = fwo.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    big, top = 1 << 40, dmc.MAX_WALKERS
    q = L.wf_dmc_fw_workspace_bytes
    assert q(-1, 2, 1) == -1 and q(0, 2, 1) == 0 and q(8, 1, 1) == -1 and q(8, 9, 1) == -1 and q(8, 2, 0) == -1 and q(8, 2, 17) == -1
    assert q(top + 1, 2, 1) == -2 and q(top, 2, 16) > 0
    # the composed anc (int32), the marks (bytes), the block partials (8 words of 8 bytes per lag and block), 17 words: each to 256 bytes
    assert q(64, 3, 2) == 512 + 256 + 256 + 256 and q(4099, 2, 3) == 49408 + 12544 + 4 * 17 * 64 + 256

    def tracker(**kw):
        f = dict(snap_dev=256, anc_dev=256, tag_dev=256, counts_dev=256, density_dev=256, pair_dev=256, sums_dev=256, measurements_dev=256,
                 series_dev=256, n_slots=2, stride=1, series_len=4, n_density_bins=8, n_pair_bins=8, lo=-1.0, hi=1.0, reserved=0)
        f.update(kw)
        return fwo.DmcFw(**f)

    def update(B=8, D=2, n_pr=0, pr=None, fw=tracker(), x=one, gen=one, ws=one, ws_bytes=big):
        return L.wf_dmc_fw_update(x, None, B, D, pr, n_pr, ctypes.byref(fw) if fw is not None else None, gen, ws, ws_bytes, None)
    assert update(B=0) == 0 and update(B=-1) == -1 and update(B=top + 1) == -2
    for D in (0, 1, 9):
        assert update(D=D) == -1, D
    assert update(n_pr=9, pr=one) == -1 and update(n_pr=2) == -1 and update(fw=None) == -1
    for bad in (dict(n_slots=0), dict(n_slots=17), dict(stride=0), dict(series_len=0), dict(n_density_bins=-1), dict(n_pair_bins=-1),
                dict(lo=1.0, hi=1.0), dict(lo=2.0), dict(lo=float("nan")), dict(hi=float("inf")), dict(snap_dev=None), dict(anc_dev=None),
                dict(tag_dev=None), dict(counts_dev=None), dict(density_dev=None), dict(pair_dev=None), dict(sums_dev=None),
                dict(measurements_dev=None), dict(series_dev=None)):
        assert update(fw=tracker(**bad)) == -1, bad
    assert update(fw=tracker(n_density_bins=513)) == -2 and update(fw=tracker(n_pair_bins=1025)) == -2
    assert update(B=0, fw=tracker(n_slots=0)) == -1                                       # the tracker is checked before B == 0 returns
    assert update(x=None) == -1 and update(gen=None) == -1 and update(ws=None) == -1
    assert update(B=64, D=3, ws_bytes=q(64, 3, 2) - 1) == -1

    assert L.wf_vqmc_dmc_fw_workspace_bytes(None, 128, 2) == -1 and L.wf_vqmc_dmc_fw_workspace_bytes(one, 0, 2) == -1
    st = dmc.DmcState(256, 256, 256, 256, 256, 256, 256, 256, 4, 0)

    def step(m=one, s=st, fw=tracker(), batch=8, pr=None, n_pr=0, tau=0.05, e_cut=0.0):
        return L.wf_vqmc_dmc_fw_step(m, ctypes.byref(s) if s is not None else None, ctypes.byref(fw) if fw is not None else None, 1, batch, pr, n_pr,
                                     tau, 0, e_cut, one, big, None)
    assert step(m=None) == -1 and step(s=None) == -1 and step(batch=0) == -1 and step(n_pr=9, pr=one) == -1
    assert step(tau=0.0) == -1 and step(tau=float("nan")) == -1 and step(e_cut=-1.0) == -1
    assert step(s=dmc.DmcState(256, 256, 256, 256, None, 256, 256, 256, 4, 0)) == -1


def test_bindings_check_their_arguments_before_anything_is_launched():
    import torch
    ok = dict(n_walkers=8, D=2, n_slots=2, stride=1, n_density_bins=8, n_pair_bins=8, lo=-1.0, hi=1.0, series_len=4, device="cpu")
    for bad, match in ((dict(n_walkers=0), "walkers"), (dict(n_walkers=dmc.MAX_WALKERS + 1), "walkers"), (dict(D=9), "2 .. 8"),
                       (dict(n_slots=0), "tag slots"), (dict(n_slots=17), "tag slots"), (dict(stride=0), "stride"), (dict(series_len=0), "series_len"),
                       (dict(n_density_bins=513), "bin counts"), (dict(n_pair_bins=-1), "bin counts"), (dict(lo=1.0), "lo < hi"),
                       (dict(), "no CPU fallback")):
        with pytest.raises(ValueError, match=match):
            fwo.ForwardWalk(**{**ok, **bad})
    with pytest.raises(ValueError, match="tag slots"):
        fwo.Reference(8, 2, 17, 1, 8, 8, -1.0, 1.0, 4)
    with pytest.raises(ValueError, match="ForwardWalk"):
        fwo.update(torch.zeros(8, 2), None, [0.0], object(), 1)
    with pytest.raises(ValueError, match="2-d"):
        fwo.update(torch.zeros(8), None, [0.0], object(), 1)
    # dmc.run: refused before the model is needed; the lag warning names the decay time
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = 2, 0, None
    with pytest.raises(ValueError, match="forward_walk"):
        dmc.run(m, [0.0], 64, 0.05, 40, 600, 1, forward_walk=object())
    with pytest.warns(RuntimeWarning, match=r"5\.7 a\.u\."):
        fwo.warn_if_short(8, 10, 0.05)                                                   # 4 a.u.
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fwo.warn_if_short(8, 25, 0.05)                                                   # 10 a.u.
    with pytest.raises(ValueError, match="tau"):
        m.dmc_fw_step(object(), object(), 1, [0.0], 0.0)
