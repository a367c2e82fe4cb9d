"""Observables on the device, host side (no GPU needed): include/waveflow_observe.h against observables.PROTOTYPES, observables.ObserveAcc and
the built library; what the entries and the Python surface refuse before any launch; the host-side Totals."""
import ctypes
import multiprocessing as mp
import os
import re
import socket
import sys

import numpy as np
import pytest

from waveflow_amd import _lib, core, observables as obs, sr
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_observe.h")
NAMES = ["wf_observe_workspace_bytes", "wf_observe_accumulate", "wf_vqmc_observe_step_workspace_bytes", "wf_vqmc_observe_step"]


def test_prototype_table_matches_the_header_and_the_library():
    """observables.PROTOTYPES against include/waveflow_observe.h: the same functions in the same order, per position the same argument class;
    every symbol exported; observables.lib() applies the table; nothing of it is in the existing tables, which keep their sizes; ABI version 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(obs.PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = obs.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = obs.PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert declared["wf_vqmc_observe_step"][1][3] == "u64" and declared["wf_observe_accumulate"][1][4] == "i64"
    assert obs.PROTOTYPES["wf_observe_accumulate"][1][8] is ctypes.POINTER(obs.ObserveAcc)
    assert obs.PROTOTYPES["wf_vqmc_observe_step"][1][1] is ctypes.POINTER(obs.ObserveAcc)
    for table in (_lib.PROTOTYPES, sr.PROTOTYPES, sr.STEP_PROTOTYPES, sr.SPRING_PROTOTYPES):
        assert not set(declared) & set(table)
    assert len(_lib.PROTOTYPES) == 55 and len(sr.PROTOTYPES) == 4 and len(sr.STEP_PROTOTYPES) == 2 and len(sr.SPRING_PROTOTYPES) == 5
    hdr = open(HEADER).read()
    assert '#include "waveflow_hip.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    assert re.search(r"#define\s+WF_OBSERVE_SCALARS\s+5\b", hdr) and len(obs.SCALARS) == 5
    assert obs.SCALARS == ("e_loc", "t_lap", "t_grad", "v_en", "v_ee")
    assert L.wf_abi_version() == 2


def test_accumulator_struct_matches_the_header():
    """wf_observe_acc field by field: four pointers, two int32, two floats -- names, order, kinds, offsets and size of observables.ObserveAcc."""
    body = re.search(r"typedef\s+struct\s+wf_observe_acc\s*\{(.*?)\}\s*wf_observe_acc\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = [n.strip() for n in decl.split(",")]    # "float lo, hi": one kind, several names
            kind, name = first.replace("*", " * ").rsplit(None, 1)
            fields += [(n, c_class(kind)) for n in [name] + more]
    assert fields == [("sums_dev", "pointer"), ("counts_dev", "pointer"), ("density_dev", "pointer"), ("pair_dev", "pointer"),
                      ("n_density_bins", "i32"), ("n_pair_bins", "i32"), ("lo", "f32"), ("hi", "f32")]
    assert [(n, ctypes_class(t)) for n, t in obs.ObserveAcc._fields_] == fields
    assert [getattr(obs.ObserveAcc, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert ctypes.sizeof(obs.ObserveAcc) == 48


def _acc(**kw):
    a = dict(sums_dev=256, counts_dev=256, density_dev=256, pair_dev=256, n_density_bins=8, n_pair_bins=8, lo=-1.0, hi=1.0)
    a.update(kw)
    return obs.ObserveAcc(**a)


def test_c_entries_refuse_bad_arguments_on_the_host():
    """What the four entries decide before they look at a model or touch a device."""
    L = obs.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    big = 1 << 30
    assert L.wf_observe_workspace_bytes(-1) == -1 and L.wf_observe_workspace_bytes(0) == 0
    # the block partials: 14 words of 8 bytes per block, 256 walkers per block, at most 1024 blocks
    assert L.wf_observe_workspace_bytes(1) == 256 and L.wf_observe_workspace_bytes(257) == 256 and L.wf_observe_workspace_bytes(768) == 512
    assert L.wf_observe_workspace_bytes(1 << 18) == L.wf_observe_workspace_bytes(1 << 30) == L.wf_observe_workspace_bytes(1 << 36) == 1024 * 14 * 8
    assert L.wf_observe_workspace_bytes((1 << 36) + 1) == -2           # one call: at most 2^36 walkers (32-bit histogram counters per workgroup)

    def accumulate(acc, B=8, D=2, n_pr=0, pr=None, x=one, psi=one, grad=one, hdiag=one, values=None, ws=one, ws_bytes=big):
        return L.wf_observe_accumulate(x, psi, grad, hdiag, B, D, pr, n_pr, ctypes.byref(acc) if acc is not None else None, values, ws, ws_bytes, None)
    good = _acc()
    assert accumulate(good, B=0) == 0                                   # an empty batch: nothing is touched
    assert accumulate(None, B=0) == 0
    assert accumulate(good, B=-1) == -1
    assert accumulate(good, B=(1 << 36) + 1) == -2
    assert accumulate(good, n_pr=9, pr=one) == -1                       # nine protons
    assert accumulate(good, n_pr=2) == -1                               # protons without positions
    for D in (0, 1, 9):
        assert accumulate(good, D=D) == -1, D
    assert accumulate(None) == -1                                       # neither an accumulator nor values
    for missing in ("x", "psi", "grad", "hdiag"):
        assert accumulate(good, **{missing: None}) == -1, missing
    for missing in ("sums_dev", "counts_dev", "density_dev", "pair_dev"):
        assert accumulate(_acc(**{missing: None})) == -1, missing
    assert accumulate(_acc(n_density_bins=-1)) == -1 and accumulate(_acc(n_pair_bins=-1)) == -1
    assert accumulate(_acc(n_density_bins=513)) == -2 and accumulate(_acc(n_pair_bins=1025)) == -2
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (0.0, float("nan"))):
        assert accumulate(_acc(lo=lo, hi=hi)) == -1, (lo, hi)
    assert accumulate(good, ws=None) == -1
    assert accumulate(good, B=257, ws_bytes=255) == -1                  # one byte short of wf_observe_workspace_bytes(257)
    # (no accepted form is tried with these pointers: it would get as far as a launch)

    assert L.wf_vqmc_observe_step_workspace_bytes(None, 128) == -1
    assert L.wf_vqmc_observe_step_workspace_bytes(one, 0) == -1
    assert L.wf_vqmc_observe_step_workspace_bytes(one, -5) == -1

    def step(m=one, acc=good, counter=one, batch=8, pr=None, n_pr=0, x=None, draw=1, values=None):
        return L.wf_vqmc_observe_step(m, ctypes.byref(acc) if acc is not None else None, counter, 1, batch, pr, n_pr, 0, x, draw, values, one, big, None)
    assert step(m=None) == -1
    assert step(batch=0) == -1
    assert step(counter=None) == -1
    assert step(n_pr=9, pr=one) == -1
    assert step(acc=None) == -1                                         # neither an accumulator nor values
    assert step(draw=0) == -1                                           # draw = 0 without walkers
    assert step(acc=_acc(lo=1.0, hi=-1.0)) == -1
    assert step(acc=_acc(sums_dev=None)) == -1
    assert step(acc=_acc(n_pair_bins=1025)) == -2


def _bare_model(D=2):
    """A DeviceModel that owns nothing (no GPU here): observe_step must refuse its arguments before it needs more than the walker width."""
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = D, 0, None
    return m


def test_python_surface_refuses_before_any_launch():
    import torch
    m = _bare_model()
    acc, counter = object(), object()   # never looked at
    with pytest.raises(ValueError, match="at least 1"):
        m.observe_step(acc, counter, 1, 0, [0.0])
    for bad in (torch.zeros(8, 3), torch.zeros(7, 2), torch.zeros(16)):
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.observe_step(acc, counter, 1, 8, [0.0], walkers=bad)
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.observe_step(acc, counter, 1, 8, [0.0], out_walkers=bad)
        with pytest.raises(ValueError, match=r"shape \[8, 5\]"):
            m.observe_step(acc, counter, 1, 8, [0.0], values=bad)
    with pytest.raises(ValueError, match="float32"):
        m.observe_step(acc, counter, 1, 8, [0.0], walkers=torch.zeros(8, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        m.observe_step(acc, counter, 1, 8, [0.0], walkers=torch.zeros(2, 8).t())          # not contiguous
    with pytest.raises(ValueError, match="float32"):
        m.observe_step(acc, counter, 1, 8, [0.0], values=torch.zeros(8, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.observe_step(acc, counter, 1, 8, [0.0], walkers=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.observe_step(acc, counter, 1, 8, [0.0], values=torch.zeros(8, 5))
    with pytest.raises(ValueError, match="exclude"):
        m.observe_step(acc, counter, 1, 8, [0.0], walkers=torch.zeros(8, 2), out_walkers=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="nothing to do"):
        m.observe_step(None, counter, 1, 8, [0.0])
    # the model-free binding and the accumulator: the same style
    x = torch.zeros(8, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        obs.accumulate(x, torch.zeros(8), x, x, [0.0], return_values=True)
    with pytest.raises(ValueError, match="2 .. 8"):
        obs.accumulate(torch.zeros(8, 9), torch.zeros(8), x, x, [0.0], return_values=True)
    with pytest.raises(ValueError, match="no CPU fallback"):
        obs.Accumulator(2, lo=-1.0, hi=1.0, device="cpu")
    with pytest.raises(ValueError, match="bin counts"):
        obs.Accumulator(2, n_density_bins=513, lo=-1.0, hi=1.0, device="cpu")
    with pytest.raises(ValueError, match="lo < hi"):
        obs.Accumulator(2, lo=1.0, hi=1.0, device="cpu")


def _totals(seed, D=3, nd=7, npair=5, lo=-2.0, hi=1.5):
    g = np.random.default_rng(seed)
    return obs.Totals(D, nd, npair, lo, hi, sums=g.normal(size=(5, 2)) * 1e3, counts=g.integers(0, 1 << 40, size=4),
                      density=g.integers(0, 1 << 40, size=(D, nd)), pair=g.integers(0, 1 << 40, size=npair))


def test_totals_merge_adds_and_refuses_another_geometry():
    a, b = _totals(1), _totals(2)
    want = {k: getattr(a, k) + getattr(b, k) for k in ("sums", "counts", "density", "pair")}
    assert a.merge(b) is a
    for k, v in want.items():
        assert np.array_equal(getattr(a, k), v) and getattr(a, k).dtype == v.dtype, k
    assert a.counts.dtype == np.int64 and a.sums.dtype == np.float64
    for other in (_totals(2, D=2), _totals(2, nd=8), _totals(2, npair=4), _totals(2, lo=-2.5), _totals(2, hi=2.0)):
        with pytest.raises(ValueError, match="geometry"):
            a.merge(other)
    z = obs.Totals.from_arrays(a.arrays())
    assert z.geometry() == a.geometry() and all(np.array_equal(getattr(z, k), getattr(a, k)) for k in want)
    with pytest.raises(ValueError, match="shape"):
        obs.Totals(3, 7, 5, -1.0, 1.0, density=np.zeros((3, 6)))


def test_result_on_hand_made_totals():
    """Five walkers with hand-made values: means, the variance with n - 1, the standard error; densities that integrate to D and D (D - 1) / 2
    when nothing is outside, and to less by the outside share when something is."""
    D, nd, npair, lo, hi = 3, 4, 8, -2.0, 2.0
    v = np.array([[1.0, 2.0, 4.0, 8.0, 16.0], [0.5, -1.0, 3.0, 3.0, 3.0], [2.0, 2.5, 2.0, 2.5, 2.0], [-1.0, -2.0, -3.0, -4.0, -5.0],
                  [0.0, 0.0, 0.0, 0.0, 1.0]])            # [scalar][walker]
    n = v.shape[1]
    density = np.array([[5, 0, 0, 0], [1, 2, 2, 0], [0, 0, 1, 4]])
    pair = np.array([3, 4, 0, 2, 1, 5, 0, 0])
    t = obs.Totals(D, nd, npair, lo, hi, sums=np.stack([v.sum(1), (v * v).sum(1)], axis=1), counts=[n, 2, 0, 0], density=density, pair=pair)
    r = t.result()
    assert r["n"] == n and r["n_skipped"] == 2 and r["outside_density"] == 0 and r["outside_pair"] == 0
    for k, name in enumerate(obs.SCALARS):
        assert abs(r[name] - v[k].mean()) <= 1e-15 * max(1.0, abs(v[k].mean())), name
        assert abs(r[name + "_variance"] - v[k].var(ddof=1)) <= 1e-13 * max(1.0, v[k].var(ddof=1)), name
        assert abs(r[name + "_stderr"] - np.sqrt(v[k].var(ddof=1) / n)) <= 1e-13, name
    wd, wp = (hi - lo) / nd, (hi - lo) / npair
    assert np.array_equal(r["density_x"], lo + (np.arange(nd) + 0.5) * wd) and np.array_equal(r["pair_r"], (np.arange(npair) + 0.5) * wp)
    assert r["density"].shape == (nd,) and r["density_by_column"].shape == (D, nd) and r["pair"].shape == (npair,)
    assert abs(r["density"].sum() * wd - D) <= 1e-14 and abs(r["pair"].sum() * wp - D * (D - 1) / 2) <= 1e-14
    assert np.allclose(r["density_by_column"].sum(1) * wd, 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(r["density"], density.sum(0) / (n * wd))
    # one coordinate and two pairs outside: the integrals fall short by exactly that share
    density[2, 3] -= 1
    pair[5] -= 2
    r = obs.Totals(D, nd, npair, lo, hi, sums=t.sums, counts=[n, 2, 1, 2], density=density, pair=pair).result()
    assert r["outside_density"] == 1 and r["outside_pair"] == 2
    assert abs(r["density"].sum() * wd - (D - 1 / n)) <= 1e-14 and abs(r["pair"].sum() * wp - (D * (D - 1) / 2 - 2 / n)) <= 1e-14
    # no histograms, no walkers
    r = obs.Totals(2, 0, 0, -1.0, 1.0).result()
    assert r["n"] == 0 and "density" not in r and "pair" not in r and np.isnan(r["e_loc"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = _totals(10 + rank).all_reduce()
        q.put((rank, t.arrays()))
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_two_gloo_ranks_equals_merge():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = _totals(10).merge(_totals(11))
    for rank, arrays in res:
        got = obs.Totals.from_arrays(arrays)
        assert got.geometry() == want.geometry()
        for k in ("sums", "counts", "density", "pair"):
            assert np.array_equal(getattr(got, k), getattr(want, k)) and getattr(got, k).dtype == getattr(want, k).dtype, (rank, k)
