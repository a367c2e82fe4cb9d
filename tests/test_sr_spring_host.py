"""The SPRING optimiser, host side (no GPU needed): include/waveflow_sr_spring.h against sr.SPRING_PROTOTYPES, sr.SpringTrainState and the built
library; the B x B form against the P x P solve in fp64; what the entries and the Python surface refuse before any launch; the trainer's
new optimizer value and attributes."""
import ctypes
import os
import re

import numpy as np
import pytest

from waveflow_amd import _lib, core, sr, vqmc
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_sr_spring.h")
NAMES = ["wf_sr_matvec", "wf_sr_apply_add", "wf_spring_rhs", "wf_vqmc_spring_step_workspace_bytes", "wf_vqmc_spring_step"]


def test_spring_prototype_table_matches_the_header_and_the_library():
    """sr.SPRING_PROTOTYPES against the header: the same functions in the same order, per position the same argument class; every symbol
    exported; sr.lib() applies the table; the existing tables keep their sizes and the ABI version stays 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(sr.SPRING_PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = sr.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        assert hasattr(raw, name), name
        restype, argtypes = sr.SPRING_PROTOTYPES[name]
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert declared["wf_vqmc_spring_step"][1].count("f64") == 5 and declared["wf_vqmc_spring_step"][1][2] == "u64"
    assert sr.SPRING_PROTOTYPES["wf_vqmc_spring_step"][1][1] is ctypes.POINTER(sr.SpringTrainState)
    assert not set(declared) & (set(_lib.PROTOTYPES) | set(sr.PROTOTYPES) | set(sr.STEP_PROTOTYPES))
    assert len(_lib.PROTOTYPES) == 55 and len(sr.PROTOTYPES) == 4 and len(sr.STEP_PROTOTYPES) == 2
    hdr = open(HEADER).read()
    assert '#include "waveflow_sr_step.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    assert L.wf_abi_version() == 2


def test_spring_state_struct_matches_the_header():
    """wf_spring_train_state: the fields of wf_sr_train_state in their order and at their offsets, then phi_dev and eff_ring_dev."""
    body = re.search(r"typedef\s+struct\s+wf_spring_train_state\s*\{(.*?)\}\s*wf_spring_train_state\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, name = decl.replace("*", " * ").rsplit(None, 1)
            fields.append((name, c_class(kind)))
    old = [(n, ctypes_class(t)) for n, t in sr.SrTrainState._fields_]
    assert fields == old + [("phi_dev", "pointer"), ("eff_ring_dev", "pointer")]
    assert [(n, ctypes_class(t)) for n, t in sr.SpringTrainState._fields_] == fields
    assert [getattr(sr.SpringTrainState, n).offset for n, _ in old] == [getattr(sr.SrTrainState, n).offset for n, _ in old]
    assert sr.SpringTrainState.phi_dev.offset == 56 and sr.SpringTrainState.eff_ring_dev.offset == 64 and ctypes.sizeof(sr.SpringTrainState) == 72


def test_b_space_form_is_the_p_space_minimiser_in_fp64():
    """(S + lambda I) d = g + lambda mu phi against q = O phi, (Tbar + lambda I) y = H (e - (mu / 2) q), d = mu phi + (2 / B) O^T H y."""
    rng = np.random.default_rng(11)
    B, P, mu = 37, 211, 0.9
    O, e, phi = rng.standard_normal((B, P)), rng.standard_normal(B), rng.standard_normal(P)
    H = np.eye(B) - 1.0 / B
    T = H @ O @ O.T @ H / B
    lam = 1e-3 * np.trace(T) / B
    want = np.linalg.solve(O.T @ H @ O / B + lam * np.eye(P), 2.0 / B * O.T @ H @ e + lam * mu * phi)
    y = np.linalg.solve(T + lam * np.eye(B), H @ (e - 0.5 * mu * (O @ phi)))
    got = mu * phi + 2.0 / B * O.T @ (H @ y)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    y0 = np.linalg.solve(T + lam * np.eye(B), H @ e)
    assert np.array_equal(0.0 * phi + 2.0 / B * O.T @ (H @ y0), 2.0 / B * O.T @ (H @ y0))   # mu = 0: today's d


def test_clip_is_median_and_mean_absolute_deviation():
    import torch
    e = torch.tensor([3.0, -1.0, 1e5, 2.0, 0.0, -1e5], dtype=torch.float32)
    assert torch.equal(sr.clip_local_energies(e, 0.0), e.double())
    c = 0.5 * (0.0 + 2.0)
    w = float(np.mean(np.abs(e.double().numpy() - c)))
    out = sr.clip_local_energies(e, 1.0).numpy()
    assert np.array_equal(out, np.clip(e.double().numpy(), c - w, c + w)) and out.max() == c + w and out.min() == c - w
    # values that are not finite sort last: 1 2 5 | nan -inf, and 0 1 2 5 | nan -inf
    nan, inf = float("nan"), float("inf")
    c, w = sr._median_and_deviation(torch.tensor([5.0, nan, 1.0, 2.0, -inf], dtype=torch.float32))
    assert float(c) == 5.0 and c.dtype == torch.float64 and bool(torch.isnan(w))
    c, w = sr._median_and_deviation(torch.tensor([5.0, 1.0, 2.0, -inf, 0.0, inf], dtype=torch.float32))
    assert float(c) == 3.5 and float(w) == inf
    got = sr.clip_local_energies(torch.tensor([5.0, 1.0, 2.0, -inf, 0.0, inf], dtype=torch.float32), 1.0)   # w = inf: nothing finite is cut
    assert got.tolist() == [5.0, 1.0, 2.0, -inf, 0.0, inf]
    assert bool(torch.isnan(sr.clip_local_energies(torch.tensor([5.0, nan, 1.0], dtype=torch.float32), 1.0)).all())   # a NaN energy spoils w


def test_c_entries_refuse_bad_arguments_on_the_host():
    L = sr.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    assert L.wf_sr_matvec(None, 4, 4, 4, one, one, None) == -1
    assert L.wf_sr_matvec(one, 0, 4, 4, one, one, None) == -1
    assert L.wf_sr_matvec(one, 4, 4, 3, one, one, None) == -1
    assert L.wf_sr_matvec(one, 4, 4, 4, None, one, None) == -1
    assert L.wf_sr_matvec(one, 65537, 4, 4, one, one, None) == -2
    for mu in (1.0, -0.1, float("nan")):
        assert L.wf_sr_apply_add(one, 4, 4, 4, one, 1.0, one, mu, one, one, 1 << 30, None) == -1, mu
    assert L.wf_sr_apply_add(one, 4, 4, 4, one, 1.0, None, 0.5, None, one, 1 << 30, None) == -1
    assert L.wf_sr_apply_add(one, 4, 4, 4, one, 1.0, None, 0.5, one, one, 8, None) == -1          # workspace too small
    assert L.wf_spring_rhs(one, one, 0, None, 0.0, 0.0, one, one, one, None, None) == -1
    assert L.wf_spring_rhs(one, one, 8, None, 0.5, 0.0, one, one, one, None, None) == -1      # momentum without q
    assert L.wf_spring_rhs(one, one, 8, one, 1.0, 0.0, one, one, one, None, None) == -1
    assert L.wf_spring_rhs(one, one, 8, one, 0.5, -1.0, one, one, one, None, None) == -1
    assert L.wf_spring_rhs(one, one, 4097, one, 0.5, 1.0, one, one, one, None, None) == -2
    assert L.wf_vqmc_spring_step_workspace_bytes(None, 128) == -1
    assert L.wf_vqmc_spring_step_workspace_bytes(one, 0) == -1

    def state():
        return sr.SpringTrainState(256, 256, 256, 256, None, 256, 128, 0, 256, None)

    def call(st, batch=8, damping=(0.0, 1e-3), spring=(0.9, 1e-3, 5.0), draw=1, n_protons=0):
        return L.wf_vqmc_spring_step(one, ctypes.byref(st), 1, batch, None, n_protons, damping[0], damping[1], spring[0], spring[1], spring[2], 0, None, draw,
                                     one, 1 << 30, None)
    assert L.wf_vqmc_spring_step(None, ctypes.byref(state()), 1, 8, None, 0, 0.0, 1e-3, 0.9, 1e-3, 5.0, 0, None, 1, one, 1 << 30, None) == -1
    assert call(state(), batch=0) == -1 and call(state(), n_protons=9) == -1
    for bad in ((0.0, 0.0), (-1.0, 1e-3), (1e-3, -1.0), (float("nan"), 1e-3)):
        assert call(state(), damping=bad) == -1, bad
    for bad in ((1.0, 1e-3, 5.0), (-0.5, 1e-3, 5.0), (float("nan"), 0.0, 0.0), (0.9, -1e-3, 5.0), (0.9, 1e-3, -5.0), (0.9, float("nan"), 0.0)):
        assert call(state(), spring=bad) == -1, bad
    assert call(state(), draw=0) == -1    # draw = 0 without walkers
    for missing in ("params_dev", "counter_dev", "step_size_dev", "loss_ring_dev", "status_dev", "phi_dev"):
        st = state()
        setattr(st, missing, None)
        assert call(st) == -1, missing


def _bare_model(D=2):
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = D, 0, None
    return m


def test_python_surface_refuses_before_any_launch():
    import torch
    m = _bare_model()
    st = {}   # never looked at
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        m.spring_step(st, 1, 8, [0.0], momentum=1.0)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        m.spring_step(st, 1, 8, [0.0], momentum=-0.1)
    with pytest.raises(ValueError, match="norm constraint"):
        m.spring_step(st, 1, 8, [0.0], norm_constraint=-1e-3)
    with pytest.raises(ValueError, match="clip"):
        m.spring_step(st, 1, 8, [0.0], clip=-1.0)
    with pytest.raises(ValueError, match="both zero"):
        m.spring_step(st, 1, 8, [0.0], damping=0.0, relative_damping=0.0)
    with pytest.raises(ValueError, match="4096"):
        m.spring_step(st, 1, 4097, [0.0])
    with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
        m.spring_step(st, 1, 8, [0.0], walkers=torch.zeros(8, 3))
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.spring_step(st, 1, 8, [0.0], walkers=torch.zeros(8, 2))
    rows, e, prev = torch.zeros(8, 5), torch.zeros(8), torch.zeros(5)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        sr.spring_direction(rows, e, prev, 1.0)
    with pytest.raises(ValueError, match="clip"):
        sr.spring_direction(rows, e, prev, 0.5, clip=-1.0)
    with pytest.raises(ValueError, match=">= 0"):
        sr.spring_direction(rows, e, prev, 0.5, damping=-1.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sr.spring_direction(rows, e, prev, 0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sr.matvec(rows, prev)
    with pytest.raises(ValueError, match="float32"):
        sr.matvec(rows.double(), prev)
    with pytest.raises(ValueError, match="at most 4096"):
        sr.spring_direction(torch.zeros(4097, 2), torch.zeros(4097), torch.zeros(2), 0.5)
    with pytest.raises(ValueError, match="2-d"):
        sr.matvec(torch.zeros(8), prev)
    with pytest.raises(NotImplementedError):
        vqmc.spring_direction(None, None, None, None, prev, 0.5, group=object())
    with pytest.raises(NotImplementedError):
        vqmc.train_step_spring(1, None, None, None, None, 1e-2, prev, 0.5, 1e-3, 5.0, group=object())
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        vqmc.train_step_spring(1, None, None, None, None, 1e-2, prev, 1.0, 1e-3, 5.0)


def test_step_size_rule():
    import torch
    d = torch.tensor([3.0, 4.0])
    assert vqmc.spring_step_size(0.02, d, 0.0) == float(np.float32(0.02))
    assert vqmc.spring_step_size(0.02, d * 0, 1e-3) == float(np.float32(0.02))
    assert vqmc.spring_step_size(0.02, d, 1e-3) == float(np.float32(np.sqrt(1e-3 / 25.0)))
    assert vqmc.spring_step_size(0.001, d, 1e-3) == float(np.float32(0.001))


def test_trainer_accepts_spring_and_still_refuses_what_it_does_not_know(monkeypatch, tmp_path):
    t = vqmc.ModelTrainer(num_epochs=1)
    assert t.optimizer == 'adam' and (t.spring_momentum, t.spring_norm_constraint, t.spring_clip) == tuple(vqmc.SPRING_DEFAULTS[k] for k in (
        "momentum", "norm_constraint", "clip"))
    t.optimizer = 'spring'
    for on_device in (False, True):
        t.sr_on_device = on_device
        with pytest.raises(NotImplementedError):
            t.start_training(group=object())
    t.optimizer = 'lbfgs'
    with pytest.raises(ValueError, match="optimizer"):
        t.start_training()
    entered = []

    class Opt:
        x = None

    monkeypatch.setattr(vqmc, "create_train_state", lambda *a, **k: (None, None, None, Opt(), None, lambda s: None))
    monkeypatch.setattr(vqmc.physics, "construct_hamiltonian_function", lambda *a, **k: None)
    monkeypatch.setattr(vqmc.ModelTrainer, "_train_spring", lambda self, *a: entered.append("eager"))
    monkeypatch.setattr(vqmc.ModelTrainer, "_train_spring_device", lambda self, *a: entered.append("device"))
    monkeypatch.setattr(vqmc.ModelTrainer, "_train_sr", lambda self, *a: entered.append("sr"))
    t = vqmc.ModelTrainer(num_epochs=1)
    t.save_dir = str(tmp_path / "run")
    t.optimizer = 'spring'
    del t.sr_on_device, t.spring_momentum, t.spring_norm_constraint, t.spring_clip   # an object from before the attributes existed
    t.start_training(verbose=False)
    assert t._spring_settings() == tuple(vqmc.SPRING_DEFAULTS[k] for k in ("momentum", "norm_constraint", "clip")) == (0.9, 0.1, 5.0)
    assert t._spring_damping() == {"relative_damping": 1e-2}
    t.sr_damping = {"damping": 1e-4}
    assert t._spring_damping() == {"damping": 1e-4}
    t.sr_on_device = True
    t.start_training(verbose=False)
    t.optimizer = 'sr'
    t.sr_on_device = False
    t.start_training(verbose=False)
    assert entered == ["eager", "device", "sr"]
