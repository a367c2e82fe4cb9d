"""Stochastic reconfiguration as a whole step on the device, host side (no GPU needed): include/waveflow_sr_step.h against sr.STEP_PROTOTYPES,
sr.SrTrainState and the built library; what the entries and the Python surface refuse before any launch; the trainer's new attribute."""
import ctypes
import os
import re

import pytest

from waveflow_amd import _lib, core, sr, vqmc
from abi_header import c_class, ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_sr_step.h")


def test_step_prototype_table_matches_the_header_and_the_library():
    """sr.STEP_PROTOTYPES against include/waveflow_sr_step.h: the same functions in the same order, per position the same argument class; every
    symbol exported; sr.lib() applies the table; nothing of it is in the two existing tables, which keep their sizes; the ABI version stays 2."""
    declared = header_prototypes(HEADER)
    assert list(declared) == list(sr.STEP_PROTOTYPES) == ["wf_vqmc_sr_step_workspace_bytes", "wf_vqmc_sr_step"]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = sr.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = sr.STEP_PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert declared["wf_vqmc_sr_step"][1].count("f64") == 2 and declared["wf_vqmc_sr_step"][1][2] == "u64"
    assert sr.STEP_PROTOTYPES["wf_vqmc_sr_step"][1][1] is ctypes.POINTER(sr.SrTrainState)
    assert not set(declared) & set(_lib.PROTOTYPES) and not set(declared) & set(sr.PROTOTYPES)
    assert len(_lib.PROTOTYPES) == 55 and len(sr.PROTOTYPES) == 4
    hdr = open(HEADER).read()
    assert '#include "waveflow_sr.h"' in hdr and "WF_ABI_VERSION" not in no_comments(HEADER)
    assert L.wf_abi_version() == 2


def test_state_struct_matches_the_header():
    """wf_sr_train_state field by field: six pointers, then two int32 -- names, order, kinds and offsets of sr.SrTrainState."""
    body = re.search(r"typedef\s+struct\s+wf_sr_train_state\s*\{(.*?)\}\s*wf_sr_train_state\s*;", no_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, name = decl.replace("*", " * ").rsplit(None, 1)
            fields.append((name, c_class(kind)))
    assert fields == [("params_dev", "pointer"), ("counter_dev", "pointer"), ("step_size_dev", "pointer"), ("loss_ring_dev", "pointer"),
                      ("norm_ring_dev", "pointer"), ("status_dev", "pointer"), ("ring_len", "i32"), ("defer_eval_tables", "i32")]
    assert [(n, ctypes_class(t)) for n, t in sr.SrTrainState._fields_] == fields
    assert ctypes.sizeof(sr.SrTrainState) == 6 * 8 + 8
    assert [getattr(sr.SrTrainState, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_c_entries_refuse_bad_arguments_on_the_host():
    """What the two entries decide before they look at the model or touch a device."""
    L = sr.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on the arguments in front of it
    assert L.wf_vqmc_sr_step_workspace_bytes(None, 128) == -1
    assert L.wf_vqmc_sr_step_workspace_bytes(one, 0) == -1
    assert L.wf_vqmc_sr_step_workspace_bytes(one, -5) == -1
    st = sr.SrTrainState(256, 256, 256, 256, None, 256, 128, 0)
    assert L.wf_vqmc_sr_step(None, ctypes.byref(st), 1, 8, None, 0, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1
    assert L.wf_vqmc_sr_step(one, None, 1, 8, None, 0, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1
    assert L.wf_vqmc_sr_step(one, ctypes.byref(st), 1, 0, None, 0, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1
    assert L.wf_vqmc_sr_step(one, ctypes.byref(st), 1, 8, None, 9, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1    # nine protons
    for bad in ((0.0, 0.0), (-1.0, 1e-3), (1e-3, -1.0), (float("nan"), 1e-3)):
        assert L.wf_vqmc_sr_step(one, ctypes.byref(st), 1, 8, None, 0, bad[0], bad[1], 0, None, 1, one, 1 << 30, None) == -1, bad
    assert L.wf_vqmc_sr_step(one, ctypes.byref(st), 1, 8, None, 0, 0.0, 1e-3, 0, None, 0, one, 1 << 30, None) == -1    # draw = 0 without walkers
    for missing in ("params_dev", "counter_dev", "step_size_dev", "loss_ring_dev", "status_dev"):
        st2 = sr.SrTrainState(256, 256, 256, 256, None, 256, 128, 0)
        setattr(st2, missing, None)
        assert L.wf_vqmc_sr_step(one, ctypes.byref(st2), 1, 8, None, 0, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1, missing
    st.ring_len = 0
    assert L.wf_vqmc_sr_step(one, ctypes.byref(st), 1, 8, None, 0, 0.0, 1e-3, 0, None, 1, one, 1 << 30, None) == -1


def _bare_model(D=2):
    """A DeviceModel that owns nothing (no GPU here): sr_step must refuse its arguments before it needs more than the walker width."""
    m = object.__new__(core.DeviceModel)
    m.D, m.device, m._h = D, 0, None
    return m


def test_python_surface_refuses_before_any_launch():
    import torch
    m = _bare_model()
    st = {}   # never looked at
    with pytest.raises(ValueError, match=">= 0"):
        m.sr_step(st, 1, 8, [0.0], damping=-1.0)
    with pytest.raises(ValueError, match=">= 0"):
        m.sr_step(st, 1, 8, [0.0], relative_damping=-1e-3)
    with pytest.raises(ValueError, match="both zero"):
        m.sr_step(st, 1, 8, [0.0], damping=0.0, relative_damping=0.0)
    with pytest.raises(ValueError, match="4096"):
        m.sr_step(st, 1, 4097, [0.0])
    with pytest.raises(ValueError, match="4096"):
        m.sr_step(st, 1, 0, [0.0])
    for bad in (torch.zeros(8, 3), torch.zeros(7, 2), torch.zeros(16)):
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.sr_step(st, 1, 8, [0.0], walkers=bad)
        with pytest.raises(ValueError, match=r"shape \[8, 2\]"):
            m.sr_step(st, 1, 8, [0.0], out_walkers=bad)
    with pytest.raises(ValueError, match="float32"):
        m.sr_step(st, 1, 8, [0.0], walkers=torch.zeros(8, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        m.sr_step(st, 1, 8, [0.0], walkers=torch.zeros(2, 8).t())          # not contiguous
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.sr_step(st, 1, 8, [0.0], walkers=torch.zeros(8, 2))
    with pytest.raises(ValueError, match="exclude"):
        m.sr_step(st, 1, 8, [0.0], walkers=torch.zeros(8, 2), out_walkers=torch.zeros(8, 2))


def test_trainer_attribute_defaults_off_and_sharded_walkers_are_refused_on_both_paths():
    t = vqmc.ModelTrainer(num_epochs=1)
    assert t.sr_on_device is False and t.optimizer == 'adam'
    t.optimizer = 'sr'
    for on_device in (False, True):
        t.sr_on_device = on_device
        with pytest.raises(NotImplementedError):
            t.start_training(group=object())
    t.optimizer = 'lbfgs'
    with pytest.raises(ValueError, match="optimizer"):
        t.start_training()


def test_trainer_without_the_attribute_takes_the_eager_path(monkeypatch, tmp_path):
    """A trainer whose sr_on_device was deleted (an object from before the attribute existed) behaves as one that never had it: optimizer='sr'
    goes through _train_sr, never through the device loop; with the attribute set it is the other way round.  Model factory and both loops are
    stand-ins: which loop start_training enters is decided on the host."""
    entered = []

    class Opt:
        x = None

    monkeypatch.setattr(vqmc, "create_train_state", lambda *a, **k: (None, None, None, Opt(), None, lambda s: None))
    monkeypatch.setattr(vqmc.physics, "construct_hamiltonian_function", lambda *a, **k: None)
    monkeypatch.setattr(vqmc.ModelTrainer, "_train_sr", lambda self, *a: entered.append("eager"))
    monkeypatch.setattr(vqmc.ModelTrainer, "_train_sr_device", lambda self, *a: entered.append("device"))
    t = vqmc.ModelTrainer(num_epochs=1)
    t.save_dir = str(tmp_path / "run")
    t.optimizer = 'sr'
    del t.sr_on_device
    t.start_training(verbose=False)
    t.sr_on_device = False
    t.start_training(verbose=False)
    t.sr_on_device = True
    t.start_training(verbose=False)
    assert entered == ["eager", "eager", "device"]
