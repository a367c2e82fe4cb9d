"""Stochastic reconfiguration, host side (no GPU needed): include/waveflow_sr.h against sr.PROTOTYPES and the built library, the push-through
identity the GPU tests lean on (fp64 numpy, restated here and nowhere in the product), and the refusals that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from waveflow_amd import _lib, sr
from conftest import ROOT


def _header_prototypes():
    """name -> (class of the return type, [class per argument]) for every wf_* function include/waveflow_sr.h declares, in its order."""
    hdr = open(os.path.join(ROOT, "include", "waveflow_sr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    scalar = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "float": "f32", "double": "f64"}

    def c_class(text, is_return=False):
        words = [w for w in text.replace("*", " * ").split() if w != "const"]
        if "*" in words:
            return "string" if is_return and words[0] == "char" else "pointer"
        if is_return and words == ["void"]:
            return "void"
        return scalar[words[0]]   # KeyError: a type this test does not know

    out = {}
    for ret, name, args in re.findall(r"^([\w \*]+?)\b(wf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        assert name not in out, name
        out[name] = (c_class(ret, True), [] if args == ["void"] else [c_class(a.rsplit(None, 1)[0] if "*" not in a else a) for a in args])
    return out


def _ctypes_class(t):
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_void_p: "pointer", ctypes.c_char_p: "string", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "u64",
            ctypes.c_float: "f32", ctypes.c_double: "f64"}[t]


def test_sr_prototype_table_matches_the_header_and_the_library():
    """sr.PROTOTYPES against include/waveflow_sr.h as tests/test_abi_host.py holds _lib.PROTOTYPES against the main header: the same functions in
    the same order, the same number of arguments, per position the same class (double is c_double); every declared symbol is exported, and
    sr.lib() applies the table to the handle _lib.lib() returns.  The main header and its table are not touched by this surface."""
    declared = _header_prototypes()
    assert list(declared) == list(sr.PROTOTYPES) == ["wf_sr_workspace_bytes", "wf_sr_gram", "wf_sr_solve", "wf_sr_apply"]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = sr.lib()
    assert L is _lib.lib()
    for name, (ret, args) in declared.items():
        restype, argtypes = sr.PROTOTYPES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert [_ctypes_class(t) for t in argtypes] == args, (name, args)
        assert _ctypes_class(restype) == ret, (name, ret)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert "f64" in declared["wf_sr_solve"][1] and "f64" in declared["wf_sr_apply"][1]
    assert not set(declared) & set(_lib.PROTOTYPES)
    assert ctypes.sizeof(ctypes.c_double) == 8
    hdr = open(os.path.join(ROOT, "include", "waveflow_sr.h")).read()
    assert '#include "waveflow_hip.h"' in hdr and "WF_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert L.wf_abi_version() == 2


def test_workspace_size_and_argument_refusals_of_the_c_entries():
    """What the entries decide on the host, before any device call."""
    L = sr.lib()
    assert L.wf_sr_workspace_bytes(0, 5) == L.wf_sr_workspace_bytes(5, 0) == -1
    n = L.wf_sr_workspace_bytes(128, 32588)
    assert n > 0 and n % 256 == 0
    assert L.wf_sr_workspace_bytes(4096, 32588) >= 4096 * 4096 * 8 // 2   # one chunk: the lower block tiles of the Gram matrix
    one = ctypes.c_void_p(256)   # never dereferenced: the calls below are refused on their arguments
    assert L.wf_sr_gram(None, 4, 4, 4, one, one, n, None) == -1
    assert L.wf_sr_gram(one, 4, 8, 7, one, one, n, None) == -1                     # ld < P
    assert L.wf_sr_gram(one, 4, 4, 4, one, one, 16, None) == -1                    # workspace too small
    assert L.wf_sr_solve(one, 4, one, -1.0, 0.0, one, one, one, n, None) == -1     # negative damping
    assert L.wf_sr_solve(one, 4, one, float("nan"), 0.0, one, one, one, n, None) == -1
    assert L.wf_sr_solve(one, 4097, one, 0.0, 1e-3, one, one, one, 1 << 40, None) == -2   # B > 4096
    assert L.wf_sr_solve(one, 4, one, 0.0, 1e-3, one, None, one, n, None) == -1    # no info
    assert L.wf_sr_apply(one, 4, 4, 4, None, 1.0, one, one, n, None) == -1
    assert L.wf_sr_apply(one, 0, 4, 4, one, 1.0, one, one, n, None) == -1


# ---- the identity, in fp64 numpy

def _p_space(O, e, lam):
    B = O.shape[0]
    H = np.eye(B) - np.ones((B, B)) / B
    S = O.T @ H @ O / B
    g = 2.0 / B * O.T @ H @ e
    return np.linalg.solve(S + lam * np.eye(O.shape[1]), g)


def _b_space(O, e, lam):
    B = O.shape[0]
    H = np.eye(B) - np.ones((B, B)) / B
    T = H @ (O @ O.T) @ H / B
    y = np.linalg.solve(T + lam * np.eye(B), H @ e)
    return 2.0 / B * O.T @ (H @ y)


@pytest.mark.parametrize("B,P", [(12, 40), (40, 12)])
@pytest.mark.parametrize("lam", [1e-3, 0.7])
def test_b_space_solution_equals_p_space_solution(B, P, lam):
    g = np.random.default_rng(B * 100 + P)
    O = g.normal(size=(B, P))
    e = g.normal(size=B) + 3.0
    dp, db = _p_space(O, e, lam), _b_space(O, e, lam)
    rel = np.linalg.norm(db - dp) / np.linalg.norm(dp)
    print(f"[identity] B {B} P {P} lambda {lam:g}: rel. difference {rel:.2e}")
    assert rel <= 1e-10


# ---- refusals before any launch (they need no GPU: the tensors below live on the host or only say what they are)

def test_validation_raises_value_error_without_a_gpu():
    import torch
    rows = torch.zeros(8, 5)
    e = torch.zeros(8)
    # CPU tensors: there is no CPU fallback
    for call in (lambda: sr.gram(rows), lambda: sr.apply(rows, e.double(), 1.0), lambda: sr.natural_gradient(rows, e),
                 lambda: sr.solve(torch.eye(8, dtype=torch.float64), e.double())):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    # dampings, before the tensors are looked at
    with pytest.raises(ValueError, match=">= 0"):
        sr.natural_gradient(rows, e, damping=-1.0)
    with pytest.raises(ValueError, match=">= 0"):
        sr.natural_gradient(rows, e, relative_damping=-1e-3)
    with pytest.raises(ValueError, match="both zero"):
        sr.natural_gradient(rows, e, damping=0.0, relative_damping=0.0)
    with pytest.raises(ValueError, match="both zero"):
        sr.solve(torch.eye(8, dtype=torch.float64), e.double(), 0.0, 0.0)
    # rows that are not float32 / not contiguous along the parameter axis
    with pytest.raises(ValueError, match="float32"):
        sr.natural_gradient(rows.double(), e)
    with pytest.raises(ValueError, match="contiguous"):
        sr.natural_gradient(torch.zeros(5, 8).t(), e)
    with pytest.raises(ValueError, match="contiguous"):
        sr.gram(torch.zeros(8, 10)[:, ::2])
    with pytest.raises(ValueError, match="2-d"):
        sr.gram(torch.zeros(8))


class _FakeCuda:
    """Says it is a float32 cuda matrix or vector; anything that would touch its data fails the test."""

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.dtype, self.is_cuda, self.device = tuple(shape), dtype, True, torch.device("cuda:0")

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def stride(self, i):
        return ([self.shape[1], 1] if len(self.shape) == 2 else [1])[i]

    def __getattr__(self, name):
        raise AssertionError(f"validation must come before any use of the data ({name})")


def test_shape_checks_come_before_any_launch():
    import torch
    rows = _FakeCuda((8, 5), torch.float32)
    with pytest.raises(ValueError, match="8 entries"):
        sr.natural_gradient(rows, _FakeCuda((7,), torch.float32))                      # e_loc of the wrong length
    with pytest.raises(ValueError, match="at most 4096"):
        sr.natural_gradient(_FakeCuda((4097, 5), torch.float32), _FakeCuda((4097,), torch.float32))
    with pytest.raises(ValueError, match="8 entries"):
        sr.apply(rows, _FakeCuda((9,), torch.float64), 1.0)


def test_vqmc_surface_refuses_sharded_walkers_and_unknown_optimizers():
    from waveflow_amd import vqmc
    with pytest.raises(NotImplementedError):
        vqmc.sr_natural_gradient(None, None, None, None, group=object())
    with pytest.raises(NotImplementedError):
        vqmc.train_step_sr(1, None, None, None, None, 1e-3, group=object())
    t = vqmc.ModelTrainer(num_epochs=1)
    assert t.optimizer == 'adam'
    t.optimizer = 'lbfgs'
    with pytest.raises(ValueError, match="optimizer"):
        t.start_training()
    t.optimizer = 'sr'
    with pytest.raises(NotImplementedError):
        t.start_training(group=object())
