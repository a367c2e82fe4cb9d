"""The matrix-free solve of stochastic reconfiguration, host side (no GPU needed): sr.cg_reference against the dense solve in fp64, the trace
identity its shift rests on, include/waveflow_sr_cg.h against sr.CG_PROTOTYPES and the built library, what the entries and the Python surface
refuse before any launch, and that the default solver='cholesky' still makes the calls it made before."""
import ctypes
import os

import numpy as np
import pytest

from waveflow_amd import _lib, sr, vqmc
from abi_header import ctypes_class, header_prototypes, no_comments
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "waveflow_sr_cg.h")
NAMES = ["wf_sr_cg_workspace_bytes", "wf_sr_cg_solve"]


def _dense(O, lam):
    B = O.shape[0]
    H = np.eye(B) - 1.0 / B
    return H @ O @ O.T @ H / B + lam * np.eye(B)


@pytest.mark.parametrize("precondition", [True, False])
@pytest.mark.parametrize("P", [1, 5, 257])
@pytest.mark.parametrize("B", [1, 2, 67, 300])
def test_cg_reference_solves_the_dense_system(B, P, precondition):
    g = np.random.default_rng(1000 * B + P)
    O = g.normal(size=(B, P)) * np.exp(g.normal(size=P))
    rhs = g.normal(size=B)
    rhs -= rhs.mean()
    if B == 1:
        rhs = np.array([0.7])   # (a centred one-vector is zero; the entry documents y = rhs / lambda for B == 1)
    damping, rel = 1e-3, 1e-2
    y, info = sr.cg_reference(O, rhs, damping=damping, relative_damping=rel, tol=1e-13, max_iter=5000, precondition=precondition)
    H = np.eye(B) - 1.0 / B
    lam = damping + rel * np.trace(H @ O @ O.T @ H / B) / B
    want = np.linalg.solve(_dense(O, lam), rhs)
    assert info[0] == 0 and abs(info[3] - lam) <= 1e-12 * lam
    assert info[2] <= 1e-13
    assert np.linalg.norm(y - want) <= 1e-10 * np.linalg.norm(want), (np.linalg.norm(y - want) / np.linalg.norm(want), info)


def test_trace_identity():
    """trace(H O O^T H / B) = sum_b |o_b - obar|^2 / B, and its summands are the diagonal (the Jacobi preconditioner)."""
    g = np.random.default_rng(5)
    for B, P in ((1, 3), (2, 5), (67, 257), (300, 41)):
        O = g.normal(size=(B, P)) + g.normal(size=P)
        H = np.eye(B) - 1.0 / B
        T = H @ O @ O.T @ H / B
        d = ((O - O.mean(0)) ** 2).sum(1) / B
        assert np.abs(np.diag(T) - d).max() <= 1e-12 * max(1.0, np.abs(d).max())
        assert abs(np.trace(T) - d.sum()) <= 1e-12 * max(1.0, d.sum())


def test_cg_reference_edge_states():
    g = np.random.default_rng(6)
    O = g.normal(size=(20, 7))
    y, info = sr.cg_reference(O, np.zeros(20), relative_damping=1e-2)
    assert not y.any() and info[0] == 0 and info[1] == 0 and info[2] == 0
    bad = O.copy()
    bad[3, 2] = np.nan
    y, info = sr.cg_reference(bad, g.normal(size=20), relative_damping=1e-2)
    assert np.isnan(y).all() and info[0] == 2
    rhs = g.normal(size=20)
    rhs -= rhs.mean()
    y, info, steps = sr.cg_reference(O, rhs, relative_damping=1e-2, tol=1e-10, max_iter=2, history=True)
    assert info[0] == 1 and info[1] == 2 and len(steps) == 2 and info[2] == steps[-1][0] > 1e-10
    assert abs(steps[-1][0] - steps[-1][1]) <= 1e-12


def test_cg_prototype_table_matches_the_header_and_the_library():
    declared = header_prototypes(HEADER)
    assert list(declared) == list(sr.CG_PROTOTYPES) == NAMES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = sr.lib()
    for name, (ret, args) in declared.items():
        assert hasattr(raw, name), name
        restype, argtypes = sr.CG_PROTOTYPES[name]
        assert [ctypes_class(t) for t in argtypes] == args, (name, args)
        assert ctypes_class(restype) == ret
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes)
    assert declared["wf_sr_cg_solve"][1].count("f64") == 3 and declared["wf_sr_cg_solve"][1].count("i32") == 3
    assert not set(declared) & (set(_lib.PROTOTYPES) | set(sr.PROTOTYPES) | set(sr.STEP_PROTOTYPES) | set(sr.SPRING_PROTOTYPES))
    assert len(sr.PROTOTYPES) == 4 and len(sr.STEP_PROTOTYPES) == 2 and len(sr.SPRING_PROTOTYPES) == 5
    assert '#include "waveflow_sr_spring.h"' in open(HEADER).read() and "WF_ABI_VERSION" not in no_comments(HEADER)
    assert L.wf_abi_version() == 2


def test_c_entries_refuse_bad_arguments_on_the_host():
    L = sr.lib()
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    assert L.wf_sr_cg_workspace_bytes(0, 5) == L.wf_sr_cg_workspace_bytes(5, 0) == -1
    assert L.wf_sr_cg_workspace_bytes(65537, 5) == -2
    for B, P in ((1, 1), (67, 257), (5000, 129), (16384, 32588)):
        need = L.wf_sr_cg_workspace_bytes(B, P)
        assert need >= (B * 8 + 255) // 256 * 256 + (B + 31) // 32 * P * 8   # at least what wf_sr_apply asks for: the apply behind the solve shares it
        assert need >= 8 * (4 * B + 2 * P + (B + 31) // 32 * P) and need % 256 == 0
        assert need <= 8 * (5 * B + 2 * P + (B + 31) // 32 * P + (P + 255) // 256) + 10 * 256   # no B x B term

    def call(rows=one, B=8, P=4, ld=4, rhs=one, damping=(0.0, 1e-3), tol=1e-8, n_iter=4, y=one, info=one, ws=one, nbytes=1 << 30):
        return L.wf_sr_cg_solve(rows, B, P, ld, rhs, damping[0], damping[1], tol, n_iter, 1, 1, y, info, ws, nbytes, None)
    assert call(B=0) == -1 and call(P=0) == -1 and call(ld=3) == -1 and call(n_iter=-1) == -1
    for name in ("rows", "rhs", "y", "info", "ws"):
        assert call(**{name: None}) == -1, name
    for bad in ((-1.0, 1e-3), (1e-3, -1.0), (float("nan"), 1e-3), (0.0, float("nan"))):
        assert call(damping=bad) == -1, bad
    for tol in (0.0, 1.0, -1e-3, 2.0, float("nan")):
        assert call(tol=tol) == -1, tol
    assert call(nbytes=L.wf_sr_cg_workspace_bytes(8, 4) - 1) == -1
    assert call(B=65537) == -2


def test_python_surface_refuses_before_any_launch():
    import torch
    rows, rhs, e, prev = torch.zeros(8, 5), torch.zeros(8, dtype=torch.float64), torch.zeros(8), torch.zeros(5)
    with pytest.raises(ValueError, match="both zero"):
        sr.solve_cg(rows, rhs, damping=0.0, relative_damping=0.0)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        sr.solve_cg(rows, rhs, tol=0.0)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        sr.solve_cg(rows, rhs, tol=1.0)
    with pytest.raises(ValueError, match="max_iter"):
        sr.solve_cg(rows, rhs, max_iter=0)
    with pytest.raises(ValueError, match="round_iters"):
        sr.solve_cg(rows, rhs, round_iters=0)
    with pytest.raises(ValueError, match="float32"):
        sr.solve_cg(rows.double(), rhs)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sr.solve_cg(rows, rhs)
    with pytest.raises(ValueError, match="at most 65536"):
        sr.solve_cg(torch.zeros(65537, 1), torch.zeros(65537, dtype=torch.float64))
    for call in (lambda **k: sr.natural_gradient(rows, e, **k), lambda **k: sr.spring_direction(rows, e, prev, 0.5, **k)):
        with pytest.raises(ValueError, match="solver"):
            call(solver="lu")
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            call(solver="cg", tol=3.0)
        with pytest.raises(ValueError, match="max_iter"):
            call(solver="cg", max_iter=0)
        with pytest.raises(ValueError, match="no CPU fallback"):
            call(solver="cg")
    # 'cg' lifts the 4096-walker limit (the next check, for a cuda tensor, is what refuses these CPU rows); 'cholesky' keeps it
    big, ebig = torch.zeros(4097, 2), torch.zeros(4097)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sr.natural_gradient(big, ebig, solver="cg")
    with pytest.raises(ValueError, match="at most 4096"):
        sr.natural_gradient(big, ebig)
    with pytest.raises(ValueError, match="no CPU fallback"):
        sr.spring_direction(big, ebig, torch.zeros(2), 0.5, solver="cg")
    with pytest.raises(ValueError, match="at most 4096"):
        sr.spring_direction(big, ebig, torch.zeros(2), 0.5, solver="cholesky")
    with pytest.raises(ValueError, match="solver"):
        vqmc.sr_natural_gradient(None, None, None, None, solver="qr")
    with pytest.raises(ValueError, match="solver"):
        vqmc.spring_direction(None, None, None, None, prev, 0.5, solver="qr")
    with pytest.raises(ValueError, match="solver"):
        vqmc.train_step_sr(1, None, None, None, None, 1e-2, solver="qr")
    with pytest.raises(ValueError, match="solver"):
        vqmc.train_step_spring(1, None, None, None, None, 1e-2, prev, 0.5, 1e-3, 5.0, solver="qr")


def test_trainer_refuses_cg_with_the_device_side_step():
    t = vqmc.ModelTrainer(num_epochs=1)
    assert t.sr_solver == 'cholesky' and t._sr_solver_args() == {}
    t.sr_solver = 'cg'
    assert t._sr_solver_args() == {"solver": "cg"}
    for optimizer in ("sr", "spring"):
        t.optimizer, t.sr_on_device = optimizer, True
        with pytest.raises(ValueError, match="sr_on_device"):
            t.start_training(verbose=False)
    t.sr_on_device, t.sr_solver = False, 'lu'
    with pytest.raises(ValueError, match="solver"):
        t.start_training(verbose=False)
    old = vqmc.ModelTrainer(num_epochs=1)
    del old.sr_solver            # an object from before the attribute existed
    assert old._sr_solver_args() == {}


def _record_calls(monkeypatch):
    """sr's launchers replaced by recorders that return CPU tensors of the right shapes; the checks accept CPU tensors."""
    import torch
    calls = []
    monkeypatch.setattr(sr, "_check_rows", lambda rows, limit=None: (int(rows.shape[0]), int(rows.shape[1]), int(rows.shape[1])))
    monkeypatch.setattr(sr, "_check_vector", lambda *a, **k: None)

    def rec(name, result):
        def f(*args):
            calls.append(name)
            return result(*args)
        monkeypatch.setattr(sr, name, f)
    rec("_workspace", lambda B, P, dev: "dense-ws")
    rec("_cg_workspace", lambda B, P, dev: "cg-ws")
    rec("_gram", lambda rows, B, P, ld, ws: torch.zeros(B, B, dtype=torch.float64))
    rec("_solve", lambda T, B, rhs, d, rd, ws: (torch.zeros(B, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)))
    rec("_solve_cg", lambda rows, B, P, ld, rhs, d, rd, tol, mi, ri, pre, ws: (torch.zeros(B, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)))
    rec("_apply", lambda rows, B, P, ld, y, scale, ws: torch.zeros(P))
    rec("_matvec", lambda rows, B, P, ld, v: torch.zeros(B, dtype=torch.float64))
    rec("_apply_add", lambda rows, B, P, ld, y, scale, prev, mu, out, ws: out)
    return calls


def test_default_solver_makes_the_calls_it_made_before(monkeypatch):
    import torch
    calls = _record_calls(monkeypatch)
    rows, e, prev = torch.zeros(8, 5), torch.arange(8.0), torch.zeros(5)
    sr.natural_gradient(rows, e)
    assert calls == ["_workspace", "_gram", "_solve", "_apply"]
    del calls[:]
    sr.natural_gradient(rows, e, solver="cholesky", tol=1e-3, max_iter=5)
    assert calls == ["_workspace", "_gram", "_solve", "_apply"]
    del calls[:]
    sr.spring_direction(rows, e, prev, 0.9, clip=5.0)
    assert calls == ["_workspace", "_matvec", "_gram", "_solve", "_apply_add"]
    del calls[:]
    sr.natural_gradient(rows, e, solver="cg")
    assert calls == ["_cg_workspace", "_solve_cg", "_apply"]          # no Gram matrix, no dense workspace
    del calls[:]
    sr.spring_direction(rows, e, prev, 0.9, clip=5.0, solver="cg")
    assert calls == ["_cg_workspace", "_matvec", "_solve_cg", "_apply_add"]
    del calls[:]
    sr.spring_direction(rows, e, prev, 0.0, solver="cg")
    assert calls == ["_cg_workspace", "_solve_cg", "_apply_add"]


def test_vqmc_passes_the_solver_only_when_it_is_not_the_default(monkeypatch):
    """vqmc.sr_natural_gradient / spring_direction call sr with exactly today's keywords under 'cholesky', and add solver / tol / max_iter for 'cg'."""
    import torch
    seen = []

    class Model:
        def psi_jacobian(self, x, w_psi=None):
            return torch.zeros(4, 3)
    monkeypatch.setattr(vqmc, "_energy_terms", lambda params, psi, h_fn, batch: (Model(), None, torch.ones(4), torch.ones(4), None))
    monkeypatch.setattr(sr, "natural_gradient", lambda rows, e, **kw: seen.append(("sr", kw)) or torch.zeros(3))
    monkeypatch.setattr(sr, "spring_direction", lambda rows, e, prev, mu, **kw: seen.append(("spring", kw)) or torch.zeros(3))
    vqmc.sr_natural_gradient(None, None, None, None, relative_damping=1e-2)
    vqmc.sr_natural_gradient(None, None, None, None, relative_damping=1e-2, solver="cg", tol=1e-6)
    vqmc.spring_direction(None, None, None, None, torch.zeros(3), 0.9, clip=5.0)
    vqmc.spring_direction(None, None, None, None, torch.zeros(3), 0.9, clip=5.0, solver="cg", max_iter=77)
    assert seen == [("sr", {"damping": 0.0, "relative_damping": 1e-2}),
                    ("sr", {"damping": 0.0, "relative_damping": 1e-2, "solver": "cg", "tol": 1e-6, "max_iter": 2000}),
                    ("spring", {"damping": 0.0, "relative_damping": 1e-3, "clip": 5.0}),
                    ("spring", {"damping": 0.0, "relative_damping": 1e-3, "clip": 5.0, "solver": "cg", "tol": 1e-8, "max_iter": 77})]
