"""The size query of every whole-step entry agrees with the way the entry carves its workspace (wf_vqmc_train_step, wf_vqmc_train_step_local,
wf_mle_train_step, wf_vqmc_sr_step; He).

Query and entry go by one layout function each.  With `workspace_bytes` equal to the query the step runs; with one byte less it returns
WF_ERR_INVALID before anything is launched: parameters, Adam moments, counter, running average, loss ring, SR's norm ring and status and the
reduce buffer of the local half stay bitwise as they were.  Two shapes: 67 walkers (ragged, the wave sampler and the wave sweeps) and 96 walkers
with WF_SAMPLE_TILE_MIN = WF_GRAD_TILE_MIN = 64, where the last area is the larger of what the matrix-core gradient and the staged sampler ask
for.  The buffer is always allocated at the full size (poisoned); only the number passed is reduced.
"""
import ctypes

import numpy as np
import pytest

from conftest import sorted_walkers

pytestmark = pytest.mark.gpu

SEED = 20240607
FIRST = 5
LR = 1e-3
WF_ERR_INVALID = -1   # include/waveflow_hip.h
SHAPES = {"wave-67": (67, {}), "tile-96": (96, {"WF_SAMPLE_TILE_MIN": "64", "WF_GRAD_TILE_MIN": "64"})}
_cache = {}


def _he(he_flat):
    """(psi, proton positions, flat parameters on the device)"""
    import torch
    from waveflow_amd import model_factory
    from waveflow_amd.utils import physics
    if "he" not in _cache:
        init = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
        _, psi, _, _ = init(7, 2)
        protons, _ = physics.system_catalogue[1]["He"]
        _cache["he"] = (psi, protons, torch.as_tensor(np.asarray(he_flat, dtype=np.float32)).cuda())
    return _cache["he"]


def _snapshot(tensors):
    import torch
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in tensors.items()}


def _same(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


@pytest.mark.parametrize("entry", ["train_step", "train_step_local", "mle_train_step", "sr_step"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_query_and_carving_agree(he_flat, monkeypatch, entry, shape):
    import torch
    from waveflow_amd import _lib, sr
    B, env = SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    psi, protons, flat0 = _he(he_flat)
    model = psi.model
    xs = flat0.clone()
    model.set_params_device(xs)
    pr, n_pr = model._protons(protons)
    stream = model._stream()
    if entry == "sr_step":
        st = model.make_sr_train_state(xs, FIRST, LR)
        watched = {k: st[k] for k in ("x", "counter", "step_size", "ring", "norm_ring", "status")}
        n = model.sr_step_workspace_bytes(B)

        def call(ws, nbytes):
            return sr.lib().wf_vqmc_sr_step(model._h, ctypes.byref(st["c"]), SEED, B, pr, n_pr, 0.0, 1e-3, 0, None, 1, ws, nbytes, stream)
    else:
        st = model.make_train_state(xs, torch.zeros_like(xs), torch.zeros_like(xs), FIRST)
        watched = {k: st[k] for k in ("x", "m", "v", "counter", "running_average", "ring")}
        c, L = ctypes.byref(st["c"]), _lib.lib()
        if entry == "train_step":
            n = model.train_step_workspace_bytes(B)

            def call(ws, nbytes):
                return L.wf_vqmc_train_step(model._h, c, SEED, B, pr, n_pr, LR, 0.9, 0.999, 1e-8, 0, ws, nbytes, stream)
        elif entry == "train_step_local":
            n = model.train_step_workspace_bytes(B)
            watched["red"] = torch.zeros(model.n_params + 3, dtype=torch.float64, device=xs.device)

            def call(ws, nbytes):
                return L.wf_vqmc_train_step_local(model._h, c, SEED, B, pr, n_pr, 1.0 / B, 0, watched["red"].data_ptr(), ws, nbytes, stream)
        else:
            n = model.mle_train_step_workspace_bytes(B)
            rows = torch.as_tensor(sorted_walkers(B, 2, 8.0, 5)).cuda()

            def call(ws, nbytes):
                return L.wf_mle_train_step(model._h, c, rows.data_ptr(), B, LR, 0.9, 0.999, 1e-8, ws, nbytes, stream)
    assert n > 0
    buf = torch.full((n,), 0xFF, dtype=torch.uint8, device=xs.device)
    before = _snapshot(watched)
    assert call(buf.data_ptr(), n - 1) == WF_ERR_INVALID
    assert _same(_snapshot(watched), before)   # nothing was launched
    assert call(buf.data_ptr(), n) == 0
    after = _snapshot(watched)
    if entry == "train_step_local":   # the half without an update: the packed buffer holds [gradient, sum E_L, sum E_L^2, walkers]
        red = after["red"]
        assert bool(torch.isfinite(red).all()) and float(red[-1]) == B and bool(red[:-3].any())
    else:
        assert int(after["counter"].item()) == FIRST + 1
        assert bool(torch.isfinite(after["x"]).all()) and not torch.equal(after["x"], flat0)
        slot = after["ring"][FIRST % st["ring_len"]]
        assert float(slot[2]) == B and np.isfinite(float(slot[0]))
    if entry == "sr_step":
        assert after["status"].tolist() == [0, 0]
