"""Host side of the per-walker parameter Jacobians (no GPU needed): the pytree with a batch axis, the memory check, the ABI declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from waveflow_amd import _lib, checkpoint, core, flows, model_factory, wavefunctions


def _he_template(gated):
    """The He parameter pytree (D = 2, k = 6, 23 knots, 3 layers) from the host-side initialisers; gated: set_nn_output_grad_to_zero=True throughout."""
    mt = model_factory.get_masked_transform
    if gated:
        imade = flows.IMADE(mt(), 6, 23, 0.05, 1e-6, {0: 0}, {0: 1}, set_nn_output_grad_to_zero=True)
        init_fun = wavefunctions.Waveflow(flows.Serial(flows.BoxTransformLayer(10.0), *(imade, flows.Reverse()) * 3), mt(allow_negative_params=True), 6, 23,
                                          constraints_dict_left={0: 0}, constraints_dict_right={0: 0}, constrained_dimension_indices_left=[0],
                                          set_nn_output_grad_to_zero=True)
    else:
        init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                    i_spline_reg=0.05, n_flow_layers=3, box_size=10)
    g = flows.as_generator(0)
    return (init_fun.transformation.init_params(g, 2), init_fun.sp.init_params(g, 2, 23 + 6 - 1))


@pytest.mark.parametrize("gated", [False, True])
def test_unflatten_batched_reproduces_leaf_order_and_shapes(gated):
    tree = _he_template(gated)
    leaves = core.tree_leaves(tree)
    n = core.flatten_params(tree).size
    assert n == 32588
    jac = np.arange(3 * n, dtype=np.float32).reshape(3, n) % 8191   # (exact in fp32; every row differs)
    out = core.unflatten_batched(tree, jac)
    got = core.tree_leaves(out)
    assert [a.shape for a in got] == [(3,) + tuple(np.shape(t)) for t in leaves]
    assert out[0][0] == () and out[0][2] == () and isinstance(out, tuple) and type(out[0]) is type(tree[0])   # Box and Reverse carry no leaves
    # row b of the pytree is what unflatten_like makes of row b: flatten_params' leaf order
    for b in range(3):
        row = core.tree_leaves(checkpoint.unflatten_like(tree, jac[b]))
        assert all(np.array_equal(a[b], r) for a, r in zip(got, row))
        assert np.array_equal(np.concatenate([a[b].reshape(-1) for a in got]), jac[b])
    # torch rows stay torch (views of the one tensor), DeviceParams stands for its template
    import torch
    t = torch.as_tensor(jac)
    tout = core.tree_leaves(core.unflatten_batched(core.DeviceParams(tree, None), t))
    assert all(isinstance(a, torch.Tensor) and a.data_ptr() >= t.data_ptr() for a in tout)
    assert all(np.array_equal(a.numpy(), r) for a, r in zip(tout, got))
    with pytest.raises(ValueError):
        core.unflatten_batched(tree, jac[:, :-1])
    with pytest.raises(ValueError):
        core.unflatten_batched(tree, jac[0])


def test_jacobian_memory_check_names_the_byte_count():
    assert core.check_jacobian_bytes(4096, 32588, 1 << 30) == 4096 * 32588 * 4
    with pytest.raises(ValueError, match=str(4096 * 32588 * 4)):
        core.check_jacobian_bytes(4096, 32588, 4096 * 32588 * 4 - 1)


def test_jacobian_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "waveflow_hip.h")).read()
    names = ["wf_logpdf_jac", "wf_logpdf_jac_workspace_bytes", "wf_psi_jac", "wf_psi_jac_workspace_bytes"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(rf"\b{n}\s*\(", hdr) and n in _lib.EXPORTS and hasattr(L, n), n
    B = _lib.lib()
    assert B.wf_logpdf_jac.argtypes[2] is ctypes.c_int64 and len(B.wf_logpdf_jac.argtypes) == 8 and len(B.wf_psi_jac.argtypes) == 9
    assert B.wf_psi_jac_workspace_bytes.restype is ctypes.c_int64
    # refusals that need no device
    assert B.wf_logpdf_jac_workspace_bytes(None, 8) == B.wf_psi_jac_workspace_bytes(None, 8) == -1
    assert B.wf_logpdf_jac(None, None, 8, None, None, None, 0, None) == B.wf_psi_jac(None, None, 8, None, None, None, None, 0, None) == -1


def test_closures_exist_and_train_step_is_not_rewired():
    import inspect
    from waveflow_amd import vqmc
    assert callable(vqmc.log_pdf_jacobian) and callable(vqmc.log_psi_jacobian)
    src = inspect.getsource(vqmc.train_step_gradients)
    assert "logpdf_vjp" in src and "jacobian" not in src
