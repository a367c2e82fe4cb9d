"""Cost of the per-walker parameter Jacobians (wf_logpdf_jac, wf_psi_jac) next to the contracted vector-Jacobian products on the same wave sweeps
(wf_logpdf_vjp, wf_psi_vjp with WF_GRAD_TILE_MIN=0) for He (the shipped checkpoint's shape, 32 588 parameters) at 128, 1024 and 4096 walkers.
The sweeps are shared: the difference is k_wjac, which writes B x n_params x 4 bytes, against k_wgrad + gather.  hipEvents around each call, 3
warm-up calls per variant, then --repeats rounds in which the variants alternate (one process, one allocation of the walkers and of the rows).
Prints one JSON line per batch size: mean and min .. max of each variant in ms, the bytes of the rows, the difference of each Jacobian call to
its contracted sibling, and the rows' bytes over the whole Jacobian call (a lower bound of k_wjac's store rate).

    python examples/bench_param_jacobian.py [--repeats 7]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import _lib, model_factory  # noqa: E402


def model(D):
    init_fun = model_factory.get_waveflow_model(D, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, sample = init_fun(42, D)
    psi.model.ensure_params(params)
    return psi.model


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_param_jacobian.py needs a GPU"
    assert a.repeats >= 5
    os.environ["WF_GRAD_TILE_MIN"] = "0"   # the contracted calls on the wave sweeps at every batch size (read per call)
    m = model(2)
    L = _lib.lib()
    for B in (128, 1024, 4096):
        g = np.random.default_rng(0)
        x = torch.from_numpy(np.sort(g.uniform(-10, 10, size=(B, 2)).astype(np.float32), -1)).cuda()
        one, zero = torch.ones(B, device="cuda"), torch.zeros(B, device="cuda")
        # the C entries with buffers allocated once: the timed region holds the launches only
        jac, grad = torch.empty(B, m.n_params, device="cuda"), torch.empty(m.n_params, device="cuda")
        ws = torch.empty(int(max(L.wf_psi_jac_workspace_bytes(m._h, B), L.wf_psi_vjp_workspace_bytes(m._h, B))), device="cuda", dtype=torch.uint8)
        X, J, G, S, n, st = x.data_ptr(), jac.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel(), m._stream()
        variants = {
            "logpdf_jacobian": lambda: _lib.check(L.wf_logpdf_jac(m._h, X, B, J, None, S, n, st), "wf_logpdf_jac"),
            "logpdf_vjp": lambda: _lib.check(L.wf_logpdf_vjp(m._h, X, B, one.data_ptr(), G, S, n, st), "wf_logpdf_vjp"),
            "psi_jacobian": lambda: _lib.check(L.wf_psi_jac(m._h, X, B, one.data_ptr(), zero.data_ptr(), J, S, n, st), "wf_psi_jac"),
            "psi_vjp": lambda: _lib.check(L.wf_psi_vjp(m._h, X, B, one.data_ptr(), zero.data_ptr(), G, S, n, st), "wf_psi_vjp"),
        }
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(once(fn))
        row_bytes = B * m.n_params * 4
        r = {"model": "He", "batch": B, "n_params": m.n_params, "repeats": a.repeats, "jacobian_bytes": row_bytes}
        for k, v in ts.items():
            r[k + "_ms"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        for k in ("logpdf", "psi"):
            extra = np.mean(ts[k + "_jacobian"]) - np.mean(ts[k + "_vjp"])
            r[k + "_jacobian_minus_vjp_ms"] = float(f"{extra:.4g}")
            r[k + "_bytes_over_whole_call_TBps"] = float(f"{row_bytes / (np.mean(ts[k + '_jacobian']) * 1e-3) / 1e12:.4g}")
        print(json.dumps(r), flush=True)
        del x, jac, ws


if __name__ == "__main__":
    main()
