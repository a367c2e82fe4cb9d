"""Cost of stochastic reconfiguration from the per-walker rows (wf_sr_gram, wf_sr_solve, wf_sr_apply, and sr.natural_gradient for the three in a
row) for He (the shipped checkpoint's shape, 32 588 parameters) at 128, 1024 and 4096 walkers, next to the same three steps done with torch:
rows.double() @ rows.double().T, torch.linalg.cholesky + cholesky_solve, and the matvec rows.T @ y (fp64 accumulation through rows.double()
would double the rows in memory; torch's line reads the fp32 rows).  The torch line is the yardstick: the centring and the shift are left out of
it (O(B^2) against the product's O(B^2 P)).  The rows are wf_psi_jac's for the model's own walkers, written once.  hipEvents around each call,
3 warm-up calls per variant, then --repeats rounds in which the variants alternate.  Prints one JSON line per batch size: mean and min .. max
of each variant in ms.

    python examples/bench_sr.py [--repeats 7]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import _lib, model_factory, sr  # noqa: E402


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
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024, 4096])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sr.py needs a GPU"
    assert a.repeats >= 5
    m = model(2)
    L = sr.lib()
    for B in a.batches:
        g = np.random.default_rng(0)
        x = torch.from_numpy(np.sort(g.uniform(-10, 10, size=(B, 2)).astype(np.float32), -1)).cuda()
        ps = m.psi(x)
        rows = m.psi_jacobian(x, w_psi=1.0 / (ps + 1e-8))
        e = torch.from_numpy(g.normal(size=B)).cuda()
        rhs = e - e.mean()
        P = m.n_params
        # the C entries with buffers allocated once: the timed region holds the launches only
        ws = torch.empty(int(L.wf_sr_workspace_bytes(B, P)), device="cuda", dtype=torch.uint8)
        T, T0 = torch.empty(B, B, dtype=torch.float64, device="cuda"), torch.empty(B, B, dtype=torch.float64, device="cuda")
        y, info, out = torch.empty(B, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(P, device="cuda")
        R, S, n, st = rows.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()
        _lib.check(L.wf_sr_gram(R, B, P, P, T0.data_ptr(), S, n, st), "wf_sr_gram")
        lam = 1e-3 * float(torch.diagonal(T0).sum()) / B

        def solve():   # (the factorisation is in place: the copy of the matrix is part of neither line's time -- see solve_copy)
            T.copy_(T0)
            _lib.check(L.wf_sr_solve(T.data_ptr(), B, rhs.data_ptr(), 0.0, 1e-3, y.data_ptr(), info.data_ptr(), S, n, st), "wf_sr_solve")

        variants = {
            "gram": lambda: _lib.check(L.wf_sr_gram(R, B, P, P, T.data_ptr(), S, n, st), "wf_sr_gram"),
            "solve_copy": lambda: T.copy_(T0),
            "solve_with_copy": solve,
            "apply": lambda: _lib.check(L.wf_sr_apply(R, B, P, P, y.data_ptr(), 2.0 / B, out.data_ptr(), S, n, st), "wf_sr_apply"),
            "natural_gradient": lambda: sr.natural_gradient(rows, e),
        }
        torch_ok, why = True, ""
        try:
            rd = rows.double()
            A0 = T0 + lam * torch.eye(B, dtype=torch.float64, device="cuda")
            yt = torch.cholesky_solve(rhs[:, None], torch.linalg.cholesky(A0))[:, 0]
            torch.cuda.synchronize()
            agree = float((yt - _solved(L, T, T0, rhs, y, info, S, n, st, B)).norm() / yt.norm())
        except Exception as ex:   # (torch's fp64 solver needs its own device library; say so and time the rest)
            torch_ok, why = False, f"{type(ex).__name__}: {ex}"
        if torch_ok:
            y32 = y.float()
            variants.update({
                "torch_gram_with_cast": lambda: rows.double() @ rows.double().T,
                "torch_gram_fp64_rows": lambda: rd @ rd.T,
                "torch_solve": lambda: torch.cholesky_solve(rhs[:, None], torch.linalg.cholesky(A0)),
                "torch_matvec_fp32": lambda: rows.T @ y32,
            })
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(once(fn))
        r = {"model": "He", "batch": B, "n_params": P, "repeats": a.repeats, "rows_bytes": B * P * 4, "workspace_bytes": n, "info": int(info.item())}
        for k, v in ts.items():
            r[k + "_ms"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        r["solve_ms_minus_copy"] = float(f"{np.mean(ts['solve_with_copy']) - np.mean(ts['solve_copy']):.4g}")
        r["gram_TFLOPs_lower_triangle"] = float(f"{B * (B + 1) * P / (np.mean(ts['gram']) * 1e-3) / 1e12:.4g}")
        r["apply_rows_TBps"] = float(f"{B * P * 4 / (np.mean(ts['apply']) * 1e-3) / 1e12:.4g}")
        if torch_ok:
            r["solve_rel_diff_to_torch"] = float(f"{agree:.3g}")
        else:
            r["torch"] = "unavailable on this device: " + why
        print(json.dumps(r), flush=True)
        del x, rows, ws, T, T0
        if torch_ok:
            del rd, A0
        torch.cuda.empty_cache()


def _solved(L, T, T0, rhs, y, info, S, n, st, B):
    T.copy_(T0)
    _lib.check(L.wf_sr_solve(T.data_ptr(), B, rhs.data_ptr(), 0.0, 1e-3, y.data_ptr(), info.data_ptr(), S, n, st), "wf_sr_solve")
    torch.cuda.synchronize()
    return y


if __name__ == "__main__":
    main()
