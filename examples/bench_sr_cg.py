"""The matrix-free solve of stochastic reconfiguration (sr.solve_cg, include/waveflow_sr_cg.h) on He's Jacobian rows (32 588 parameters):

  - at 1024 and 4096 walkers next to the dense path (sr.gram + sr.solve) with the same damping, and the distance between the two solutions;
  - at 16 384 walkers, where the dense path does not exist, on its own;
  - per size: iterations used with and without the Jacobi preconditioner, the time of one iteration (a window of --iters iterations of a solve
    that is kept from converging, between two hipEvents), that time against twice the rows' bytes at 4.8 TB/s (what the RQS kernel streams), and
    against one sr.matvec plus one sr.apply on the same rows in the same process -- the two passes an iteration is made of.

The rows are those of vqmc.sr_natural_gradient: psi_jacobian of the tests' He checkpoint (a fresh model without it) on sorted uniform walkers in
(-8, 8)^2, weight 1 / (psi + 1e-8); the right-hand side is H e_loc.  Prints one JSON line per batch size.

    python examples/bench_sr_cg.py [--batches 1024 4096 16384] [--repeats 5] [--iters 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from waveflow_amd import checkpoint, model_factory, sr, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

STREAM_BYTES_PER_S = 4.8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--relative-damping", type=float, default=1e-3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=4000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sr_cg.py needs a GPU"
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    params, psi, _, _ = init_fun(0, 2)
    ckpt = os.path.join(ROOT, "tests", "golden", "he_checkpoint.npz")
    if os.path.exists(ckpt):
        params = checkpoint.unflatten_like(params, np.load(ckpt)["flat"])
    protons, _ = physics.system_catalogue[1]["He"]
    h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
    rel = a.relative_damping

    def timed(fn, n=1):
        """mean, min, max ms per unit over --repeats windows of fn(), each between two events, after one warm call"""
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.repeats):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e) / n)
        return {"mean": float(f"{np.mean(ts):.4g}"), "min": float(f"{np.min(ts):.4g}"), "max": float(f"{np.max(ts):.4g}")}

    for B in a.batches:
        g = np.random.default_rng(B)
        x = torch.as_tensor(np.sort(g.uniform(-8.0, 8.0, size=(B, 2)).astype(np.float32), -1)).cuda()
        model, xd, hpsi, ps, _ = vqmc._energy_terms(params, psi, h_fn, x)
        inv = 1.0 / (ps + 1e-8)
        e = (hpsi * inv).double()
        rows = model.psi_jacobian(xd, w_psi=inv)
        rhs = e - e.mean()
        P, ld = int(rows.shape[1]), int(rows.stride(0))
        ws = sr._cg_workspace(B, P, rows.device)
        r = {"model": "He", "batch": B, "n_params": P, "rows_bytes": B * P * 4, "relative_damping": rel, "tol": a.tol, "repeats": a.repeats}
        solved = {}
        for pre in (True, False):
            name = "jacobi" if pre else "plain"
            try:
                t0 = time.perf_counter()
                y, info = sr.solve_cg(rows, rhs, relative_damping=rel, tol=a.tol, max_iter=a.max_iter, precondition=pre, workspace=ws)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                n_it = int(info.cpu().numpy()[1])
                r[f"solve_cg_{name}"] = {"iterations": n_it, "ms": float(f"{wall:.4g}"), "residual": float(f"{info.cpu().numpy()[2]:.3e}")}
                solved[pre] = y
            except sr.NotConverged as err:
                r[f"solve_cg_{name}"] = {"iterations": err.iterations, "not_converged_at": float(f"{err.residual:.3e}")}
        # one iteration: a solve that cannot converge (tol 1e-300 is never met), started once, then windows of --iters iterations
        y = torch.empty(B, dtype=torch.float64, device="cuda")
        info = torch.empty(4, dtype=torch.float64, device="cuda")
        sr._cg_call(rows, B, P, ld, rhs, 0.0, rel, 1e-300, 0, True, True, y, info, ws)
        r["iteration_ms"] = timed(lambda: sr._cg_call(rows, B, P, ld, rhs, 0.0, rel, 1e-300, a.iters, False, True, y, info, ws), a.iters)
        assert info.cpu().numpy()[0] == 1.0, "the timed iterations must all have run"
        r["restart_ms"] = timed(lambda: sr._cg_call(rows, B, P, ld, rhs, 0.0, rel, 1e-300, 0, True, True, y, info, ws))
        v, yv = torch.randn(P, device="cuda"), torch.randn(B, device="cuda", dtype=torch.float64)
        r["matvec_ms"] = timed(lambda: [sr.matvec(rows, v) for _ in range(a.iters)], a.iters)
        r["apply_ms"] = timed(lambda: [sr.apply(rows, yv, 2.0 / B, workspace=ws) for _ in range(a.iters)], a.iters)
        two = r["matvec_ms"]["mean"] + r["apply_ms"]["mean"]
        r["iteration_over_matvec_plus_apply"] = float(f"{r['iteration_ms']['mean'] / two:.3g}")
        r["two_passes_at_4p8_TBps_ms"] = float(f"{2 * B * P * 4 / STREAM_BYTES_PER_S * 1e3:.4g}")
        r["iteration_over_stream_time"] = float(f"{r['iteration_ms']['mean'] / r['two_passes_at_4p8_TBps_ms']:.3g}")
        if B <= sr.MAX_WALKERS:
            dws = sr._workspace(B, P, rows.device)

            def dense():
                T = sr.gram(rows, workspace=dws)
                return sr.solve(T, rhs, relative_damping=rel, workspace=dws)
            r["gram_plus_solve_ms"] = timed(dense)
            yd, pivot = dense()
            r["dense_pivot"] = int(pivot.item())
            for pre, yc in solved.items():
                r[f"cg_{'jacobi' if pre else 'plain'}_vs_dense"] = float(f"{float((yc - yd).norm() / yd.norm()):.3e}")
            del dws
        print(json.dumps(r), flush=True)
        del rows, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
