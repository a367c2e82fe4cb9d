"""Walkers per second of the 8-electron chain (D = 8, k = 6, 3 layers, box 10) at 33 knots (39 I-bases / 38 B-bases: the 64-row layouts) next
to the same model at 23 knots (29 / 28 bases): log_pdf, H psi, loss + gradient (wf_vqmc_loss_grad) and sample at 2^17 walkers.  For 33 knots
the second-order sweeps run in R3 by default; the RF forms (WF_WIDE_RF) are timed as well.  hipEvents around each call, 3 warm-up calls,
median of --iters timed ones.  Prints one JSON line per (knots, form).

    python examples/bench_wide_chains.py [--batch 131072] [--iters 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import model_factory  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def chain(kn):
    init_fun = model_factory.get_waveflow_model(8, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=kn, n_i_internal_knots=kn,
                                                i_spline_reg=0.05, i_spline_reverse_fun_tol=1e-6, n_flow_layers=3, box_size=10.0)
    params, psi, log_pdf, sample = init_fun(42, 8)
    psi.model.ensure_params(params)
    return psi.model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 17)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wide_chains.py needs a GPU"
    B = a.batch
    g = np.random.default_rng(0)
    x = torch.from_numpy(np.sort(g.uniform(-10, 10, size=(B, 8)).astype(np.float32), -1)).cuda()
    protons = np.linspace(-3.5, 3.5, 8)
    for kn, form in ((23, "default"), (33, "default"), (33, "WF_WIDE_RF")):
        if form == "WF_WIDE_RF":
            os.environ["WF_WIDE_RF"] = "1"        # read per call by H psi, at model creation by the gradient
        m = chain(kn)
        r = {"knots": kn, "i_bases": m.i_nb, "form": form, "batch": B}
        r["log_pdf"] = B / timed(lambda: m.log_pdf(x), a.iters)
        r["hpsi"] = B / timed(lambda: m.hamiltonian(x, protons), a.iters)
        r["loss_grad"] = B / timed(lambda: m.vqmc_loss_grad(x, protons, -2.0), a.iters)
        r["sample"] = B / timed(lambda: m.sample(7, B, exact=True), a.iters)
        os.environ.pop("WF_WIDE_RF", None)
        print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
        del m


if __name__ == "__main__":
    main()
