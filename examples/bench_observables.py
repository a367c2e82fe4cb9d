"""Time of one measurement step (DeviceModel.observe_step: sampler, coordinate derivatives, accumulation of the five per-walker values,
density and pair histograms) for the shipped He model, beside the two library calls it is built around:

  observe   the step -- captured once in a hipGraph and replayed at --graph-batch walkers (default 2^17), called eagerly at --eager-batch
            (default 2^20)
  parts     model.sample + model.psi_derivatives(hessian_diag=True) at the same batch in the same process: the walkers and the derivatives
            without any measurement, with torch's allocations of their outputs as an eager caller pays them

A repeat times --steps consecutive steps between two hipEvents.  Each variant first runs until --warmup-seconds have passed (sustained clocks,
code objects loaded, allocator warm); then --repeats rounds in which the variants alternate.  Prints one JSON line per batch size: mean and
min .. max in ms per step, walkers per second of the step, and what the step measured (so that a run that measured nothing cannot pass).

    python examples/bench_observables.py [--repeats 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import model_factory, observables, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

SEED = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--graph-batch", type=int, default=1 << 17)
    ap.add_argument("--eager-batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--bins", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_observables.py needs a GPU"
    assert a.repeats >= 5
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    _, psi, _, _ = init_fun(42, 2)
    model = psi.model
    flat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "he_checkpoint.npz"))["flat"]
    model.set_params_device(torch.as_tensor(np.asarray(flat, dtype=np.float32)).cuda())
    protons, _ = physics.system_catalogue[1]["He"]
    for B, captured in ((a.graph_batch, True), (a.eager_batch, False)):
        acc = observables.Accumulator(model.D, a.bins, a.bins, model=model)
        counter = torch.zeros(1, dtype=torch.int64, device=acc.device)
        acc.st["ws"] = model._workspace(model.observe_step_workspace_bytes(B), acc.device)

        def step():
            model.observe_step(acc, counter, SEED, B, protons, exact_sampler=True)
        launch = vqmc.capture_step(model, step, warm_up=step) if captured else step
        drawn = [0]

        def observe_steps(n):
            for _ in range(n):
                launch()

        def parts_steps(n):
            for _ in range(n):
                drawn[0] += 1
                x = model.sample(SEED + drawn[0], B, exact=True)
                model.psi_derivatives(x, hessian_diag=True, return_psi=True)

        variants = {"observe": observe_steps, "parts": parts_steps}

        def window(fn, n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(n)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / n

        warm = {}
        for k, fn in variants.items():
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < a.warmup_seconds:
                fn(a.steps)
                torch.cuda.synchronize()
                n += a.steps
            warm[k] = n
        acc.reset()
        counter.zero_()
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(window(fn, a.steps))
        torch.cuda.synchronize()
        res = acc.totals().result()
        r = {"model": "He", "batch": B, "captured": captured, "repeats": a.repeats, "steps_per_window": a.steps, "warmup_steps": warm, "bins": a.bins,
             "workspace_bytes": int(acc.st["ws"].numel())}
        for k, v in ts.items():
            r[k + "_ms_per_step"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        r["observe_over_parts"] = float(f"{np.mean(ts['observe']) / np.mean(ts['parts']):.4g}")
        r["walkers_per_second"] = float(f"{B / (np.mean(ts['observe']) * 1e-3):.4g}")
        r["measured"] = {"n": res["n"], "n_skipped": res["n_skipped"], "steps": int(counter.item()), "e_loc": float(f"{res['e_loc']:.6g}"),
                         "e_loc_stderr": float(f"{res['e_loc_stderr']:.3g}"), "outside_density": res["outside_density"]}
        assert res["n"] + res["n_skipped"] == a.repeats * a.steps * B == int(counter.item()) * B
        print(json.dumps(r), flush=True)
        del launch, acc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
