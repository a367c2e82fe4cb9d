"""Per-step time of stochastic reconfiguration for He (32 588 parameters) at 128, 1024 and 4096 walkers per step, three ways:

  eager    the loop of ModelTrainer._train_sr: sample -> vqmc.train_step_sr -> copy the new parameters back (allocates rows, matrix and
           workspace every step, waits for the device twice per step) -- the yardstick
  direct   DeviceModel.sr_step (wf_vqmc_sr_step) called once per step: the same arithmetic, one workspace, no wait
  graph    that step captured once in a hipGraph and replayed

Every variant keeps its own parameter vector and does the whole arithmetic of a step, update included, at --learning-rate (default 0: the
parameters stay where they are, so the work per step does not drift and the three variants stay comparable; from a fresh initialisation a
stochastic-reconfiguration step has |d|^2 of 1e12 and more, and a run at 1e-4 leaves the region of finite psi within 50 steps whichever
variant computes it).  A repeat times --steps consecutive steps between two
hipEvents (the eager loop's host waits are inside the window, as they are in training) and reports the time per step.  Each variant first runs
until --warmup-seconds have passed (sustained clocks, code objects loaded, torch's allocator warm); then --repeats rounds in which the three
variants alternate.  Prints one JSON line per batch size: mean and min .. max of each variant in ms per step, the launches a captured step
holds, and the steps the solver refused (expected: 0).

    python examples/bench_sr_step.py [--repeats 7] [--batches 128 1024 4096]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import core, model_factory, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

SEED = 11


def launches_per_step(B):
    """Kernel launches of one wf_vqmc_sr_step at B walkers (wave sampler, one chunk of rows), counted from the sequence in DESIGN 4.20."""
    panels = (B + 31) // 32
    solve = 1 + panels + 2 * (panels - 1) + panels          # shift; potrf per panel; trsm + syrk below every panel but the last; back substitution
    # ("rhs": without momentum the one-block right-hand side runs ahead of the rows and computes inv and e_loc itself; a SPRING step with
    # momentum has three there instead: e_loc, q = O phi, rhs)
    n = {"sampler": 1, "energy": 2, "rhs": 1, "rows": 3, "gram": 5, "solve": solve, "apply": 3, "verdict_update": 2, "images": 1,
         "ring": 1 if B <= 256 else 2}
    n["total"] = sum(n.values())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024, 4096])
    ap.add_argument("--steps", type=int, nargs="+", default=None, help="steps per timed window, one per batch size (default: 200, 20, 5)")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--learning-rate", type=float, default=0.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sr_step.py needs a GPU"
    assert a.repeats >= 5
    LR = a.learning_rate
    steps_of = dict(zip(a.batches, a.steps)) if a.steps else {}
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    template, psi, _, sample = init_fun(42, 2)
    model = psi.model
    protons, _ = physics.system_catalogue[1]["He"]
    h_fn = physics.construct_hamiltonian_function(psi, protons=protons, n_space_dimensions=1, eps=0.0)
    flat0 = torch.as_tensor(core.flatten_params(template).astype(np.float32)).cuda()
    for B in a.batches:
        n_steps = steps_of.get(B, 200 if B <= 256 else 20 if B <= 2048 else 5)

        # eager: the parent's loop
        eager = {"flat": flat0.clone(), "version": 0, "epoch": 0}

        def eager_steps(n):
            for _ in range(n):
                eager["epoch"] += 1
                params = core.DeviceParams(template, eager["flat"], eager["version"])
                batch = sample(SEED + eager["epoch"], params, B, exact_inverse=False)
                new, _ = vqmc.train_step_sr(eager["epoch"], psi, h_fn, params, batch, LR)
                eager["flat"].copy_(new.flat)
                eager["version"] += 1

        # the device-side step, called and replayed; each with its own parameters, state and workspace
        states = {}
        for name in ("direct", "graph"):
            x = flat0.clone()
            st = model.make_sr_train_state(x, 1, LR, defer_eval_tables=True)
            st["ws"] = model._workspace(model.sr_step_workspace_bytes(B), x.device)
            states[name] = (x, st)

        def device_step(name):
            x, st = states[name]
            model.sr_step(st, SEED, B, h_fn.protons)

        def direct_steps(n):
            model.set_params_device(states["direct"][0])
            for _ in range(n):
                device_step("direct")

        model.set_params_device(states["graph"][0])
        # (one step outside the capture: every kernel of the sequence has run once)
        replay = vqmc.capture_step(model, lambda: device_step("graph"), warm_up=lambda: device_step("graph"))

        def graph_steps(n):
            # (the model's images follow whichever parameter vector stepped last: hand them back to this variant's, as a trainer that shares
            # a model between optimisers would)
            model.set_params_device(states["graph"][0])
            for _ in range(n):
                replay()

        variants = {"eager": eager_steps, "direct": direct_steps, "graph": graph_steps}

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
                fn(n_steps)
                torch.cuda.synchronize()
                n += n_steps
            warm[k] = n
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(window(fn, n_steps))
        torch.cuda.synchronize()
        r = {"model": "He", "batch": B, "n_params": model.n_params, "repeats": a.repeats, "learning_rate": LR, "steps_per_window": n_steps, "warmup_steps": warm,
             "workspace_bytes": int(states["graph"][1]["ws"].numel()), "launches": launches_per_step(B)}
        for k, v in ts.items():
            r[k + "_ms_per_step"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        r["eager_over_graph"] = float(f"{np.mean(ts['eager']) / np.mean(ts['graph']):.4g}")
        r["skipped_steps"] = {k: int(states[k][1]["status"][1].item()) for k in states}
        r["finite"] = {"eager": bool(torch.isfinite(eager["flat"]).all()), **{k: bool(torch.isfinite(states[k][0]).all()) for k in states}}
        print(json.dumps(r), flush=True)
        del replay, states, eager
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
