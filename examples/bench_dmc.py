"""Time of one DMC generation (DeviceModel.dmc_step: propose, coordinate derivatives at the proposals, accept, the comb, the ring record) for
the shipped He model, captured once in a hipGraph and replayed, beside the one library call it is built around:

  dmc      the captured step
  derivs   model.psi_derivatives(hessian_diag=True, return_psi=True) on the population's walkers at the same size in the same process,
           with torch's allocations of its outputs as an eager caller pays them

A repeat times --steps consecutive steps between two hipEvents.  Each variant first runs until --warmup-seconds have passed (sustained clocks,
code objects loaded, allocator warm); then --repeats rounds in which the variants alternate.  Prints one JSON line per population size: mean
and min .. max in ms per step, and what the run measured (so that a run that walked nowhere cannot pass).  --profile-steps N instead replays
N steps per size and exits: the body of a `rocprofv3 --kernel-trace --stats -- python examples/bench_dmc.py --profile-steps 50` run.

    python examples/bench_dmc.py [--repeats 7] [--sizes 2048 16384 131072]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveflow_amd import model_factory, vqmc  # noqa: E402
from waveflow_amd.utils import physics  # noqa: E402

SEED = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 1 << 14, 1 << 17])
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dmc.py needs a GPU"
    assert a.repeats >= 5
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    _, psi, _, _ = init_fun(42, 2)
    model = psi.model
    flat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "he_checkpoint.npz"))["flat"]
    model.set_params_device(torch.as_tensor(np.asarray(flat, dtype=np.float32)).cuda())
    protons, _ = physics.system_catalogue[1]["He"]
    for B in a.sizes:
        state = model.make_dmc_state(B, ring_len=4096)
        state.st["ws"] = model._workspace(model.dmc_workspace_bytes(B), state.device)
        model.dmc_init(state, SEED, protons)

        def step():
            # (the shipped checkpoint is kept for parity and is no ground state -- <E_L> = 248, DESIGN 4.22: the energy cut keeps exp() in
            # range for it; the launches and their cost are those of any run)
            model.dmc_step(state, SEED, protons, a.tau, limit_drift=True, e_cut=1.0)
        launch = vqmc.capture_step(model, step, warm_up=step)

        def dmc_steps(n):
            for _ in range(n):
                launch()

        def derivs_steps(n):
            for _ in range(n):
                model.psi_derivatives(state.x, hessian_diag=True, return_psi=True)

        if a.profile_steps:
            dmc_steps(a.profile_steps)
            derivs_steps(a.profile_steps)
            torch.cuda.synchronize()
            continue
        variants = {"dmc": dmc_steps, "derivs": derivs_steps}

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
        first = int(state.counter.item())
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(window(fn, a.steps))
        torch.cuda.synchronize()
        done = int(state.counter.item())
        ring = state.ring.cpu().numpy()
        rows = ring[[g % state.ring_len for g in range(max(first, done - state.ring_len), done)]]
        r = {"model": "He", "walkers": B, "tau": a.tau, "repeats": a.repeats, "steps_per_window": a.steps, "warmup_steps": warm,
             "workspace_bytes": int(state.st["ws"].numel())}
        for k, v in ts.items():
            r[k + "_ms_per_step"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        r["dmc_over_derivs"] = float(f"{np.mean(ts['dmc']) / np.mean(ts['derivs']):.4g}")
        r["own_kernels_ms"] = float(f"{np.mean(ts['dmc']) - np.mean(ts['derivs']):.4g}")
        r["walkers_per_second"] = float(f"{B / (np.mean(ts['dmc']) * 1e-3):.4g}")
        r["measured"] = {"generations": done, "timed": done - first, "e_mixed": float(f"{(rows[:, 1] / rows[:, 0]).mean():.6g}"),
                         "acceptance": float(f"{rows[:, 3].sum() / (B * len(rows)):.4g}"), "status": int(state.status.item())}
        assert done - first == a.repeats * a.steps and np.isfinite(rows).all() and int(state.status.item()) == 0
        print(json.dumps(r), flush=True)
        del launch, state
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
