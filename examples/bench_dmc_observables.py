"""Time of one DMC generation with its forward-walking update (DeviceModel.dmc_fw_step, 8 tag slots) for the shipped He model, captured once
in a hipGraph and replayed, beside the captured plain generation (DeviceModel.dmc_step) at the same size in the same process:

  dmc        the captured plain generation (what examples/bench_dmc.py times)
  fw1        the captured generation with the update, stride = 1: every generation measures 9 lags and retags
  fw20       the same with stride = 20: 19 generations out of 20 only compose the genealogy (4 launches that decide on the device)

A repeat times --steps consecutive steps between two hipEvents.  Each variant first runs until --warmup-seconds have passed; then --repeats
rounds in which the variants alternate.  Prints one JSON line per population size: mean and min .. max in ms per step, the differences to the
plain generation in microseconds, and what the run measured.  --profile-steps N instead replays N steps of fw20 per size and exits: the body
of a `rocprofv3 --kernel-trace --stats -- python examples/bench_dmc_observables.py --profile-steps 60` run.

    python examples/bench_dmc_observables.py [--repeats 7] [--sizes 2048 16384 131072]"""
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

SEED, SLOTS = 11, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 1 << 14, 1 << 17])
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window (a multiple of 20 holds one measurement of fw20 per 20)")
    ap.add_argument("--warmup-seconds", type=float, default=2.0)
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dmc_observables.py needs a GPU"
    assert a.repeats >= 5 and a.steps % 20 == 0
    init_fun = model_factory.get_waveflow_model(2, base_spline_degree=6, i_spline_degree=6, n_prior_internal_knots=23, n_i_internal_knots=23,
                                                i_spline_reg=0.05, n_flow_layers=3, box_size=10.0)
    _, psi, _, _ = init_fun(42, 2)
    model = psi.model
    flat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "he_checkpoint.npz"))["flat"]
    model.set_params_device(torch.as_tensor(np.asarray(flat, dtype=np.float32)).cuda())
    protons, _ = physics.system_catalogue[1]["He"]
    for B in a.sizes:
        runs = {}
        for name, stride in (("dmc", 0), ("fw1", 1), ("fw20", 20)):
            state = model.make_dmc_state(B, ring_len=4096)
            fw = model.make_forward_walk(B, SLOTS, stride, series_len=4096) if stride else None
            nbytes = model.dmc_fw_workspace_bytes(B, SLOTS) if stride else model.dmc_workspace_bytes(B)
            state.st["ws"] = model._workspace(nbytes, state.device)
            model.dmc_init(state, SEED, protons)

            def step(state=state, fw=fw):
                # (limit_drift and e_cut = 1 as examples/bench_dmc.py: the shipped checkpoint is no ground state)
                if fw is None:
                    model.dmc_step(state, SEED, protons, a.tau, limit_drift=True, e_cut=1.0)
                else:
                    model.dmc_fw_step(state, fw, SEED, protons, a.tau, limit_drift=True, e_cut=1.0)
            runs[name] = (vqmc.capture_step(model, step, warm_up=step), state, fw)

        def steps_of(name):
            launch = runs[name][0]

            def go(n):
                for _ in range(n):
                    launch()
            return go
        variants = {k: steps_of(k) for k in runs}
        if a.profile_steps:
            variants["fw20"](a.profile_steps)
            torch.cuda.synchronize()
            continue

        def window(fn, n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn(n)
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / n

        for k, fn in variants.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.warmup_seconds:
                fn(a.steps)
                torch.cuda.synchronize()
        first = {k: int(runs[k][1].counter.item()) for k in runs}
        ts = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ts[k].append(window(fn, a.steps))
        torch.cuda.synchronize()
        r = {"model": "He", "walkers": B, "slots": SLOTS, "tau": a.tau, "repeats": a.repeats, "steps_per_window": a.steps,
             "workspace_bytes": {k: int(runs[k][1].st["ws"].numel()) for k in runs}}
        for k, v in ts.items():
            r[k + "_ms_per_step"] = {"mean": float(f"{np.mean(v):.4g}"), "min": float(f"{np.min(v):.4g}"), "max": float(f"{np.max(v):.4g}")}
        for k in ("fw1", "fw20"):
            r[k + "_minus_dmc_us"] = float(f"{(np.mean(ts[k]) - np.mean(ts['dmc'])) * 1e3:.4g}")
        measured = {}
        for k, (_, state, fw) in runs.items():
            done = int(state.counter.item())
            assert done - first[k] == a.repeats * a.steps and int(state.status.item()) == 0
            measured[k] = {"generations": done}
            if fw is not None:
                counts = fw.counts.cpu().numpy()
                m = int(fw.measurements.item())
                assert m == done // fw.stride and counts[0, 0] + counts[0, 1] == m * B and (counts[:, 0] > 0).all()
                measured[k].update(measurements=m, counted_at_longest_lag=int(counts[SLOTS, 0]))
        r["measured"] = measured
        print(json.dumps(r), flush=True)
        del runs, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
